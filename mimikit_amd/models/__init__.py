from .ensemble_generator import *
from .nnn import *
