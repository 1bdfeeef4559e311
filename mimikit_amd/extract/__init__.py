from .from_neighbors import *
from .clusters import *
