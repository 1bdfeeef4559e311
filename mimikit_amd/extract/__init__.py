from .from_neighbors import *
from .clusters import *
from .segment import *
from .samplify import *
