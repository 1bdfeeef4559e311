from .from_neighbors import *
