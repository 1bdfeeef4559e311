"""The weight fingerprint (csrc/linear.hip: fingerprint_word, fingerprint_kernel) restated in numpy, shared by test_fingerprint_refs.py
(CPU) and test_gpu_fingerprint.py (the device against it).

A word w at position pos of the concatenated buffers contributes
    h = (w ^ (pos * 0x9E3779B1)) * 0x85EBCA77;  h ^= h >> 15;  h *= 0xC2B2AE3D;  (h ^ (h >> 13)) + (w << 20)
with h in 32-bit arithmetic and the sum of the two terms, and of all words, in 64-bit arithmetic.  The positions run through the buffers in
order (mod 2^32).  Here every intermediate is a uint64 masked to the width the kernel computes it in; the device's number is read back as
int64 and compared mod 2^64."""
import numpy as np
import torch

M32 = np.uint64(0xFFFFFFFF)
MAX_BUFFERS = 96                  # kFpMaxBuffers: buffers per launch; positions continue across launches


def words(x) -> np.ndarray:
    """the 32-bit words of a tensor or an array of a 4-byte dtype, as uint32"""
    if isinstance(x, torch.Tensor):
        x = x.detach().cpu().contiguous().numpy()
    return np.ascontiguousarray(x).reshape(-1).view(np.uint32)


def fingerprint(w: np.ndarray, pos0: int = 0) -> int:
    """of the uint32 words `w`, the first of which stands at position pos0"""
    w = np.asarray(w, dtype=np.uint32).astype(np.uint64)
    pos = (np.arange(w.size, dtype=np.uint64) + np.uint64(pos0 % 2 ** 32)) & M32
    h = ((w ^ ((pos * np.uint64(0x9E3779B1)) & M32)) * np.uint64(0x85EBCA77)) & M32
    h ^= h >> np.uint64(15)
    h = (h * np.uint64(0xC2B2AE3D)) & M32
    terms = (h ^ (h >> np.uint64(13))) + (w << np.uint64(20))
    return int(np.add.reduce(terms, dtype=np.uint64)) if w.size else 0        # (uint64 sums wrap: mod 2^64)


def fingerprint_buffers(buffers) -> int:
    """of several buffers: the fingerprint of their concatenation"""
    total, pos = 0, 0
    for b in buffers:
        b = words(b)
        total = (total + fingerprint(b, pos)) % 2 ** 64
        pos += b.size
    return total


def unsigned(v: int) -> int:
    """the device's int64 read-back mod 2^64"""
    return int(v) % 2 ** 64
