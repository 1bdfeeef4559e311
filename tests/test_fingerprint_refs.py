"""CPU side of the weight fingerprint's tests: the numpy restatement of tests/fingerprint_refs.py against a word-by-word evaluation in
Python integers, its behaviour over concatenations, and the constants it shares with csrc/linear.hip."""
import os
import re

import numpy as np
import torch

from tests import fingerprint_refs as R

HERE = os.path.dirname(os.path.abspath(__file__))
SOURCE = os.path.join(os.path.dirname(HERE), "mimikit_amd", "csrc", "linear.hip")


def _word(w, pos):
    """fingerprint_word in Python integers"""
    h = ((w ^ ((pos * 0x9E3779B1) & 0xFFFFFFFF)) * 0x85EBCA77) & 0xFFFFFFFF
    h ^= h >> 15
    h = (h * 0xC2B2AE3D) & 0xFFFFFFFF
    return (h ^ (h >> 13)) + (w << 20)


def _rand(n, seed):
    return np.random.default_rng(seed).integers(0, 2 ** 32, size=n, dtype=np.uint64).astype(np.uint32)


def test_restatement_word_by_word():
    w = np.concatenate([_rand(300, 1), np.array([0, 1, 0xFFFFFFFF, 0x80000000], dtype=np.uint32)])
    for pos0 in (0, 7, 2 ** 32 - 100, 2 ** 32 + 5):
        want = sum(_word(int(v), (pos0 + i) % 2 ** 32) for i, v in enumerate(w)) % 2 ** 64
        assert R.fingerprint(w, pos0) == want
    assert R.fingerprint(np.zeros(0, dtype=np.uint32)) == 0
    big = np.full(1 << 13, 0xFFFFFFFF, dtype=np.uint32)               # 2^13 terms of about 2^52: the sum wraps
    assert R.fingerprint(big) == sum(_word(0xFFFFFFFF, i) for i in range(big.size)) % 2 ** 64


def test_concatenation_is_the_sum_of_the_parts_at_their_positions():
    w = _rand(50000, 2)
    cuts = [0, 0, 1, 6, 8199, 8199, 28199, 50000]
    parts = [w[a:b] for a, b in zip(cuts[:-1], cuts[1:])]
    assert sum(R.fingerprint(p, a) for p, a in zip(parts, cuts[:-1])) % 2 ** 64 == R.fingerprint(w)
    assert R.fingerprint_buffers(parts) == R.fingerprint(w)
    assert R.fingerprint_buffers([torch.from_numpy(p.view(np.float32).copy()) for p in parts]) == R.fingerprint(w)
    assert R.fingerprint_buffers(parts[::-1]) != R.fingerprint(w)


def test_zeros_do_not_hash_to_zero_and_changes_move_the_number():
    for n in (1, 3, 4, 5, 8192, 8193):
        z = np.zeros(n, dtype=np.uint32)
        assert (R.fingerprint(z) != 0) == (n > 1)                         # (word 0 at position 0 is the one term that is 0)
        assert R.fingerprint(z, 1) != 0
    w = _rand(8197, 3)
    base = R.fingerprint(w)
    for i, bit in ((0, 0), (0, 31), (8196, 0), (8196, 31), (8193, 12), (4000, 22)):
        v = w.copy()
        v[i] ^= np.uint32(1 << bit)
        assert R.fingerprint(v) != base, (i, bit)
    v = w.copy()
    v[[100, 101]] = v[[101, 100]]
    assert R.fingerprint(v) != base
    assert R.fingerprint(np.roll(w, 1)) != base and R.fingerprint(w[1:], 0) != R.fingerprint(w[1:], 1)
    assert R.unsigned(-1) == 2 ** 64 - 1 and R.unsigned(5) == 5


def test_constants_are_the_kernels():
    text = open(SOURCE).read()
    body = text[text.index("fingerprint_word(uint32_t w, uint32_t pos)"):]
    body = body[:body.index("}")]
    assert "(w ^ (pos * 0x9E3779B1u)) * 0x85EBCA77u" in body and "h ^= h >> 15" in body and "h *= 0xC2B2AE3Du" in body
    assert "(h ^ (h >> 13)) + ((unsigned long long)w << 20)" in body
    assert int(re.search(r"constexpr int kFpMaxBuffers = (\d+);", text).group(1)) == R.MAX_BUFFERS
