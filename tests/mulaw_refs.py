"""Crafted inputs and expected codes for the mu-law kernels' tests, shared by test_mulaw_refs.py (CPU: the reference alone) and
test_gpu_mulaw_paths.py (the device against it).

The contract is the reference project's fp32 formula, oracle.torch_ref.mulaw_compress / mulaw_expand, evaluated on a whole tensor in one
call (torch's vectorised loop, which functionals.mulaw_edges was derived with).  It is NOT float64: the two disagree by one code on a share
of the threshold neighbours, by design (test_mulaw_refs.py measures it and holds it to one code).

A case is one (q_levels, compression).  Its crafted block holds every decision threshold of functionals.mulaw_edges(q, c) with its
neighbours up to +-2 ulp on the fp32 number line (clamped to [-1, 1]) and +-0, +-1, +-1e-45, +-FLT_MIN.  The block is tiled, shuffled with
a seeded permutation and kept as the case's `master`; the input of length n is master[:n], so the runs at 65535 and 65536 samples see the
same data.  Neighbouring samples then almost never share a code (test_mulaw_refs.py: at most 2 % at the offsets 1, 2, 4, 128, 256 from
q = 64 on), so a misdirected lane exchange or a shifted store cannot hide behind equal codes; the DEFECTS below are that statement's test.

Which kernel a case takes at length (csrc/features.hip, mmk_mulaw_compress_f32_i64; test_mulaw_refs.py reads the three constants from its
text): the stream kernel for q <= LDS_LEVELS / 2 from STREAM_MIN_N samples on, the general kernel with the table in LDS up to LDS_LEVELS,
with the table in global memory beyond."""
import functools
from typing import NamedTuple

import numpy as np
import torch

from mimikit_amd.features.functionals import mulaw_edges
from oracle import torch_ref as O

STREAM_MIN_N = 1 << 16             # n >= (1 << 16)
LDS_LEVELS = 8192                  # kMuLawLdsLevels
STREAM_MAX_Q = LDS_LEVELS // 2     # q_levels <= kMuLawLdsLevels / 2
STREAM_GRID_CAP = 8192             # workgroups of the stream kernel at most
STREAM_TILE = 1024                 # float4s per workgroup and round: 256 lanes x 4

CASES = [(2, 1.0), (3, 1.0), (64, 1.0), (256, 1.0), (256, 0.5), (1024, 2.0), (4096, 1.0), (4097, 1.0), (8192, 1.0), (8193, 1.0), (65536, 1.0)]
STREAM_CASES = [c for c in CASES if c[0] <= STREAM_MAX_Q]
PARTIAL_WAVE_N = 4 * (16384 + 37) + 2      # n4 % 64 = 37: the last wave is partial and keeps its own stores
WAVES_PAST_END_N = 4 * (16384 + 192)       # whole waves of the last workgroup lie past the end
LENGTHS = [STREAM_MIN_N - 1, STREAM_MIN_N, STREAM_MIN_N + 1, STREAM_MIN_N + 2, STREAM_MIN_N + 3, PARTIAL_WAVE_N, WAVES_PAST_END_N]
L_MAX = max(LENGTHS)
GRID_CAP_N4 = STREAM_GRID_CAP * STREAM_TILE + 64 * 5 + 3     # a second trip of the grid-stride loop: five whole waves and a partial one
GRID_CAP_N = 4 * GRID_CAP_N4 + 1
OFFSETS = (1, 2, 4, 128, 256)              # the distances a wrong exchange or store moves a code by
SPECIALS = np.array([0.0, -0.0, 1.0, -1.0, 1e-45, -1e-45, np.finfo(np.float32).tiny, -np.finfo(np.float32).tiny], dtype=np.float32)


# ---- the fp32 number line ------------------------------------------------------------------------------------------------------------------------------
def ordered_key(x: np.ndarray) -> np.ndarray:
    """monotone int64 key of fp32 values: consecutive floats have consecutive keys, +-0 share key 0"""
    bits = np.ascontiguousarray(x, dtype=np.float32).view(np.int32).astype(np.int64)
    return np.where(bits >= 0, bits, -(bits & 0x7FFFFFFF))


def from_key(k: np.ndarray) -> np.ndarray:
    k = np.asarray(k, dtype=np.int64)
    bits = np.where(k >= 0, k, (-k) | 0x80000000)
    return bits.astype(np.uint32).view(np.float32)


def step(x: np.ndarray, ulps: int) -> np.ndarray:
    """x moved by `ulps` places on the fp32 number line, clamped to [-1, 1]"""
    return np.clip(from_key(ordered_key(x) + ulps), -1.0, 1.0).astype(np.float32)


def ulp_distance(x: np.ndarray, edges: np.ndarray) -> np.ndarray:
    """places on the fp32 number line between every x and its nearest threshold"""
    kx, ke = ordered_key(x), ordered_key(edges)
    i = np.clip(np.searchsorted(ke, kx), 1, len(ke) - 1) if len(ke) > 1 else np.zeros(len(kx), dtype=np.int64)
    near = np.minimum(np.abs(kx - ke[i]), np.abs(kx - ke[i - 1])) if len(ke) > 1 else np.abs(kx - ke[0])
    return near


# ---- the crafted data ----------------------------------------------------------------------------------------------------------------------------------
def crafted_block(q: int, c: float, ulps: int = 2) -> np.ndarray:
    """every threshold with its neighbours up to +-`ulps` places, and the special values"""
    e = mulaw_edges(q, c).numpy()
    return np.concatenate([step(e, k) for k in range(-ulps, ulps + 1)] + [SPECIALS]).astype(np.float32)


def float64_codes(x: torch.Tensor, q: int, c: float) -> torch.Tensor:
    """the formula in float64 (NOT the contract: within one code of it)"""
    x = x.double()
    mu = q - 1.0
    y = torch.sign(x) * torch.log1p(mu * x.abs() * c) / np.log1p(mu * c)
    return ((y + 1) / 2 * mu + 0.5).to(torch.int64)


class Crafted(NamedTuple):
    q: int
    c: float
    edges: torch.Tensor       # (q - 1,) fp32, host
    block: torch.Tensor       # the shuffled crafted block (each value once)
    block_want: torch.Tensor
    x: torch.Tensor           # the master: the tiled block, shuffled; an input of length n is x[:n]
    want: torch.Tensor        # the oracle's codes of x, one call
    lengths: tuple


@functools.lru_cache(maxsize=None)
def crafted(q: int, c: float) -> Crafted:
    block = crafted_block(q, c)
    rng = np.random.default_rng(1000 * q + int(100 * c))
    reps = -(-L_MAX // len(block))
    master = np.tile(block, reps)
    master = master[rng.permutation(len(master))]
    shuffled = block[rng.permutation(len(block))]
    x, b = torch.from_numpy(master), torch.from_numpy(shuffled)
    # beyond the LDS table the block is longer than every length: the whole master is one more length, so that every code is asked for
    lengths = tuple(LENGTHS) + ((len(master),) if q > LDS_LEVELS else ())
    return Crafted(q, c, mulaw_edges(q, c), b, O.mulaw_compress(b, q, c), x, O.mulaw_compress(x, q, c), lengths)


def same_code_shares(codes: torch.Tensor) -> dict:
    """share of positions whose code equals the code `off` samples on, per offset"""
    return {off: float((codes[off:] == codes[:-off]).double().mean()) for off in OFFSETS}


# ---- defects, applied to the expected codes: what a subtly wrong stream kernel would write ----------------------------------------------------------
def defect_pair_swapped(d: Crafted, n: int) -> torch.Tensor:
    """samples 2 l and 2 l + 1 swapped: the two halves of an exchanged 16-byte store in the wrong order"""
    w = d.want[:n].clone()
    m = n & ~1
    w[:m] = w[:m].view(-1, 2).flip(1).reshape(-1)
    return w


def defect_halves_swapped(d: Crafted, n: int) -> torch.Tensor:
    """the two 128-sample halves of a wave's round swapped: store A fed from lanes 32.., store B from lanes 0.."""
    w = d.want[:n].clone()
    m = n - n % 256
    w[:m] = w[:m].view(-1, 2, 128).flip(1).reshape(-1)
    return w


def defect_table_one_ulp(d: Crafted, n: int) -> torch.Tensor:
    """`<` for `<=`: a sample on a threshold gets the code below"""
    return torch.bucketize(d.x[:n], d.edges, right=False)


def defect_high_byte_lost(d: Crafted, n: int) -> torch.Tensor:
    """the high half of a 16-bit pair lost on the way through the exchange"""
    return d.want[:n] & 0xFF


def defect_tail_from_start(d: Crafted, n: int) -> torch.Tensor:
    """the hand-off of the last n & 3 samples to the general kernel with the output pointer shifted and the input pointer not"""
    w = d.want[:n].clone()
    if n & 3:
        w[n - (n & 3):] = d.want[:n & 3]
    return w


DEFECTS = dict(pair_swapped=defect_pair_swapped, halves_swapped=defect_halves_swapped, table_one_ulp=defect_table_one_ulp,
               high_byte_lost=defect_high_byte_lost)


def changed_per_window(a: torch.Tensor, b: torch.Tensor, window: int = 256) -> torch.Tensor:
    """codes that differ in every whole window of `window` samples"""
    m = a.numel() - a.numel() % window
    return (a[:m] != b[:m]).view(-1, window).sum(1)


# ---- out-of-range and non-finite samples among lanes that exchange -----------------------------------------------------------------------------------
ONE_PLUS = float(np.nextafter(np.float32(1.0), np.float32(2.0)))
POKE_VALUES = (ONE_PLUS, -ONE_PLUS, 1.5, -1.5, 1e30, -1e30, float("inf"), float("-inf"), float("nan"))
POKE_LANES = (0, 31, 32, 63)
POKE_COMPONENTS = (0, 3)


def pokes(n: int):
    """[(sample index, value)]: one sample per wave and round of the stream kernel, so that the 63 other lanes of that wave - and the
    waves around it, which exchange - must stay exact.  A wave's round is 64 float4s; round r of the input is workgroup r // 16, round
    (r // 4) % 4 of it, wave r % 4.  Poke j goes to round (255 - 7 j) % 256: the last whole wave of both lengths first, every round 0..3 of
    a workgroup, many workgroups.  Then the partial wave (if n has one) and the samples the general kernel takes over."""
    n4 = n >> 2
    assert n4 // 64 == 256
    out, j = [], 0
    for v in POKE_VALUES:
        for lane in POKE_LANES:
            for comp in POKE_COMPONENTS:
                r = (255 - 7 * j) % 256
                out.append((4 * (64 * r + lane) + comp, v))
                j += 1
    rounds = {(((255 - 7 * i) % 256) // 4) % 4 for i in range(j)}
    assert rounds == {0, 1, 2, 3} and len({s for s, _ in out}) == j
    partial = n4 % 64
    if partial:
        for k, (lane, comp) in enumerate(((0, 0), (31, 3), (32, 0), (partial - 1, 3))):
            out.append((4 * (64 * 256 + lane) + comp, POKE_VALUES[(2 * k + 3) % len(POKE_VALUES)]))
    if n & 3:
        out.append((n - 1, -1.5))
    return out


# ---- expand ----------------------------------------------------------------------------------------------------------------------------------------------
def expand_codes(q: int, n: int) -> torch.Tensor:
    """all q codes and -2, -1, q, q + 1 scattered among them, n of them, shuffled"""
    rng = np.random.default_rng(q + n)
    codes = np.arange(n, dtype=np.int64) % q
    where = rng.choice(n, size=64, replace=False)
    codes = codes[rng.permutation(n)]
    keep = np.zeros(q, dtype=bool)                 # the scattered out-of-range codes must not take a code's only occurrence
    codes[where] = np.array([-2, -1, q, q + 1], dtype=np.int64)[np.arange(64) % 4]
    keep[codes[(codes >= 0) & (codes < q)]] = True
    assert keep.all()
    return torch.from_numpy(codes)
