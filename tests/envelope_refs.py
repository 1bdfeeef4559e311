"""float64 restatements, cases and derived error bounds of the envelope kernels (include/mmk.h: mmk_stft_energy_f32, mmk_interp1d_f32,
mmk_derivative_f32), shared by tests/test_envelope_refs.py (CPU) and tests/test_gpu_envelope.py.  In the style of tests/f64_bounds.py:
u = 2^-24, one constant per kernel, every bound derived from the roundings the computation makes, none fitted to what the GPU returns.

Energy.  out[f] = sum_k |S_f[k]|.  Each magnitude carries the bound of the spectral tests (f64_bounds.stft_err_bound, 'mag':
C_FFT fft_unit(frame) + 2 u |S|); summed over the n_fft/2 + 1 bins.  The reduction adds a lane's ceil(bins / lanes) magnitudes in turn, then
6 butterfly levels, then up to 3 joins of the waves: `depth` roundings, each relative to a partial sum of non-negative terms, so at most
depth u sum_k |S|.  Over the sizes the library takes, depth / sqrt(bins) is largest for n_fft = 64 (33 bins on 64 lanes: 1 + 6 = 7
against sqrt(33) = 5.7: 1.22) and falls from there (2048: 17 + 6 = 23 against 32.0); with a factor for orderings the kernel may choose
    C_ENERGY = 2:      bound[f] = sum_k (C_FFT unit_f + 2 u |S_f[k]|) + C_ENERGY u sqrt(bins) sum_k |S_f[k]|.

Interpolation.  Positions are exact: with align = 1 they are numpy's float64 linspace itself (the kernel forms double(i) * step and forces the
last one, as numpy does), with align = 0 the fp32 arithmetic of torch's CPU kernel (one fused multiply-add and a clamp), restated here in numpy; the restatement then
interpolates in float64.  The kernel rounds the weight once (align = 1: w = fl(pos - lo), u w), then  y_lo + w (y_hi - y_lo)  makes three
roundings, each of a value no larger than |y_lo| + |y_hi|;  align = 0:  fl(1 - l1) y_0 + l1 y_1  makes three as well (the weight
fl(1 - l1) is torch's own and is part of the restatement).  First order, at most 4 u (|y_lo| + |y_hi|):
    C_INTERP = 4:      bound[i] = C_INTERP u (|y_lo| + |y_hi|);       'previous' copies: exact.

Derivative.  With A[p] bounding |xp[p]| and the roundings that made it - |x[p]| inside the row (no rounding), 2 |x_end| + |x[m]| for a
reflected sample x_end + (x_end - x[m]) (two roundings, each of a value no larger than A: 2 u A) - a lag's term
fl(fl(1/d) fl(fl(xp[i+d] - x[i]) + fl(x[i] - xp[i-d]))) / 2 / L rounds five times (1/d to fp32, three sums, the product, the division by L;
the halving is exact) values no larger than S_d = A[i+d] + 2 |x[i]| + A[i-d] and inherits 2 u (A[i+d] + A[i-d]) from the reflection: at most
7.5 u S_d / (2 d L), rounded up
    C_DERIV = 8;
the running sum adds lag k to the sum of the lags before it, one rounding of a value no larger than P_k = sum_{d <= k} S_d / (2 d L):
    bound[i] = C_DERIV u sum_d S_d / (2 d L) + u sum_{k = 2 .. L} P_k.
tests/test_envelope_refs.py measures the sequential fp32 restatements against these bounds (worst error / bound over the cases: energy of
torch's fp32 rfft 0.034, interpolation 0.46 / 0.32 (align 1 / 0), derivative 0.17) and holds every bound to the near misses below.
"""
import functools
import math

import numpy as np
import torch

from mimikit_amd import native
from tests import f64_bounds as B

U = B.U
C_ENERGY = 2.0
C_INTERP = 4.0
C_DERIV = 8.0
TILE, MAX_LAG = native.DERIV_TILE, native.DERIV_MAX_LAG


@functools.lru_cache(maxsize=None)
def case_input(n, seed=0):
    """(3, n) float32 in [-1, 1), seeded by the length; a batch of 1 is its first row"""
    x = np.random.default_rng(7940 + 31 * seed + n).uniform(-1.0, 1.0, size=(3, n)).astype(np.float32)
    x.setflags(write=False)
    return x


# ------------------------------------------------------------------------------------------------------------------------ energy
def energy_cases(n_fft):
    """(hop, center, reflect, n_samples): a hop that divides n_fft and one that does not; centred with reflection, centred with zeros, not
    centred; the least input reflection allows (n_fft / 2 + 1) and lengths of 1, 2 and 67 frames (with reflection: 67, and what the least
    input gives)"""
    cases = []
    for hop in (n_fft // 4, n_fft // 4 + 3):
        cases += [(hop, 1, 1, n_fft // 2 + 1), (hop, 1, 1, 66 * hop + 1)]
        cases += [(hop, 1, 0, hop - 1), (hop, 1, 0, hop), (hop, 1, 0, 66 * hop + 2)]
        cases += [(hop, 0, 0, n_fft), (hop, 0, 0, n_fft + hop), (hop, 0, 0, n_fft + 66 * hop + hop - 1)]
    return cases


def n_frames(n, n_fft, hop, center):
    return 1 + (n + (2 * (n_fft // 2) if center else 0) - n_fft) // hop


def energy_ref(x64, n_fft, hop, center, reflect, defect=None):
    """x64 (B, n) float64 tensor -> want (B, frames), bound (B, frames).  Defects: 'shift' (every frame starts one sample late), 'symmetric'
    (a symmetric Hann window), 'nyquist' (the sum skips the last bin)"""
    pad = "reflect" if reflect else "constant"
    S, fw = B.stft_ref(x64, n_fft, hop, bool(center), pad, window=B.hann64(n_fft, periodic=False) if defect == "symmetric" else None,
                       shift=1 if defect == "shift" else 0)
    mag = S.abs()
    bins = n_fft // 2 + 1
    want = (mag[..., :-1] if defect == "nyquist" else mag).sum(-1)
    total = mag.sum(-1)
    bound = bins * B.C_FFT * B.fft_unit(fw, n_fft) + 2 * U * total + C_ENERGY * U * math.sqrt(bins) * total
    return want, bound


@functools.lru_cache(maxsize=None)
def energy_reference(n_fft, hop, center, reflect, n):
    want, bound = energy_ref(torch.from_numpy(case_input(n).astype(np.float64)), n_fft, hop, center, reflect)
    return want.numpy(), bound.numpy()


# ----------------------------------------------------------------------------------------------------------------- interpolation
INTERP_SIZES = ((2, 1), (2, 5), (7, 7), (300, 4097), (100, 13))


def interp_positions(n, n_out, align):
    """-> lo, hi (int64), w_hi, w_lo (float64): out = w_lo y[lo] + w_hi y[hi].  align 1: numpy's linspace; align 0: torch's CPU kernel, fp32"""
    if align:
        pos = np.linspace(0, n - 1, n_out)
        lo = np.minimum(np.floor(pos).astype(np.int64), n - 1)
        hi = np.minimum(lo + 1, n - 1)
        w = pos - lo
        return lo, hi, w, 1.0 - w
    if n_out == n:
        i = np.arange(n)
        return i, i, np.zeros(n), np.ones(n)
    scale = np.float32(n) / np.float32(n_out)
    # one fused multiply-add, as torch's vectorised CPU build makes it: the product of two floats is exact in float64
    src = (np.float64(scale) * (np.arange(n_out, dtype=np.float32) + np.float32(0.5)).astype(np.float64) - 0.5).astype(np.float32)
    src = np.maximum(src, np.float32(0))
    lo = np.minimum(src.astype(np.int64), n - 1)
    hi = lo + (lo < n - 1)
    l1 = np.clip(src - lo.astype(np.float32), np.float32(0), np.float32(1))
    l0 = np.float32(1) - l1
    return lo, hi, l1.astype(np.float64), l0.astype(np.float64)


def interp_ref(x, n_out, mode="linear", align=1, dtype=np.float64):
    """x (..., n) -> (..., n_out) in `dtype` (float64: the reference; float32: the kernel's operations, each rounded) and the bound"""
    n = x.shape[-1]
    lo, hi, w_hi, w_lo = interp_positions(n, n_out, align)
    a, b = x[..., lo].astype(dtype), x[..., hi].astype(dtype)
    if mode == "previous":
        return a, np.zeros(a.shape)
    bound = C_INTERP * U * (np.abs(a) + np.abs(b)).astype(np.float64)
    if align:
        return a + w_hi.astype(dtype) * (b - a), bound
    return w_lo.astype(dtype) * a + w_hi.astype(dtype) * b, bound


# -------------------------------------------------------------------------------------------------------------------- derivative
DERIV_CASES = ((1, 2), (3, 4), (9, 10), (33, 5000), (3, TILE - 1), (3, TILE), (3, TILE + 1), (MAX_LAG, MAX_LAG + 1), (MAX_LAG, 2 * TILE + 5))


def reflect_pad(x, L, even=False):
    """odd reflection of the last axis about its ends by L samples (even: the defect x[m] instead of x[0] + (x[0] - x[m]))"""
    head, tail = x[..., 1:L + 1][..., ::-1], x[..., -L - 1:-1][..., ::-1]
    if even:
        return np.concatenate([head, x, tail], -1)
    return np.concatenate([x[..., :1] + (x[..., :1] - head), x, x[..., -1:] + (x[..., -1:] - tail)], -1)


def derivative_ref(x, L, defect=None):
    """x (..., n), n > L -> (..., n) in x's dtype: float64 the reference, float32 the sequential restatement of the kernel.  Defects: 'even'
    (an even reflection), 'no_1/d' (the lag weight is dropped)"""
    n, dt = x.shape[-1], x.dtype.type
    xp = reflect_pad(x, L, even=defect == "even")
    acc = np.zeros(x.shape, dtype=x.dtype)
    for d in range(1, L + 1):
        b, a = xp[..., L + d:L + d + n], xp[..., L - d:L - d + n]
        w = dt(1.0) if defect == "no_1/d" else dt(1.0 / d)
        acc = acc + (w * ((b - x) + (x - a))) / dt(2) / dt(L)
    return acc


def derivative_bound(x64, L):
    n = x64.shape[-1]
    ax = np.abs(x64)
    head, tail = ax[..., 1:L + 1][..., ::-1], ax[..., -L - 1:-1][..., ::-1]
    A = np.concatenate([2 * ax[..., :1] + head, ax, 2 * ax[..., -1:] + tail], -1)
    total, chain = np.zeros(x64.shape), np.zeros(x64.shape)
    for d in range(1, L + 1):
        total = total + (A[..., L + d:L + d + n] + 2 * ax + A[..., L - d:L - d + n]) / (2 * d * L)
        if d >= 2:
            chain = chain + total
    return C_DERIV * U * total + U * chain


@functools.lru_cache(maxsize=None)
def derivative_reference(L, n):
    x64 = case_input(n, seed=L).astype(np.float64)
    return derivative_ref(x64, L), derivative_bound(x64, L)


def outside(got, want, bound):
    """elements of `got` outside the bound (NaN counts as outside)"""
    return ~(np.abs(np.asarray(got, dtype=np.float64) - want) <= bound)


def worst_ratio(got, want, bound):
    return float(np.max(np.abs(np.asarray(got, dtype=np.float64) - want) / np.maximum(bound, 1e-300)))


def assert_inside(got, want, bound, what):
    bad = outside(got, want, bound)
    if bad.any():
        i = tuple(int(a[0]) for a in np.nonzero(bad))
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.size} elements outside the derived bound; at {i}: got {float(got[i]):.9g}, "
                             f"want {want[i]:.9g}, error {abs(float(got[i]) - want[i]):.3e} > bound {bound[i]:.3e}")
    return worst_ratio(got, want, bound)
