"""float64 restatements, seeded fixtures and derived bounds of the two harmonic spectrogram filters (include/mmk_spec_filter.h,
mimikit_amd/features/functionals.py AutoConvolve / F0Filter), shared by tests/test_spec_filter_refs.py (no GPU), tests/test_gpu_spec_filter.py
and tests/golden/make_golden_spec_filter.py.  Nothing here needs a GPU, librosa or the reference tree.

AutoConvolve.  p[t, b] is a product of k float64 factors (k - 1 roundings), z = log(1.0 + p) two more, the frame's sum of F non-negative
terms at most F - 1 more in any order, the division and the product with s two more: the float64 relative error of any fixed summation
order is at most (F + k + 8) 2^-52, far below 2^-24.  The float32 result therefore differs from the reference's rounded value by at most
one float32 ulp, and only where the float64 value lies that close to a rounding boundary: ulp_rule() - no element off by more than 1 ulp,
at most 1 element in 10 000 off at all.  auto_convolve64 adds the frame with math.fsum (the exact sum, rounded once).

F0Filter.  scipy's interp1d (what librosa.interp_harmonics calls) differs from the definition in two places: it subtracts the two float32
knots of a term in float32 before it goes to float64, and it may take an integer position's knot as the UPPER end of its bracket.  Per bin

    E_b = 2^-24 * sum |difference of the two knots of every term| + 2^-48 * sum |terms|

where an integer overtone position p counts the pair (p - 1, p) (p = 0: the pair (0, 1), scipy's bracket there), and an undertone with
r = 0 counts the pair (lo - 1, lo) as well as (lo, lo + 1).  The first part is the float32 rounding of a difference at its unit roundoff,
carried by an interpolation fraction of at most 1; the second is room for the float64 operations of either side (a few 2^-53 per term).
Propagation to the output, soft and normalised, with Y = sum y+ + 1e-8 and E = sum_b E_b:

    |d out_b| <= 1.01 z_b (E_b / Y + y+_b E / Y^2) + 2^-23 |out_b|

(the quotient rule to first order, 1 % for the second order, one float32 rounding and the float64 operations in the last term).  Soft and
not normalised: 1.01 z_b E_b + 2^-23 |out_b|.  The hard mask has no E_b term once |y_b| >= 4 E_b holds at every bin (min_gap): no decision
y > 0 can flip, the mask and its count are exact, and only the last term remains.
"""
import math

import numpy as np

MAX_BINS = 4097               # include/mmk_spec_filter.h: MMK_SPEC_FILTER_MAX_BINS
TILE_FRAMES = 4               # MMK_SPEC_FILTER_TILE_FRAMES
MAX_WINDOW = 64               # MMK_AUTO_CONVOLVE_MAX_WINDOW
MAX_OVERTONE = 16             # MMK_F0_FILTER_MAX_OVERTONE
MAX_UNDERTONE = 16            # MMK_F0_FILTER_MAX_UNDERTONE
MIN_GAP = 4.0                 # |y_b| >= MIN_GAP * E_b at every bin of a fixture
MODES = ((True, True), (True, False), (False, True), (False, False))        # (soft, normalize)

# ---- fixtures: name -> (seed, frames, bins) and what is recorded of each
F0_SHAPES = {"f1025": (0, 9, 1025), "f513": (1, 33, 513), "f65": (2, 6, 65), "f1026": (3, 5, 1026)}
F0_PARAMS = ((4, 4), (8, 6), (2, 9), (16, 16))
# the pairs whose scipy result is recorded (the file must stay below the size limit for a committed file; the generator holds EVERY shape
# x parameter pair, at the seeds 0 to 3, to its three conditions before it writes anything)
F0_RECORDED = {"f1025": F0_PARAMS, "f513": ((8, 6),), "f65": F0_PARAMS, "f1026": F0_PARAMS}
AC_SHAPES = {"a1025": (0, 7, 1025), "a513": (0, 40, 513), "a65": (0, 5, 65)}
# (the zero frame 2 lies in every window of 7 frames at k = 8: all zeros, which would show nothing)
AC_WINDOWS = {"a1025": (2, 3, 4, 5), "a513": (2, 3, 4, 5, 8), "a65": (2, 3, 4)}


def frames(seed, n_frames, bins):
    """|N(0, 1)| as float32 times a per-frame scale U(0.01, 30); frame 2 is zero, the upper half of frame 3 is zero"""
    rng = np.random.default_rng(seed)
    s = np.abs(rng.standard_normal((n_frames, bins))).astype(np.float32)
    s *= rng.uniform(0.01, 30.0, size=(n_frames, 1)).astype(np.float32)
    s[2] = 0.0
    s[3, bins // 2:] = 0.0
    return s


def f0_fixture(name):
    return frames(*F0_SHAPES[name])


def ac_fixture(name):
    return frames(*AC_SHAPES[name])


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


# ====================================================================================================================== AutoConvolve
def auto_convolve_numpy(s, k):
    """the reference's np_func line by line (float64 result); librosa.feature.stack_memory(x, n_steps=k, delay=-1, constant_values=1) is
    restated: x is padded by k - 1 columns of 1 on the right and block i of the stack at time t' is padded[t' + i]"""
    S = s
    x_padded = np.pad(S.T, ((0, 0), (k // 2, 0)), constant_values=1)
    t = x_padded.shape[1]
    data = np.pad(x_padded, ((0, 0), (0, k - 1)), constant_values=1)
    stacked = np.concatenate([data[:, i:i + t] for i in range(k)], axis=0)
    x_win = stacked[:, :-(k // 2)].reshape(k, *S.shape[::-1])
    z = np.log(1 + np.prod(x_win.astype(np.float64), axis=0)).T
    z = z / (z.sum(axis=1, keepdims=True) + 1e-8)
    return z * S


def auto_convolve64(s, k):
    """the definition of include/mmk_spec_filter.h with an exact frame sum -> float64 (T, F)"""
    n_frames, _ = s.shape
    z64 = s.astype(np.float64)
    out = np.empty_like(z64)
    for t in range(n_frames):
        p = np.ones(s.shape[1])
        for u in range(t - k // 2, t - k // 2 + k):
            if 0 <= u < n_frames:
                p = p * z64[u]
        z = np.log(1.0 + p)
        out[t] = z / (math.fsum(z) + 1e-8) * z64[t]
    return out


def ulp_rule(got32, want32, what):
    """no element differs by more than 1 float32 ulp, at most 1 in 10 000 differs at all (both non-negative) -> the number that differ"""
    got32, want32 = np.asarray(got32), np.asarray(want32)
    assert got32.dtype == np.float32 and want32.dtype == np.float32 and got32.shape == want32.shape, what
    assert np.isfinite(got32).all() and (bits(got32) >= 0).all(), f"{what}: a value is not finite or is negative"
    d = np.abs(bits(got32).astype(np.int64) - bits(want32).astype(np.int64))
    n = int((d > 0).sum())
    assert d.max() <= 1, f"{what}: {int((d > 1).sum())} elements differ by more than 1 ulp (worst {int(d.max())}, first at {tuple(int(a[0]) for a in np.nonzero(d > 1))})"
    assert n * 10000 <= d.size, f"{what}: {n} of {d.size} elements differ by one ulp, more than 1 in 10 000"
    return n


# ====================================================================================================================== F0Filter
def f0_parts64(s, n_overtone, n_undertone):
    """-> (y, E_b): the definition's y = sl - sl2 in float64 and the per-bin bound on scipy's distance from it (module docstring)"""
    z = s.astype(np.float64)
    n_bins = z.shape[1]
    b = np.arange(n_bins)
    sl, sl2 = np.zeros_like(z), np.zeros_like(z)
    diffs, terms = np.zeros_like(z), np.zeros_like(z)
    for h in range(1, n_overtone):
        p = h * b
        ok = p <= n_bins - 1
        q = p[ok]
        term = z[:, q]
        sl[:, ok] += term
        terms[:, ok] += np.abs(term)
        hi = np.maximum(q, 1)
        diffs[:, ok] += np.abs(z[:, hi] - z[:, hi - 1])
    for x in range(2, n_undertone):
        lo, r = b // x, b % x
        up = np.minimum(lo + 1, n_bins - 1)
        term = z[:, lo] + (z[:, up] - z[:, lo]) * (r / x)
        sl2 += term
        terms += np.abs(term)
        diffs += np.abs(z[:, up] - z[:, lo])
        below = np.maximum(lo - 1, 0)
        diffs += np.where(r == 0, np.abs(z[:, lo] - z[:, below]), 0.0)
    return sl - sl2, 2.0 ** -24 * diffs + 2.0 ** -48 * terms


def f0_from_y(s, y, soft, normalize):
    """the reference's last lines on a given y (float64 arithmetic) -> out float64"""
    y = y * (y > 0) if soft else (y > 0)
    if normalize:
        y = y / (y.sum(axis=1, keepdims=True) + 1e-8)
    return s.astype(np.float64) * y


def f0_filter64(s, n_overtone, n_undertone, soft, normalize):
    """-> (out float64, bound): the definition and the bound on the distance of scipy's (and the device's float32) output from it"""
    y, e_b = f0_parts64(s, n_overtone, n_undertone)
    z = s.astype(np.float64)
    yp = np.where(y > 0, y, 0.0) if soft else (y > 0).astype(np.float64)
    big_y = yp.sum(axis=1, keepdims=True) + 1e-8
    out = z * (yp / big_y if normalize else yp)
    bound = 2.0 ** -23 * np.abs(out)
    if soft and normalize:
        bound = bound + 1.01 * z * (e_b / big_y + yp * e_b.sum(axis=1, keepdims=True) / big_y ** 2)
    elif soft:
        bound = bound + 1.01 * z * e_b
    return out, bound


def min_gap(y, e_b):
    """the smallest |y_b| / E_b over the bins where E_b > 0 (inf if there is none); a bin with E_b = 0 must have y = 0 exactly on both
    sides or a gap of its own: it is a bin whose every knot is zero"""
    pos = e_b > 0
    assert (y[~pos] == 0).all(), "a bin without any error term has y != 0"
    return float((np.abs(y[pos]) / e_b[pos]).min()) if pos.any() else math.inf


def assert_inside(got, want, bound, what):
    """|got - want| <= bound everywhere -> the worst error / bound (0 / 0 counts as 0)"""
    err = np.abs(np.asarray(got, dtype=np.float64) - want)
    bad = err > bound
    assert not bad.any(), (f"{what}: {int(bad.sum())} of {bad.size} elements outside the bound, first at {tuple(int(a[0]) for a in np.nonzero(bad))}: "
                           f"error {err[bad][0]:.3e}, bound {bound[bad][0]:.3e}")
    return float(np.where(err > 0, err / np.maximum(bound, 1e-300), 0.0).max())
