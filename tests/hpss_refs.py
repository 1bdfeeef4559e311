"""Restatements, cases and derived error bounds of the HPSS kernel (include/mmk.h: mmk_hpss_f32), shared by tests/test_hpss_refs.py (CPU)
and tests/test_gpu_hpss.py.  numpy only.  In the style of tests/f64_bounds.py: u = 2^-24, every bound derived from the roundings the
kernel makes, none fitted to what the GPU returns.

Medians.  median_reflect is the rule scipy.ndimage.median_filter(mode="reflect") follows while size // 2 <= n (tests/test_hpss_refs.py holds
it to scipy's own results in tests/golden/hpss.npz): a window of s at i covers i - s//2 .. i - s//2 + s - 1, the result is its element of
rank s//2, indices outside fold by half-sample reflection.  A selection: compared bit for bit.

Masks.  hpss64 takes the exact medians, rounds the two products perc * margin_harm and harm * margin_perc to float32 as the kernel and
numpy do (so Z = max(X, R), the `bad` test and the hard mask X > R see the very numbers the kernel sees: no branch can differ), and computes
the rest in float64.  The kernel then rounds, with relative error u each:
    m = fl(X / Z), r = fl(R / Z)        one of the two is exactly 1 (Z is X or R)
    m^p, r^p                             powf: p times the quotient's error, and 4 u of its own (libm: a few ulp); 1^p = 1; not taken for p = 1
    fl(m + r)                            both terms are non-negative: the sum's relative error is the larger of theirs, and u
    fl(m / (m + r)), fl(S * mask)        u each
so out carries C(p) = 2 (p + 4) + 3 roundings' worth for p != 1, and C(1) = 2 + 3 = 5:
    bound = gamma(C) |out| + S (e_m + 2 e0) + e0,     gamma(C) = C u / (1 - C u),
where the second part is for results below the normal range, whose rounding is absolute, e0 = 2^-150 (half the smallest subnormal): the
quotient m or r carries e0, which powf turns into at most e_m = p e0 for p >= 1 (m <= 1, slope <= p) and e0^p for p < 1 (concavity:
(a + e)^p - a^p <= e^p); powf's result and the mask carry e0 each (d mask / dm and d mask / dr are at most 1 because m + r >= 1); the product e0.
Where `bad` holds the mask is 0.5 or 0 and only the product rounds.  The hard mask (p = inf) is S or 0: compared bit for bit.
"""
import functools

import numpy as np

U = 2.0 ** -24
E0 = 2.0 ** -150
TINY = np.finfo(np.float32).tiny
WINDOWS = (1, 2, 3, 4, 17, 31, 32, 63)
POWERS = (1.0, 2.0, 0.5)
MARGINS = (1.0, 1.5, (1.0, 3.0))
DEFECTS = ("swapped_axes", "lower_median", "window_right", "clamped_edge", "whole_sample", "margin_side", "no_split_zeros", "tiny_zero",
           "crosses_clips")


def pair(v):
    return tuple(v) if isinstance(v, (tuple, list)) else (v, v)


def median_reflect(x, s, axis, defect=None):
    """running median of `x` along `axis` by scipy's rule.  Defects: 'lower_median' (rank (s - 1) // 2), 'window_right' (the window one to
    the right), 'clamped_edge' (the edge value repeated), 'whole_sample' (d c b | a b c d | c b a)"""
    x = np.moveaxis(np.asarray(x), axis, -1)
    n = x.shape[-1]
    if s // 2 > n:
        raise ValueError(f"median_reflect: a window of {s} folds an axis of {n} more than once")
    left = s // 2 - (1 if defect == "window_right" else 0)
    right = s - 1 - left
    mode = {"clamped_edge": "edge", "whole_sample": "reflect"}.get(defect, "symmetric")
    xp = np.pad(x, [(0, 0)] * (x.ndim - 1) + [(max(left, 0), right)], mode=mode)
    if left < 0:
        xp = xp[..., 1:]
    win = np.lib.stride_tricks.sliding_window_view(xp, s, axis=-1)
    rank = (s - 1) // 2 if defect == "lower_median" else s // 2
    med = np.partition(win, rank, axis=-1)[..., rank]
    return np.moveaxis(med, -1, axis)


def medians(S32, kernel_size, defect=None):
    """S32 (..., frames, bins) -> (harm, perc): every bin along time, every frame along frequency"""
    win_harm, win_perc = pair(kernel_size)
    S = np.asarray(S32, dtype=np.float32)
    if defect == "swapped_axes":
        return median_reflect(S, win_harm, -1), median_reflect(S, win_perc, -2)
    if defect == "crosses_clips" and S.ndim == 3:
        flat = S.reshape(-1, S.shape[-1])
        return median_reflect(flat, win_harm, -2).reshape(S.shape), median_reflect(S, win_perc, -1)
    d = defect if defect in ("lower_median", "window_right", "clamped_edge", "whole_sample") else None
    return median_reflect(S, win_harm, -2, d), median_reflect(S, win_perc, -1, d)


def softmask64(X, R, power, split_zeros, tiny=TINY):
    """X, R float32 -> the mask in float64 (p = inf: 0 or 1), and where `bad` held"""
    X64, R64 = X.astype(np.float64), R.astype(np.float64)
    if np.isinf(power):
        return (X > R).astype(np.float64), np.zeros(X.shape, dtype=bool)
    Z = np.maximum(X64, R64)
    bad = Z < tiny
    Z = np.where(bad, 1.0, Z)
    with np.errstate(invalid="ignore", divide="ignore"):
        m, r = (X64 / Z) ** power, (R64 / Z) ** power
        mask = m / (m + r)
    return np.where(bad, 0.5 if split_zeros else 0.0, mask), bad


def hpss64(S32, kernel_size=31, power=1.0, margin=1.0, defect=None):
    """S32 (..., frames, bins) float32 -> harmonic, percussive (float64), harm_median, perc_median (float32), and `bad` of either mask"""
    S = np.asarray(S32, dtype=np.float32)
    margin_harm, margin_perc = (np.float32(m) for m in pair(margin))
    if margin_harm < 1 or margin_perc < 1 or not power > 0:
        raise ValueError("hpss64: margins must be at least 1 and power positive")
    harm, perc = medians(S, kernel_size, defect)
    split = bool(margin_harm == 1 and margin_perc == 1) and defect != "no_split_zeros"
    tiny = 0.0 if defect == "tiny_zero" else TINY
    if defect == "margin_side":
        mh, bad_h = softmask64(harm * margin_harm, perc, power, split, tiny)
        mp, bad_p = softmask64(perc * margin_perc, harm, power, split, tiny)
    else:
        mh, bad_h = softmask64(harm, perc * margin_harm, power, split, tiny)          # (float32 products)
        mp, bad_p = softmask64(perc, harm * margin_perc, power, split, tiny)
    S64 = S.astype(np.float64)
    return S64 * mh, S64 * mp, harm, perc, bad_h | bad_p


def roundings(power):
    return 5.0 if power == 1 else 2.0 * (power + 4.0) + 3.0


def hpss_bound(out64, S32, power):
    """the bound of a soft output against hpss64 (finite power)"""
    c = roundings(power) * U
    e_m = power * E0 if power >= 1 else E0 ** power
    return c / (1.0 - c) * np.abs(out64) + np.asarray(S32, dtype=np.float64) * (e_m + 2 * E0) + E0


# ------------------------------------------------------------------------------------------------------------------------- cases
KINDS = ("uniform", "ties", "zeros", "constant")


@functools.lru_cache(maxsize=None)
def case_input(kind, batch, frames, bins):
    """(batch, frames, bins) float32, non-negative, seeded by kind and shape; every clip has its own content.
    'ties': four levels; 'zeros': a band of frames of exact zeros with single bins left standing in it (both medians vanish under a live bin:
    the `bad` branch with S > 0), a band of bins below the normal range; 'constant': one frame and one bin constant"""
    rng = np.random.default_rng(7360 + 1000003 * KINDS.index(kind) + 101 * frames + bins)
    x = rng.uniform(0.0, 1.0, size=(batch, frames, bins)).astype(np.float32)
    if kind == "ties":
        x = (np.floor(x * 4) / 4).astype(np.float32)
    elif kind == "zeros":
        f0, f1, b0, b1 = frames // 8, max(3 * frames // 4, 1), bins // 4, bins // 2 + 1      # (more than half a window of 31 at 40 frames)
        x[:, :, b0:b1] *= np.float32(1e-39)
        x[:, f0:f1, :] = 0.0
        x[:, (f0 + f1) // 2, ::5] = np.float32(0.75)
        x[:, (f0 + f1) // 2, 1::5] = np.float32(3e-40)
    elif kind == "constant":
        x[:, frames // 2, :] = np.float32(0.25)
        x[:, :, bins // 2] = np.float32(0.5)
    x.setflags(write=False)
    return x


def tile_shapes(tile_frames, tile_bins):
    return [(f, b) for f in (tile_frames - 1, tile_frames, tile_frames + 1, 2 * tile_frames + 1) for b in (tile_bins - 1, tile_bins + 1)]


# (frames, bins) -> the (win_harm, win_perc) run on it: the largest windows the small axes allow (s // 2 == n and s // 2 == n - 1)
SMALL_CASES = {(1, 1): ((1, 1), (2, 3), (3, 2)), (15, 15): ((31, 30), (30, 31), (29, 28), (28, 29)), (16, 16): ((33, 32), (32, 33), (31, 30), (30, 31))}
TILE_WINDOWS = tuple((w, w) for w in WINDOWS) + ((31, 5), (4, 63))
LARGE_CASES = {(37, 1025): ((31, 31), (4, 63), (63, 17)), (300, 513): ((31, 31), (63, 32), (17, 5))}


@functools.lru_cache(maxsize=None)
def reference(kind, batch, frames, bins, kernel_size, power=1.0, margin=1.0):
    out = hpss64(case_input(kind, batch, frames, bins), kernel_size, power, margin)
    for a in out:
        a.setflags(write=False)
    return out


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float32), np.ascontiguousarray(b, dtype=np.float32)
    return a.shape == b.shape and bool(np.array_equal(a.view(np.uint32), b.view(np.uint32)))


def outside(got, want, bound):
    """elements of `got` outside the bound (NaN counts as outside)"""
    return ~(np.abs(np.asarray(got, dtype=np.float64) - want) <= bound)


def assert_inside(got, want, bound, what):
    bad = outside(got, want, bound)
    if bad.any():
        i = tuple(int(a[0]) for a in np.nonzero(bad))
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.size} elements outside the derived bound; at {i}: got {float(got[i]):.9g}, "
                             f"want {want[i]:.9g}, error {abs(float(got[i]) - want[i]):.3e} > bound {bound[i]:.3e}")
    return float(np.max(np.abs(np.asarray(got, dtype=np.float64) - want) / bound))
