"""numpy / scipy restatement, seeded fixtures and bounds of the spline and onset-cut kernels (include/mmk_samplify.h) and of
mimikit_amd.Samplifyer, shared by tests/test_samplify_refs.py (no GPU), tests/test_gpu_samplify.py and tests/golden/make_golden_samplify.py.
Nothing here touches the GPU.

The reference (mimikit/extract/samplify.py) needs numba and librosa, which are not installed; its algorithm is restated here in plain numpy:
attack_decay (:56-70), Samplifyer.fit II-III (:234-262), left_right_scores (:75-85), _refine (:89-96), refine_cuts (:102-122) and
librosa.zero_crossings(pad=True) without its clipping of |y| <= 1e-10.  The selection takes float32 `envs` / `grads` arrays - scipy's, or the
device's own materialised ones, in which case every decision is the same arithmetic on the same bits and the comparison is exact.

The bound of a spline value.  With u = 2^-24 (float32) and v = 2^-53 (float64), y the float32 knots of a row and s the value scipy's
interp1d(kind="quadratic") returns in float64:
  * both sides solve A c = y in float64 for a tridiagonal, strictly diagonally dominant A (rows (1/8, 3/4, 1/8), (1/10, 31/40, 1/8),
    (1/9, 28/45, 4/15), identity) with |A|_inf = 1 and |A^-1|_inf <= 1 / min_i (|a_ii| - sum_j |a_ij|) = 45 / 11 < 4.1.  Elimination without
    pivoting on such a matrix has a backward error below 8 v |A| (Higham, Accuracy and Stability, 9.13), so each side's c is off by at most
    8 * 4.1 v |c|_inf <= 8 * 4.1^2 v |y|_inf = 135 v |y|_inf; the device's truncation of the system at +-32 rows adds 1e-23 |y|_inf;
  * both sides evaluate three basis values from de Boor's recurrence (six roundings each, all terms positive) and sum three products:
    below 16 v |c|_inf <= 66 v |y|_inf each;
  * the device rounds the result to float32 once: u |s'|, s' within the float64 term of s.
So |device - s| <= u |s| + SPLINE_C64 v |y|_inf with SPLINE_C64 = 2 * (135 + 66) rounded up to 512."""
import functools
import os

import numpy as np
import scipy.interpolate as SI
import torch

from tests import envelope_refs as ER

U = 2.0 ** -24
V = 2.0 ** -53
SPLINE_C64 = 512.0
MAX_WINDOW = 2000            # include/mmk_samplify.h: MMK_SAMPLIFY_MAX_WINDOW
GOLDEN_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "samplify.npz")


# ------------------------------------------------------------------------------------------------------------------------- the spline
def knots(n):
    """scipy's not-a-knot vector of make_interp_spline(k=2) on the sites 0 .. n - 1"""
    return np.r_[(0.0,) * 3, np.arange(1.5, n - 2, 1.0), (float(n - 1),) * 3]


def positions(n, n_out):
    return np.linspace(0, n - 1, n_out)


def spline_ref(y, n_out):
    """y (..., n >= 3) -> scipy's interp1d(kind="quadratic") at linspace(0, n - 1, n_out) in float64, and the bound of the module docstring"""
    y64 = np.asarray(y, dtype=np.float64)
    n = y64.shape[-1]
    s = SI.interp1d(np.arange(n), y64, kind="quadratic", axis=-1, assume_sorted=True)(positions(n, n_out))
    return s, U * np.abs(s) + SPLINE_C64 * V * np.abs(y64).max(axis=-1, keepdims=True)


def collocation(n):
    """the (n, n) collocation matrix of the knot vector, dense"""
    return SI.BSpline.design_matrix(np.arange(n, dtype=np.float64), knots(n), 2).toarray()


def near_miss(y, n_out, which):
    """what a plausible mistake computes instead (float64)"""
    y64 = np.asarray(y, dtype=np.float64)
    n = y64.shape[-1]
    pos = positions(n, n_out)
    if which == "linear":
        return SI.interp1d(np.arange(n), y64, kind="linear")(pos)
    if which == "interior_rows":           # (1/8, 3/4, 1/8) in every row but the two identity rows
        A = np.diag(np.full(n, 0.75)) + np.diag(np.full(n - 1, 0.125), 1) + np.diag(np.full(n - 1, 0.125), -1)
        A[0], A[-1] = 0.0, 0.0
        A[0, 0] = A[-1, -1] = 1.0
        return SI.BSpline(knots(n), np.linalg.solve(A, y64), 2)(pos)
    if which == "align0":                  # torch's align_corners=False positions
        p = np.clip((np.arange(n_out) + 0.5) * (n / n_out) - 0.5, 0, n - 1)
        return SI.interp1d(np.arange(n), y64, kind="quadratic")(p)
    if which == "natural":                 # knots at the sites and a vanishing second derivative at the left end
        return SI.make_interp_spline(np.arange(n), y64, k=2, bc_type=([(2, 0.0)], None))(pos)
    raise KeyError(which)


NEAR_MISSES = ("linear", "interior_rows", "align0", "natural")


# ----------------------------------------------------------------------------------------------------------------------- the selection
def attack_decay(g):
    """reference :56-70 on a float32 row -> (att, dec) int64"""
    g = np.asarray(g)
    T = g.shape[-1]
    att = ((g[:-1] < 0) & (g[1:] > 0)).nonzero()[0] + 1
    dec = np.zeros_like(att)
    nxt = np.concatenate((att[1:], np.array([T - 1], dtype=att.dtype)))
    for k, (a, b) in enumerate(zip(att, nxt)):
        m = (g[a:b - 1] > 0) & (g[a + 1:b] < 0) if b - 1 > a else np.zeros(0, dtype=bool)
        dec[k] = m.nonzero()[0][0] + a if m.any() else T - 1
    return att.astype(np.int64), dec.astype(np.int64)


def zero_crossings(y):
    z = np.empty(y.shape[0], dtype=bool)
    z[0] = True
    z[1:] = np.signbit(y[1:]) != np.signbit(y[:-1])
    return z


def left_right(ce, fe, cuts, windows):
    """-> (count, 2) float32: the maxima of ce - fe over [max(c - w, 0), c) and [c, min(c + w, T)); an empty window is -inf"""
    out = np.full((len(cuts), 2), -np.inf, dtype=np.float32)
    for k, (c, w) in enumerate(zip(cuts, windows)):
        lo, hi = max(c - w, 0), min(c + w, ce.shape[0])
        if c > lo:
            out[k, 0] = (ce[lo:c] - fe[lo:c]).max()
        if hi > c:
            out[k, 1] = (ce[c:hi] - fe[c:hi]).max()
    return out


def objective(e, g):
    """0.9 * double(e) + 0.1 * (1.0 - double(g)), every operation rounded (numpy does not fuse)"""
    return 0.9 * e.astype(np.float64) + 0.1 * (1.0 - g.astype(np.float64))


def refine_step(c, d, e, g, be=None, bg=None):
    """reference :89-96 -> (c, d, robust): robust = the argmin and the argmax winners lead their runners-up by more than twice the largest
    bound of the values compared (be / bg: the bounds of e and g, or None)"""
    if c == d:
        return c, d, True
    obj, ee = objective(e[c:d], g[c:d]), e[c:d]
    s, m = int(obj.argmin()), int(ee.argmax())
    ok = True
    if be is not None and obj.size > 1:
        lead_s, lead_m = np.partition(obj, 1)[1] - obj[s], float(ee[m]) - float(np.partition(ee, -2)[-2])
        ok = bool(lead_s > 2 * (0.9 * be[c:d] + 0.1 * bg[c:d]).max() and lead_m > 2 * be[c:d].max())
    s = s if s < d - 1 else 0
    return c + s, max(c + m, c + s), ok


def snap(c, z):
    before, after, T = c, c + 1, z.shape[0]
    while not z[before] and not (after < T and z[after]):
        before -= 1
        after += 1
    return before if z[before] else after


def cuts_ref(y, envs, grads, coarse_cuts, coarse_peaks, env_bounds=None, grad_bounds=None):
    """Samplifyer.fit III -> dict(sides, lr, cuts, windows, refine_robust): envs / grads are the levels' float32 (T,) arrays, level 0 the
    coarse one; env_bounds / grad_bounds their value bounds, for the robust flag only"""
    cc, cp = np.asarray(coarse_cuts, dtype=np.int64), np.asarray(coarse_peaks, dtype=np.int64)
    windows = np.minimum(cp - cc, MAX_WINDOW)
    lr = left_right(envs[0], envs[-1], cc, windows)
    sides = (lr[:, 0] < lr[:, 1]).astype(np.int64)              # np.stack((left, right)).argmax(0): 0 on a tie
    z = zero_crossings(np.asarray(y))
    cuts, robust = np.zeros_like(cc), np.ones(len(cc), dtype=bool)
    for k in range(len(cc)):
        c, d = int(cc[k]), int(cp[k])
        if sides[k] == 0:
            d = c                                                # (d = c; c = c - (d - c): c stays, the range is empty)
        for l in range(1, len(envs)):
            c, d, ok = refine_step(c, d, envs[l], grads[l], None if env_bounds is None else env_bounds[l], None if grad_bounds is None else grad_bounds[l])
            robust[k] &= ok
        cuts[k] = snap(c, z)
    return dict(sides=sides, lr=lr, cuts=cuts, windows=windows, refine_robust=robust)


def fit_ref(y, envs, grads, sensitivity, env_bounds=None, grad_bounds=None):
    """Samplifyer.fit II + III on float32 curves -> everything the class exposes"""
    att, dec = attack_decay(grads[0])
    ce = envs[0]
    scores = (ce[dec] - ce[att]).astype(np.float32)
    keep = scores > np.float32(sensitivity)
    out = dict(att=att, dec=dec, all_scores=scores, keep=keep, scores=scores[keep], coarse_cuts=att[keep], coarse_peaks=dec[keep])
    out.update(cuts_ref(y, envs, grads, out["coarse_cuts"], out["coarse_peaks"], env_bounds, grad_bounds))
    return out


# ------------------------------------------------------------------------------------------------------------------------- the levels
# How far the device's curves can lie from the golden ones, which come from a float64 transform.  A frame energy of the float32 transform is
# within C_ENERGY u of it (tests/envelope_refs.py), the division by the largest frame adds that frame's error and a rounding, the stored
# float32 one more: FRAME_C u relative per frame.  The spline of perturbed frames moves by at most |A^-1|_inf = 1 / (3/4 - 1/4) = 2 times the
# largest perturbation near by (the interior rows; 0.1716^k away from k frames on), and is rounded to float32 once: VALUE_C = 2 FRAME_C + 1,
# against the largest |e| within BOUND_HOPS frames.  The gradient's lag terms (e[i + d] - e[i - d]) / (2 d L) carry those frame errors and
# tests/envelope_refs.py's C_DERIV u of float32 arithmetic on operands of that size: (FRAME_C + 2 C_DERIV) u E H_L / L <= GRAD_C u E with
# H_L / L <= 1 / 3 from L = 9 on; the division by the largest magnitude M makes that GRAD_C u E / M and adds M's own relative error to |g|.
FRAME_C = ER.C_ENERGY + 3.0 + 1.0
VALUE_C = 2.0 * FRAME_C + 1.0
GRAD_C = 2.0 * (FRAME_C + 2.0 * ER.C_DERIV) / 3.0
BOUND_HOPS = 4


def fixed_length(n_samples, n_fft, hop):
    """samples kept by STFT._fix_length (alignment "end", center=True)"""
    return (n_samples // hop) * hop


def level_frames(y, n_fft, overlap, lag, dtype=torch.float64):
    """-> (env, grad, M): the float32 frames of one level - the bin sums of a torch.stft magnitude (reflect padding, periodic Hann) of the
    length-fixed signal divided by their maximum, and the reference's float32 derivative of that divided by its largest magnitude M"""
    hop = n_fft // overlap
    keep = fixed_length(y.shape[0], n_fft, hop)
    x = torch.from_numpy(np.ascontiguousarray(y[y.shape[0] - keep:])).to(dtype)
    S = torch.stft(x, n_fft, hop_length=hop, return_complex=True, center=True, window=torch.hann_window(n_fft, dtype=dtype),
                   pad_mode="reflect").abs().transpose(-1, -2).numpy()
    e = S.sum(axis=1)
    e = (e / e.max()).astype(np.float32)
    g = ER.derivative_ref(e, lag)
    m = np.abs(g).max()
    return e, (g / m).astype(np.float32), float(m)


def level_curves(y, levels, dtype=torch.float64):
    """-> (envs, grads, env_bounds, grad_bounds): per level the float32 (T,) curves scipy's quadratic interpolation makes of the frames
    (Interpolate.np_func), and the bounds above at every sample"""
    from scipy.ndimage import maximum_filter1d
    T, envs, grads, be, bg = y.shape[0], [], [], [], []
    for n_fft, overlap, lag in levels:
        e, g, m = level_frames(y, n_fft, overlap, lag, dtype)
        envs.append(spline_ref(e, T)[0].astype(np.float32))
        grads.append(spline_ref(g, T)[0].astype(np.float32))
        width = 2 * BOUND_HOPS * (n_fft // overlap) + 1
        big_e = maximum_filter1d(np.abs(envs[-1]).astype(np.float64), width, mode="nearest")
        big_g = maximum_filter1d(np.abs(grads[-1]).astype(np.float64), width, mode="nearest")
        be.append(VALUE_C * U * big_e)
        bg.append(2.0 * U * (GRAD_C * big_e / m + (FRAME_C + 1.0) * big_g))
    return envs, grads, be, bg


def robust_flags(r, grads, sensitivity, be, bg):
    """a kept cut is robust when no decision it went through is closer to its tie than the bounds of the values it compares: the coarse
    gradient on both sides of its attack and of its peak crossing, its score against the threshold, left against right, and every argmin
    and argmax winner's lead (refine_step)"""
    g = np.abs(grads[0].astype(np.float64))
    flags = r["refine_robust"].copy()
    T = g.shape[0]
    for k, (a, p, w) in enumerate(zip(r["coarse_cuts"], r["coarse_peaks"], r["windows"])):
        ok = g[a - 1] > bg[0][a - 1] and g[a] > bg[0][a]
        if p < T - 1:
            ok = ok and g[p] > bg[0][p] and g[p + 1] > bg[0][p + 1]
        ok = ok and abs(float(r["scores"][k]) - sensitivity) > be[0][a] + be[0][p]
        lo, hi = max(a - w, 0), min(a + w, T)
        ok = ok and abs(float(r["lr"][k, 0]) - float(r["lr"][k, 1])) > 2 * (be[0][lo:hi] + be[-1][lo:hi]).max()
        flags[k] &= bool(ok)
    return flags


# ----------------------------------------------------------------------------------------------------------------------- the fixtures
SR = 16000
LEVELS = ((1024, 16, 9), (512, 8, 9), (256, 8, 9))
FIXTURES = {
    # name: (seed, seconds, sensitivity, gap in ms, level of the sustained tone, samples of the gate's smoothing)
    "bursts": (6, 3.0, 0.05, 16.0, 0.3, 9),           # eight cuts, all refined on the right
    "dense": (7, 3.0, 0.0, 16.0, 0.5, 17),            # every attack kept: 21 cuts, 13 of them on the left
}
N_BURSTS = 7


def signal(seed, seconds, gap_ms, tone, smooth):
    """decaying tone bursts over faint noise and a sustained 220 Hz tone that stops `gap_ms` before every burst: the dip gives the finer
    envelopes a pronounced minimum in front of an onset, so that the refinement's winners lead by more than the curves' bounds"""
    rng = np.random.default_rng(seed)
    T = int(SR * seconds)
    t = np.arange(T) / SR
    y = 0.001 * rng.standard_normal(T)
    starts = np.linspace(0.25, seconds - 0.45, N_BURSTS) + rng.uniform(-0.05, 0.05, N_BURSTS)
    gate = np.ones(T)
    for s in starts:
        gate[(t >= s - gap_ms / 1000) & (t < s)] = 0.0
    k = np.hanning(smooth)
    gate = np.convolve(gate, k / k.sum(), mode="same")
    y += tone * np.sin(2 * np.pi * 220 * t) * gate
    for s in starts:
        f, amp, tau = rng.uniform(150, 900), rng.uniform(0.5, 1.0), rng.uniform(0.05, 0.12)
        on = t >= s
        y[on] += amp * np.sin(2 * np.pi * f * (t[on] - s)) * np.exp(-(t[on] - s) / tau) * (1 - np.exp(-(t[on] - s) / 0.001))
    return (y / np.abs(y).max()).astype(np.float32)


@functools.lru_cache(maxsize=None)
def fixture(name, dtype=torch.float64):
    seed, seconds, sens, gap_ms, tone, smooth = FIXTURES[name]
    y = signal(seed, seconds, gap_ms, tone, smooth)
    envs, grads, be, bg = level_curves(y, LEVELS, dtype)
    r = fit_ref(y, envs, grads, sens, be, bg)
    r["robust"] = robust_flags(r, grads, sens, be, bg)
    r["score_bound"] = be[0][r["coarse_cuts"]] + be[0][r["coarse_peaks"]]
    r.update(y=y, sensitivity=sens, envs=envs, grads=grads)
    return r


@functools.lru_cache(maxsize=None)
def golden():
    return np.load(GOLDEN_PATH)


GOLDEN_KEYS = ("y", "sensitivity", "coarse_cuts", "coarse_peaks", "scores", "score_bound", "sides", "cuts", "windows", "robust", "robust_f32")
