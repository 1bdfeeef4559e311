"""float64 restatements, cases and derived error bounds of the segmentation kernels (include/mmk.h: mmk_novelty_f32, mmk_novelty_finish_f32,
mmk_pick_peaks_f32) and of mimikit_amd.extract.segment, shared by tests/test_segment_refs.py (CPU) and tests/test_gpu_segment.py.  In the style of
tests/neighbors_refs.py: u = 2^-24, every bound is derived from the roundings the computation makes, none is fitted to what the GPU returns.

The reference (mimikit/extract/segment.py:21-174), for frames X (T, D) and a half-width h:
    d(r, c) = 1 - <X_r, X_c> / (|X_r| |X_c|),   1 where the denominator is 0,   d(r, r) = 0 (its loop skips i == j, a zero row included)
    raw_h[i] = 1 / (4 h^2) sum_{a = -h..h, a != 0} sum_{b = -h..h, b != 0} -sign(a) sign(b) d(i + a, i - 1 + b)      (outside [0, T): 0)
    scores[q] = raw_{h_q} - min_i raw_{h_q},     dg = mean_q scores[q]
`raw64` is the direct double sum over the (T, T) matrix, not the band the kernel or the reference walk.

Distance bound.  The kernel's cosine is the chain of tests/neighbors_refs.py's cos_bound - a dot product of K fused multiply-adds in one fixed
order (the zeros a tile is padded with add nothing), two inverse norms of (K + 6) / 2 + 2 roundings each, two products - so
|c32 - c64| <= g(2 K + 12) a[r, c] with a = <|x_r|, |x_c|> / (|x_r| |x_c|).  The subtraction from 1 rounds once more, relative to the fp32
distance, which is within that bound of d64:
    dist_bound[r, c] = cb (1 + u) + u |d64|,    cb = g(2 K + 12) a[r, c];        0 on the diagonal, for a zero row (exactly 1) and outside.
Board bound.  The weights' absolute sum is 4 h^2 / (4 h^2) = 1 at most, so the fp64 sum of fp32 distances is within the LARGEST distance bound
under the board of raw64; the sum itself is exact to 4 h^2 v (v = 2^-53) relative to the sum of magnitudes (at most 2), and rounds to fp32 once:
    raw_bound[i] = max_{(a, b) on the board, in range} dist_bound[i + a, i - 1 + b] + u |raw64[i]| + 8 h^2 v.
Scores: the minimum of fp32 values within raw_bound of their float64 twins is within max_i raw_bound of the float64 minimum, the
subtraction rounds once:   scores_bound[i] = raw_bound[i] + max_i raw_bound + u |scores64[i]|.
dg: n - 1 additions and a division, each one rounding of a partial sum no larger than n dg:
    dg_bound[i] = mean_q scores_bound[q][i] + n u (|dg64[i]| + mean_q scores_bound[q][i]).

Picker.  `picker64` restates pick_globally_sorted_maxes (segment.py:135-160) with equal values taken lower index first (the reference's
argsort is not stable there).  `robust(x, eps, wb, wa, ms)` is True when no perturbation of x by at most eps per element can change its
result, so that a device result computed from a dg within eps = dg_bound of the float64 one MUST equal picker64 of the float64 dg:
  * every index that could be a local maximum under such a perturbation (x[i] > x[i-1] - 2 eps and x[i] >= x[i+1] - 2 eps) has a strength
    further from min_strength than the strength's own error: numerator x - min moves by 2 eps, the range by 2 eps;
  * those above the threshold differ from both neighbours, and from both dominance means, by more than 2 eps (a mean moves by eps);
  * any two that survive and lie in one another's window differ by more than 2 eps, so their order is fixed.
"""
import functools

import numpy as np

from mimikit_amd import native

U = 2.0 ** -24
V = 2.0 ** -53
TILE = native.NOVELTY_TILE
MAX_HALF = native.NOVELTY_MAX_HALF

TS = (2, 5, TILE - 1, TILE, TILE + 1, 2 * TILE + 3)
DS = (1, 31, 33, 513)
HALVES = ([1], [6], [MAX_HALF], [1, 6, MAX_HALF])
CORPUS_BOUNDS = [37, 87, 110, 174, 215, 244]          # the segment boundaries of corpus_case(): what the float64 picker returns
CORPUS_HALVES = [6, 12]
CORPUS_MIN_DUR, CORPUS_MIN_STRENGTH = 4, 0.03


def gamma(n):
    return n * U / (1 - n * U)


# ---------------------------------------------------------------------------------------------------------------- distances and scores
def _norms(x):
    return np.sqrt((x * x).sum(-1))


def dist64(x, defect=None):
    """x (T, D) -> (T, T) float64 cosine distances as the reference defines them.  Defects: 'no_diag_zero' (d(r, r) = 1 - cos, which is 1 for
    a zero row), 'zero_row_d0' (0 instead of 1 where a norm is 0)"""
    x = np.asarray(x, dtype=np.float64)
    n = _norms(x)
    den = n[:, None] * n[None, :]
    with np.errstate(divide="ignore", invalid="ignore"):
        d = np.where(den == 0, 0.0 if defect == "zero_row_d0" else 1.0, 1.0 - (x @ x.T) / den)
    if defect != "no_diag_zero":
        np.fill_diagonal(d, 0.0)
    return d


def board_terms(h):
    """(a, b, weight) of the normalised checkerboard of half-width h"""
    return [(a, b, -np.sign(a) * np.sign(b) / (4.0 * h * h)) for a in range(-h, h + 1) if a for b in range(-h, h + 1) if b]


def _under_board(d, h, centre=1, edge=False):
    """(terms, T): row t holds d[i + a_t, i - centre + b_t] for every i, 0 (or the nearest entry: `edge`) outside; and the weights (terms,)"""
    terms = board_terms(h)
    T = d.shape[0]
    i = np.arange(T)[None, :]
    r = i + np.array([t[0] for t in terms])[:, None]
    c = i - centre + np.array([t[1] for t in terms])[:, None]
    vals = d[np.clip(r, 0, T - 1), np.clip(c, 0, T - 1)]
    if not edge:
        vals = np.where((r >= 0) & (r < T) & (c >= 0) & (c < T), vals, 0.0)
    return vals, np.array([t[2] for t in terms])


def raw64(x, h, defect=None):
    """the direct double sum.  Defects: those of dist64, 'centre_ii' (the board centred on (i, i)), 'edge_pad' (the matrix continued by its
    edge values instead of zeros)"""
    vals, w = _under_board(dist64(x, defect), h, 0 if defect == "centre_ii" else 1, defect == "edge_pad")
    return w @ vals


def scores64(x, halves, defect=None):
    """-> raw (n, T), scores (n, T), dg (T,) float64"""
    raw = np.stack([raw64(x, h, defect) for h in halves])
    scores = raw - raw.min(-1, keepdims=True)
    return raw, scores, scores.mean(0)


def band64(x, k):
    """pwdk_cosine(X, k) by its in-bounds meaning: (T, 2 k - 1), column k + (j - i) holds d(i, j) for |j - i| <= k where that column exists"""
    d = dist64(x)
    T = d.shape[0]
    band = np.zeros((T, 2 * k - 1))
    for i in range(T):
        for j in range(max(i - k, 0), min(i + k + 1, T)):
            if i != j and k + (j - i) < 2 * k - 1:
                band[i, k + (j - i)] = d[i, j]
    return band


def convolve_diagonals64(diagonals, kernel):
    """convolve_diagonals: out[i] = sum_{j, l} diagonals[i + j, K - j - 1 + l] kernel[j, l]"""
    K = kernel.shape[0]
    n = diagonals.shape[0] - K + 1
    return np.array([sum(diagonals[i + j, K - j - 1:2 * K - j - 1] @ kernel[j] for j in range(K)) for i in range(n)])


def checker64(h):
    c = np.zeros((2 * h + 1, 2 * h + 1))
    for a, b, w in board_terms(h):
        c[a + h, b + h] = w
    return c


def raw_by_parts(x, h, h_max):
    """the reference's assembly (segment.py:120-130) from the restated parts: the band of the largest kernel, sliced to this one, padded
    with h rows of zeros, convolved with the checkerboard"""
    band = band64(x, 2 * h_max + 1)
    extra = 2 * (h_max - h)
    dk = band[:, extra:band.shape[1] - extra] if extra else band
    return convolve_diagonals64(np.pad(dk, ((h, h), (0, 0))), checker64(h))


def dist_bound(x):
    x = np.asarray(x, dtype=np.float64)
    k = x.shape[-1]
    n = _norms(x)
    den = n[:, None] * n[None, :]
    with np.errstate(divide="ignore", invalid="ignore"):
        a = np.where(den == 0, 0.0, (np.abs(x) @ np.abs(x).T) / den)
    cb = gamma(2 * k + 12) * a
    b = cb * (1 + U) + U * np.abs(dist64(x))
    b[den == 0] = 0.0
    np.fill_diagonal(b, 0.0)
    return b


def raw_bound(x, h, raw):
    return _under_board(dist_bound(x), h)[0].max(0) + U * np.abs(raw) + 8.0 * h * h * V


def bounds(x, halves):
    """-> raw64, scores64, dg64 and their bounds (six arrays), float64"""
    raw, scores, dg = scores64(x, halves)
    rb = np.stack([raw_bound(x, h, r) for h, r in zip(halves, raw)])
    sb = rb + rb.max(-1, keepdims=True) + U * np.abs(scores)
    n = len(halves)
    gb = sb.mean(0) + n * U * (np.abs(dg) + sb.mean(0))
    return raw, scores, dg, rb, sb, gb


def raw32_numpy(x, h):
    """a plain fp32 evaluation (numpy's own order of the sums): what the bound must hold"""
    x = np.asarray(x, dtype=np.float32)
    n = np.sqrt((x * x).sum(-1, dtype=np.float32))
    with np.errstate(divide="ignore"):
        inv = np.where(n > 0, np.float32(1) / n, np.float32(0)).astype(np.float32)
    d = (np.float32(1) - (x @ x.T) * inv[:, None] * inv[None, :]).astype(np.float32)
    np.fill_diagonal(d, 0.0)
    vals, w = _under_board(d.astype(np.float64), h)
    return (w @ vals).astype(np.float32)


def outside(got, want, bound):
    return ~(np.abs(np.asarray(got, dtype=np.float64) - want) <= bound)


def assert_inside(got, want, bound, what):
    bad = outside(got, want, bound)
    if bad.any():
        i = tuple(int(a[0]) for a in np.nonzero(bad))
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.size} elements outside the derived bound; at {i}: got {float(np.asarray(got)[i]):.9g}, "
                             f"want {np.asarray(want)[i]:.9g}, error {abs(float(np.asarray(got)[i]) - np.asarray(want)[i]):.3e} > bound {np.asarray(bound)[i]:.3e}")
    return float(np.max(np.abs(np.asarray(got, dtype=np.float64) - want) / np.maximum(bound, 1e-300)))


# ---------------------------------------------------------------------------------------------------------------- picker
def localmax(x):
    """librosa.util.localmax on one axis: x[i] > x[i-1] and x[i] >= x[i+1], the ends padded with themselves"""
    x = np.asarray(x)
    p = np.pad(x, 1, mode="edge")
    return (x > p[:-2]) & (x >= p[2:])


def min_filter(x, size, cval):
    """scipy.ndimage.minimum_filter1d(x, size, mode='constant', cval=cval): the window [i - size // 2, i + size - size // 2 - 1]"""
    T = x.shape[0]
    p = np.concatenate([np.full(size, cval), x, np.full(size, cval)])
    lo = size - size // 2
    return np.array([p[lo + i:lo + i + size].min() for i in range(T)])


def _candidates(x, wb, wa, ms):
    x = np.asarray(x, dtype=np.float64)
    T = x.shape[0]
    rg = x.max() - x.min()
    if rg == 0:
        return x, np.zeros(T, bool)
    strength = (x - min_filter(x, wb + wa, x.min())) / rg
    cand = localmax(x) & (strength >= ms)
    for m in np.nonzero(cand)[0]:
        lo, hi = max(0, m - wb), min(T, m + wa)
        cand[m] = m > lo and x[m] > x[lo:m].mean() and x[m] > x[m:hi].mean()
    return x, cand


def picker64(x, wb, wa, ms=0.02):
    """pick_globally_sorted_maxes in float64: the dominance test first (it does not depend on what has been accepted), then the candidates
    by falling x, equal values lower index first, one accepted unless an accepted one lies in [m - wb, m + wa).  A constant x: none."""
    x, cand = _candidates(x, wb, wa, ms)
    idx = np.nonzero(cand)[0]
    order = idx[np.argsort(-x[idx], kind="stable")]
    final = np.zeros(x.shape[0], bool)
    for m in order:
        if not final[max(0, m - wb):min(x.shape[0], m + wa)].any():
            final[m] = True
    return np.nonzero(final)[0]


def cuts64(dg, min_dur, ms):
    mx = picker64(dg, min_dur, min_dur, ms)
    return mx[(mx > min_dur) & (mx < dg.shape[0] - min_dur)]


def robust(x, eps, wb, wa, ms):
    x = np.asarray(x, dtype=np.float64)
    eps = np.broadcast_to(np.asarray(eps, dtype=np.float64), x.shape).max()
    T = x.shape[0]
    rg = x.max() - x.min()
    if not rg > 4 * eps:
        return False
    p = np.pad(x, 1, mode="edge")
    possible = (x > p[:-2] - 2 * eps) & (x >= p[2:] - 2 * eps)
    possible[0] = False                                  # x[0] > x[0] holds under no perturbation
    strength = (x - min_filter(x, wb + wa, x.min())) / rg
    s_err = (2 * eps + 2 * eps * np.abs(strength)) / (rg - 2 * eps) + 1e-12
    if (np.abs(strength - ms) <= s_err)[possible].any():
        return False
    keep = []
    for m in np.nonzero(possible & (strength >= ms))[0]:
        lo, hi = max(0, m - wb), min(T, m + wa)
        if hi - m == 1:
            continue                                     # the right-hand mean is x[m] itself: never above it, under any perturbation
        diffs = [x[m] - x[m - 1], x[m] - x[lo:m].mean(), x[m] - x[m:hi].mean()] + ([x[m] - x[m + 1]] if m + 1 < T else [])
        if min(abs(v) for v in diffs) <= 2 * eps:
            return False
        if min(diffs) > 0:
            keep.append(m)
    for i, m in enumerate(keep):
        for n in keep[i + 1:]:
            if (m - wb <= n < m + wa or n - wb <= m < n + wa) and abs(x[m] - x[n]) <= 2 * eps:
                return False
    return True


# ---------------------------------------------------------------------------------------------------------------- cases
@functools.lru_cache(maxsize=None)
def frames_case(T, D, batch=1):
    """(batch, T, D) float32 frames, signed (D > 1), a few strong bins per frame; where T allows: a zero frame in the middle and at index 0 of
    clip 0, two identical neighbouring frames - computed once, shared, read-only"""
    rng = np.random.default_rng(7000 + 131 * T + D + 7 * batch)
    x = rng.exponential(1.0, (batch, T, D)) ** 3
    if D > 1:
        x = x * rng.choice((-1.0, 1.0), x.shape)
    else:
        x = x * np.where(rng.uniform(size=x.shape) < 0.3, -1.0, 1.0)
    x = x.astype(np.float32)
    if T >= 5:
        x[0, 0] = 0
        x[:, T // 2] = 0
        x[:, T // 2 - 2] = x[:, T // 2 - 1]
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def corpus_case():
    """a piecewise-stationary corpus: 7 segments of 23 to 70 frames, each a fixed non-negative random frame of 33 bins plus 5 % noise;
    float32 (293, 33).  The float64 cuts with CORPUS_HALVES, CORPUS_MIN_DUR and CORPUS_MIN_STRENGTH are CORPUS_BOUNDS"""
    rng = np.random.default_rng(2024)
    lengths = np.diff([0] + CORPUS_BOUNDS + [CORPUS_BOUNDS[-1] + 49])
    parts = [np.abs(rng.uniform(0.0, 1.0, (1, 33)) * (1.0 + 0.05 * rng.standard_normal((n, 33)))) for n in lengths]
    x = np.concatenate(parts).astype(np.float32)
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def constant_case():
    """every frame the same, of norm 2: <x, x> = 4, 1 / |x| = 1 / 2 and the cosine 1 are exact in fp32 and in float64, so every distance is
    exactly 0, raw and dg are constant 0 and the picker has nothing to divide by.  (With a norm that is no power of two the distances are a
    common rounding residue, which the zero padding turns into a step at the two ends: dg is then NOT constant.)"""
    return np.ones((150, 4), dtype=np.float32)


@functools.lru_cache(maxsize=None)
def case_bounds(T, D, halves, batch=1, clip=0):
    """bounds() of clip `clip` of frames_case(T, D, batch) for the tuple `halves` - computed once, shared"""
    return bounds(frames_case(T, D, batch)[clip], list(halves))
