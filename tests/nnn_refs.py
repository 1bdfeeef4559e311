"""numpy restatements, cases and derived error bounds of NearestNextNeighbor's alignment (include/mmk.h: mmk_inv_row_norm_f32,
mmk_cosine_cost_f32, mmk_dtw_subseq_f32), shared by tests/test_nnn_refs.py (CPU) and tests/test_gpu_nnn.py.  In the style of
tests/f64_bounds.py: u = 2^-24, every bound is derived from the roundings the computation makes, none is fitted to the kernel.

The reference (mimikit/models/nnn.py:14-35):
    predict_start_frame(X) = dtw(C=pairwise_distances(|X|, |Y|, metric='cosine'), subseq=True)[1][::-1][-1, -1] + 1
sklearn's cosine distance is 1 - <a, b> / (|a| |b|) with a row of norm 0 left as zeros (distance 1 to everything), clipped to [0, 2];
`cosine_distances` below is checked against it where sklearn is installed.  librosa is not installed: `dtw_subseq` restates its
documented algorithm (steps (1,1), (0,1), (1,0), unit weights, subseq=True) and is NOT checked against librosa's code:
    D[0, j] = C[0, j],   D[i, 0] = D[i-1, 0] + C[i, 0],   D[i, j] = C[i, j] + min(D[i-1, j-1], D[i, j-1], D[i-1, j])
Backtracking starts at argmin_j D[N-1, j] (np.argmin: the first minimum), which is where the reversed path ends, so
predict_start_frame = argmin_j D[N-1, j] + 1 and only the last row is needed.

Cost bound.  x, y >= 0 after |.|, so every partial sum is at most the whole.  dot32 = dot (1 + t), |t| <= g(K): K fused multiply-adds.
A squared norm goes through at most K + 6 roundings (a lane's fmaf chain and six butterfly adds), the square root halves that and
rounds, the reciprocal rounds: an inverse norm carries ((K + 6) / 2 + 2) u.  Two products round once each.  The cosine similarity c is
therefore off by at most g(2 K + 12) c, and 1 - c' rounds once more, a value of at most 1: u.  Clipping moves nothing apart.
    cost_bound = g(2 K + 12) c + u,        g(n) = n u / (1 - n u).

DTW bound.  D[N-1, j] is the minimum over paths of the sum of their costs; a path that ends in column j has at most N + j cells.
A cost off by at most e moves every path sum, and so the minimum, by at most (N + j) e.  Each D is one rounded add of an exact
minimum; costs are non-negative, so every partial sum on a path is at most the cell's value and the roundings along a path add up to
at most (N + j) u D.  With e the largest cost bound of the clip:
    dtw_bound[j] = (N + j) (u (D64[N-1, j] + (N + j) e) + e).
Given the SAME fp32 costs, the kernel's last row is not merely close: min is exact and the add is the loop's add, so it is
bit-identical to the sequential fp32 loop.
"""
import functools

import numpy as np

from mimikit_amd import native

U = 2.0 ** -24
MAX_ROWS, ROW_PAD, LOOK = native.NNN_MAX_ROWS, native.NNN_ROW_PAD, native.NNN_LOOKAHEAD

NS = (1, 2, 16, 63, 64)
MS_COST = (1, 2, 63, 64, 65, 257)
KS = (1, 3, 4, 513, 1025)
BATCHES = (1, 3)
MS_DTW = MS_COST + (LOOK - 1, LOOK, LOOK + 1, 4099)


def gamma(n):
    return n * U / (1 - n * U)


def n_pad(n):
    return (n + ROW_PAD - 1) // ROW_PAD * ROW_PAD


# ---------------------------------------------------------------------------------------------------------------- cosine distance
def cosine_similarity(x, y):
    """x (..., N, K), y (M, K) -> (..., N, M) float64: <|x|, |y|> / (|x| |y|), 0 where a norm is 0"""
    x, y = np.abs(np.asarray(x, dtype=np.float64)), np.abs(np.asarray(y, dtype=np.float64))
    nx, ny = np.sqrt((x * x).sum(-1, keepdims=True)), np.sqrt((y * y).sum(-1, keepdims=True))
    xn = np.divide(x, nx, out=np.zeros_like(x), where=nx > 0)
    yn = np.divide(y, ny, out=np.zeros_like(y), where=ny > 0)
    return xn @ yn.T


def cosine_distances(x, y):
    """sklearn.metrics.pairwise_distances(|x|, |y|, metric='cosine') in float64"""
    return np.clip(1.0 - cosine_similarity(x, y), 0.0, 2.0)


def cost_bound(x, y):
    k = np.asarray(x).shape[-1]
    return gamma(2 * k + 12) * cosine_similarity(x, y) + U


# ---------------------------------------------------------------------------------------------------------------- subsequence DTW
def dtw_subseq(C):
    """the accumulated-cost matrix D (N, M) of the module's comment, cell by cell in C's dtype: in float32 this IS the sequential
    fp32 loop (numpy rounds every float32 add once)"""
    C = np.asarray(C)
    N, M = C.shape
    D = np.empty_like(C)
    D[0] = C[0]
    for i in range(1, N):
        D[i, 0] = D[i - 1, 0] + C[i, 0]
        for j in range(1, M):
            D[i, j] = C[i, j] + min(D[i - 1, j - 1], D[i, j - 1], D[i - 1, j])
    return D


def dtw_last_row(C):
    """D[..., N-1, :] of C (..., N, M) in C's dtype.  The same cells with the same arithmetic as `dtw_subseq` (an exact minimum, one add),
    visited anti-diagonal by anti-diagonal so that numpy works on a whole diagonal at once - bit-identical, and fast enough for M = 4099"""
    C = np.asarray(C)
    N, M = C.shape[-2:]
    lead = C.shape[:-2]
    inf = np.array(np.inf, dtype=C.dtype)
    cur = np.full(lead + (N,), inf, dtype=C.dtype)       # D[i, j-1]: row i's value on the previous diagonal
    prev = cur.copy()                                     # ... and on the one before
    pad = np.full(lead + (1,), inf, dtype=C.dtype)
    last = np.empty(lead + (M,), dtype=C.dtype)
    rows = np.arange(N)
    for s in range(M + N - 1):
        j = s - rows
        act = (j >= 0) & (j < M)
        up = np.concatenate([pad, cur[..., :-1]], -1)     # D[i-1, j]
        diag = np.concatenate([pad, prev[..., :-1]], -1)  # D[i-1, j-1]
        m = np.minimum(np.minimum(up, diag), cur)
        m[..., 0] = 0
        d = cur.copy()
        d[..., act] = C[..., rows[act], j[act]] + m[..., act]
        prev, cur = cur, d
        if act[N - 1]:
            last[..., j[N - 1]] = d[..., N - 1]
    return last


def end_column(last_row):
    """np.argmin: the first minimum"""
    return np.argmin(last_row, axis=-1)


def dtw_bound(last64, n, e):
    """last64 (..., M): the float64 last row; e: the clip's largest cost bound (0 where the kernel was given the float64 run's own costs)"""
    length = n + np.arange(last64.shape[-1], dtype=np.float64)
    e = np.asarray(e, dtype=np.float64)[..., None]
    return length * (U * (last64 + length * e) + e)


def outside(got, want, bound):
    """elements of `got` outside the bound (NaN counts as outside)"""
    return ~(np.abs(np.asarray(got, dtype=np.float64) - want) <= bound)


# ---------------------------------------------------------------------------------------------------------------- cases
@functools.lru_cache(maxsize=None)
def frames(rows, k, seed, signed=False):
    """(rows, k) float32, uniform in [0, 1) (or [-1, 1)), read-only"""
    rng = np.random.default_rng(seed)
    a = rng.uniform(-1.0 if signed else 0.0, 1.0, size=(rows, k)).astype(np.float32)
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def cost_case(batch, n, m, k):
    """signed prompts (batch, n, k) and corpus (m, k) with one zero row each (where there are two rows to spare), the float64 distances
    (batch, n, m) and their bound - computed once, shared, never written to"""
    x = frames(batch * n, k, 100 + 7 * n + k, signed=True).reshape(batch, n, k).copy()
    y = frames(m, k, 200 + 11 * m + k, signed=True).copy()
    if n > 1:
        x[-1, n // 2] = 0
    if m > 1:
        y[m // 2] = 0
    want, bound = cosine_distances(x, y), cost_bound(x, y)
    for a in (x, y, want, bound):
        a.setflags(write=False)
    return x, y, want, bound


PLANT_K = 64
# (n, m, per-clip (offset of the copy in the corpus, gain)): offsets differ per clip, touch the corpus' start and end
PLANTED = ((16, 257, ((0, 0.5), (100, 1.0), (241, 3.0))),
           (64, 257, ((193, 2.0), (0, 1.0), (77, 0.25))),
           (63, 4099, ((4036, 1.5), (1234, 0.75), (3, 1.0))))


@functools.lru_cache(maxsize=None)
def planted_case(index):
    """corpus (m, PLANT_K) of random non-negative frames; clip b's prompt is gain_b times the n corpus frames from offset_b on, so its
    alignment ends at offset_b + n - 1 with distance 0.  -> x (batch, n, k), y, the float64 last rows, the planted end columns"""
    n, m, plants = PLANTED[index]
    y = frames(m, PLANT_K, 300 + index)
    x = np.stack([(np.float32(g) * y[o:o + n]).astype(np.float32) for o, g in plants])
    last64 = dtw_last_row(cosine_distances(x, y))
    ends = np.array([o + n - 1 for o, _ in plants])
    for a in (x, last64):
        a.setflags(write=False)
    return x, y, last64, ends


def planted_gap(index):
    """per clip: (float64 minimum outside the planted segment) - (float64 minimum), and twice the end-to-end bound at its largest"""
    n, m, plants = PLANTED[index]
    x, y, last64, ends = planted_case(index)
    e = cost_bound(x, y).max(axis=(-1, -2))
    bound = dtw_bound(last64, n, e)
    gaps = []
    for b, (o, _) in enumerate(plants):
        out = np.ones(m, dtype=bool)
        out[o:o + n] = False
        gaps.append((last64[b][out].min() if out.any() else np.inf) - last64[b].min())
    return np.array(gaps), 2 * bound.max(-1)
