"""float64 restatements, cases and derived bounds of the k-best and edge-component kernels (include/mmk.h: mmk_nn_topk_f32,
mmk_half_neg_sqnorm_f32, mmk_edge_components_i64) and of mimikit_amd.extract.clusters.QCluster, shared by tests/test_qcluster_refs.py (CPU),
tests/test_gpu_qcluster.py and tests/golden/make_golden_qcluster.py.  numpy only, in the style of tests/hcluster_refs.py: u = 2^-24,
v = 2^-53, every bound is derived from the roundings the computation makes, none is fitted to what the GPU returns.

The reference (mimikit/extract/clusters.py:27-98), restated by `qcluster64`.  With qe = 1 - cores_prop, n = n_neighbors (int(sqrt(N)) if
None), k = core_neighborhood_size (int(qe n) if None):
    lists[i]      the max(n, k) nearest OTHER frames of frame i under the metric, nearest first (ties to the lower index)
    in_degree[j]  the number of i with j among the first n of lists[i]
    is_core       in_degree >= numpy.quantile(in_degree, qe)      (the default "linear" method, float64)
    edges         core i - every core j among the first k of lists[i];  non-core i - its nearest core
    labels_, K_   the connected components of the undirected edges, numbered by rising smallest member (as scipy numbers them)

Keys.  The kernel orders by key[r, j] = (<x_r, y_j> qscale[r]) cscale[j] + cshift[j], the larger the nearer.
  cosine      scales = the inverse norms, shift 0, clamped to [-1, 1]: the cosine of mmk_nn_cosine_f32, operation for operation, and
              neighbors_refs.cos_bound holds as it stands:   bound[r, j] = g(2 K + 12) a[r, j].
  euclidean   scales 1 (exact), shift s_j = -|y_j|^2 / 2:  |x - y|^2 = |x|^2 - 2 key, so the largest key is the smallest distance.
              The dot product is a chain of K fused multiply-adds: |d32 - d| <= e1 = g(K) <|x|, |y|>.  The shift is K fused multiply-adds
              and six butterfly adds of non-negative terms in fp64, a product with -0.5 (exact) and ONE rounding to fp32:
              |s32 - s| <= e2 = (u + (K + 7) v) |y|^2 / 2.  The sum rounds once: u |d32 + s32| <= u (|key| + e1 + e2).
                  bound[r, j] = (e1 + e2) (1 + u) + u |key64[r, j]|.
Index rule.  With b = the row's largest bound over the candidates, fp32 keys order two frames as float64 does wherever their float64 keys
differ by more than 2 b.  So slot p must hold the float64 choice where BOTH float64 gaps next to slot p exceed 2 b (the frames before
p are then exactly float64's first p in some order, and the frame at p beats everything behind it), and the SET of the first T must be
float64's where the gap between the T-th and the (T + 1)-th exceeds 2 b.  Slots past the last candidate hold -1 / -inf.

QCluster.  The result depends on the lists only through the SET of the first n, the SET of the first k and, for a non-core, the nearest
core: `qcluster64` returns, per fixture, the smallest float64 gap at those three boundaries over the row's bound (`ratio`).  The fixtures
keep it at 4 or more (twice what the index rule needs), so the device must reproduce the reference's labels exactly.
"""
import functools

import numpy as np

from mimikit_amd import native
from tests import neighbors_refs as NR

U = NR.U
V = NR.V
SPAN = NR.SPAN
TOPK_MAX = native.NN_TOPK_MAX
METRICS = ("euclidean", "cosine")

SELF_ROWS = (2, 3, 50, 129)
SELF_KS = (1, 33, 64)
TS = (1, 2, 9, TOPK_MAX)
# (queries, corpus frames, bins) without self_exclude; the last three: one query row, one corpus frame, one of each with one bin
CROSS_CASES = ((200, 5, 33), (200, 131, 33), (1, 131, 33), (200, 1, 33), (1, 1, 1))
BIG_CASE = (2 * SPAN + 3, 33)
COPIES = ((127, 128), (2047, 2048))               # exact copies across a tile / query-block edge and across a span edge
ZERO_ROW = 1000
DEFECTS = ("self_counted", "floor_quantile", "edges_to_non_cores", "edges_from_all", "nearest_frame", "number_by_largest")

# name: (seed, low, frames, metric, parameters) - tests/golden/make_golden_qcluster.py
FIXTURES = {
    "euclid": (802, -1.0, 300, "euclidean", {}),
    "euclid_q": (802, -1.0, 300, "euclidean", dict(cores_prop=.25, n_neighbors=12, core_neighborhood_size=5)),
    "cosine": (802, 0.0, 300, "cosine", {}),
    "cosine_q": (802, 0.0, 300, "cosine", dict(cores_prop=.25, n_neighbors=12, core_neighborhood_size=5)),
    "auto": (802, -1.0, 150, "euclidean", dict(n_neighbors=None, core_neighborhood_size=None)),
    # the quantile falls between two different order statistics of the in-degree: a floor quantile names other cores
    "between": (802, -1.0, 60, "euclidean", dict(cores_prop=.3, n_neighbors=6, core_neighborhood_size=4)),
}


def fixture_frames(seed, low, frames):
    rng = np.random.default_rng(seed)
    c = rng.uniform(low, 1, (5, 8))
    return (c[rng.integers(0, 5, frames)] + 0.3 * rng.standard_normal((frames, 8))).astype(np.float32)


# ---------------------------------------------------------------------------------------------------------------- keys and bounds
def key64(x, y, metric):
    """(rows, m) float64 keys: the cosine, or <x, y> - |y|^2 / 2"""
    if metric == "cosine":
        return NR.cosine64(x, y)
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    return x @ y.T - 0.5 * (y * y).sum(-1)[None, :]


def key_bound(x, y, metric):
    """(rows, m) bound on |device key - float64 key|"""
    if metric == "cosine":
        return NR.cos_bound(x, y)
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    k = x.shape[-1]
    e1 = NR.gamma(k) * (np.abs(x) @ np.abs(y).T)
    e2 = (U + (k + 7) * V) * 0.5 * (y * y).sum(-1)[None, :]
    return (e1 + e2) * (1 + U) + U * np.abs(key64(x, y, metric))


def others(a, fill):
    a = a.copy()
    np.fill_diagonal(a, fill)
    return a


def order64(key):
    """every row's columns by falling key, equal keys by rising index"""
    return np.argsort(-key, axis=-1, kind="stable")


def topk_rule_violations(index, key, bound, t):
    """rows of index (rows, t) that break the index rule against the float64 keys (rows, m) (-inf = no candidate) and their bounds"""
    index = np.asarray(index)
    rows, m = key.shape
    order = order64(key)
    s = np.take_along_axis(key, order, -1)
    cand = np.isfinite(key).sum(-1)
    b = np.where(np.isfinite(key), bound, 0.0).max(-1)
    sp = np.concatenate([np.full((rows, 1), np.inf), s, np.full((rows, max(t + 1 - m, 1)), -np.inf)], -1)       # sp[:, p + 1] = s[:, p]
    bad = np.zeros(rows, dtype=bool)
    for r in range(rows):
        got, c = index[r], min(int(cand[r]), t)
        if (got[c:] != -1).any() or (got[:c] < 0).any() or (got[:c] >= m).any() or np.unique(got[:c]).shape[0] != c:
            bad[r] = True
            continue
        if not np.isfinite(key[r, got[:c]]).all():
            bad[r] = True
            continue
        for p in range(c):
            above, below = sp[r, p] - sp[r, p + 1], sp[r, p + 1] - sp[r, p + 2]
            if above > 2 * b[r] and below > 2 * b[r] and got[p] != order[r, p]:
                bad[r] = True
        if c and sp[r, c] - sp[r, c + 1] > 2 * b[r] and set(got[:c].tolist()) != set(order[r, :c].tolist()):
            bad[r] = True
    return bad


def _ro(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


@functools.lru_cache(maxsize=None)
def self_case(rows, k, metric):
    """x (rows, k) float32 (signed where k == 1), its float64 keys with the diagonal at -inf, and the bounds - computed once, read-only"""
    rng = np.random.default_rng(9000 + 131 * rows + k)
    x = NR._frames(rng, rows, k, k == 1)
    if k == 1:
        x = x + np.sign(x).astype(np.float32)
    return _ro(x, others(key64(x, x, metric), -np.inf), others(key_bound(x, x, metric), 0.0))


@functools.lru_cache(maxsize=None)
def cross_case(rows, m, k, metric):
    rng = np.random.default_rng(9500 + rows + 17 * m + k)
    x, y = NR._frames(rng, rows, k, True), NR._frames(rng, m, k, True)
    return _ro(x, y, key64(x, y, metric), key_bound(x, y, metric))


@functools.lru_cache(maxsize=None)
def big_case(metric):
    """non-negative x (2 SPAN + 3, 33) with exact copies at COPIES and a zero row.  Every row is scaled to norm 1 (to within its fp32
    roundings): the euclidean keys of a row are then of one size, and the row's bound says something about every one of them"""
    rows, k = BIG_CASE
    x = NR._frames(np.random.default_rng(7778), rows, k, False).astype(np.float64)
    x = (x / np.sqrt((x * x).sum(-1, keepdims=True))).astype(np.float32)
    for a, b in COPIES:
        x[b] = x[a]
    x[ZERO_ROW] = 0
    return _ro(x, others(key64(x, x, metric), -np.inf), others(key_bound(x, x, metric), 0.0))


# ---------------------------------------------------------------------------------------------------------------- edge components
def edge_components64(src, dst, n, defect=None):
    """(labels (n,) int64, K): the connected components of the undirected edges by union-find, numbered by rising smallest member
    ('number_by_largest': by rising largest member)"""
    parent = np.arange(n)

    def find(i):
        while parent[i] != i:
            parent[i] = parent[parent[i]]
            i = parent[i]
        return i
    for u, v in zip(np.asarray(src).tolist(), np.asarray(dst).tolist()):
        a, b = find(u), find(v)
        if a != b:
            parent[max(a, b)] = min(a, b)
    root = np.array([find(i) for i in range(n)], dtype=np.int64)
    if defect == "number_by_largest":
        largest = np.zeros(n, dtype=np.int64)
        np.maximum.at(largest, root, np.arange(n))
        root = largest[root]
    uniq, labels = np.unique(root, return_inverse=True)
    return labels.astype(np.int64), int(uniq.shape[0])


@functools.lru_cache(maxsize=None)
def edge_cases():
    """name -> (src, dst, n), int64 and read-only"""
    rng = np.random.default_rng(4343)
    n_path = 4099
    ids = rng.permutation(n_path)
    shuffle = rng.permutation(n_path - 1)
    a, b = np.arange(20), np.arange(20, 45)
    clique = lambda m: np.array([(i, j) for i in m for j in m if i < j])
    two = np.concatenate([clique(a), clique(b), [[7, 31]]])
    big = rng.integers(0, 100003, (150000, 2))
    cases = {
        "empty_5": (np.zeros(0), np.zeros(0), 5),
        "self_loops_6": (np.array([0, 3, 3, 5]), np.array([0, 3, 3, 5]), 6),
        "repeated_reversed_9": (np.array([1, 2, 1, 2, 7, 8, 8, 4]), np.array([2, 1, 2, 1, 8, 7, 7, 4]), 9),
        "path_4099_permuted": (ids[:-1][shuffle], ids[1:][shuffle], n_path),
        "two_cliques_one_bridge": (two[:, 0], two[:, 1], 47),
        "star_1000": (np.full(999, 613), np.delete(np.arange(1000), 613), 1000),
        "random_100003": (big[:, 0], big[:, 1], 100003),
    }
    out = {}
    for name, (s, d, n) in cases.items():
        s, d = s.astype(np.int64), d.astype(np.int64)
        _ro(s, d)
        out[name] = (s, d, n)
    return out


# ---------------------------------------------------------------------------------------------------------------- QCluster
def qcluster64(x, cores_prop=.5, n_neighbors=8, core_neighborhood_size=8, metric="euclidean", defect=None):
    """-> dict(labels (N,) int64, is_core (N,) bool, K, n, k, src, dst, ratio): the reference's fit restated in float64; `ratio` is the
    smallest float64 gap, over the row's bound, at the boundaries the result hangs on (see the module docstring)"""
    x = np.asarray(x)
    N = x.shape[0]
    qe = 1 - cores_prop
    n = int(np.sqrt(N)) if n_neighbors is None else n_neighbors
    k = int(qe * n) if core_neighborhood_size is None else core_neighborhood_size
    if N <= n:
        raise ValueError(f"n_neighbors = {n} needs more than {n} frames")
    key_all = key64(x, x, metric)
    key = others(key_all, -np.inf)
    bound = others(key_bound(x, x, metric), 0.0)
    b = bound.max(-1)
    order = order64(key)
    lists = order[:, :max(n, k)]
    counted = order64(key_all)[:, :n] if defect == "self_counted" else lists[:, :n]
    in_degree = np.bincount(counted.reshape(-1), minlength=N)
    is_core = in_degree >= np.quantile(in_degree, qe, method="lower" if defect == "floor_quantile" else "linear")
    cores = np.nonzero(is_core)[0]
    src, dst = [], []
    for i in range(N):
        if is_core[i] or defect == "edges_from_all":
            for j in lists[i, :k]:
                if is_core[j] or defect == "edges_to_non_cores":
                    src.append(i)
                    dst.append(int(j))
        if not is_core[i]:
            j = order[i, 0] if defect == "nearest_frame" else next(int(j) for j in order[i] if is_core[j])
            src.append(i)
            dst.append(int(j))
    src, dst = np.array(src, dtype=np.int64), np.array(dst, dtype=np.int64)
    labels, K = edge_components64(src, dst, N, defect)
    s = np.take_along_axis(key, order, -1)
    gaps = [s[:, n - 1] - s[:, n]] if n < N - 1 else []
    if 0 < k < N - 1 and k != n:
        gaps.append(s[:, k - 1] - s[:, k])
    ratio = min(float((g / b).min()) for g in gaps) if gaps else np.inf
    if cores.shape[0] >= 2 and cores.shape[0] < N:
        kc = np.sort(key[~is_core][:, cores], -1)
        ratio = min(ratio, float(((kc[:, -1] - kc[:, -2]) / b[~is_core]).min()))
    return dict(labels=labels, is_core=is_core, K=K, n=n, k=k, src=src, dst=dst, ratio=ratio, in_degree=in_degree)


def fixture_result(name, x, defect=None):
    _, _, _, metric, params = FIXTURES[name]
    return qcluster64(x, metric=metric, defect=defect, **params)
