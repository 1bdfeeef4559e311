"""float64 restatements, cases and derived bounds of the clustering kernels (include/mmk.h: mmk_nn_cosine_self_f32, mmk_nn_components_i64,
mmk_segment_mean_f32) and of mimikit_amd.extract.clusters, shared by tests/test_hcluster_refs.py (CPU) and tests/test_gpu_hcluster.py.
numpy only, in the style of tests/neighbors_refs.py: u = 2^-24, v = 2^-53, every bound is derived from the roundings the computation
makes, none is fitted to what the GPU returns.

The reference (mimikit/extract/clusters.py:157-205), restated by `hcluster64`: at every level the cosine of every row with every OTHER row
(a zero row has cosine 0 to everything; self excluded by index), the arg-max with ties to the lower index, the weakly connected components
of i -> nearest[i] numbered by their smallest member, the label column composed with the one before, and the UNWEIGHTED mean of the level's
rows of every component as the next level's rows; it stops at one component.

Level 0.  The rows are the fp32 inputs, exact on both sides: `neighbors_refs.cos_bound` with the diagonal at -inf, and its index rule - a
row whose float64 gap between best and second best exceeds 2 row_bound must return the float64 arg-max.

Level L > 0.  The device's rows are centroids rounded to fp32 once per level, so they differ from the float64 restatement's by an
element-wise error e with |e| <= E_L:
    E_0 = 0;    E_L[c] = mean_members(E_{L-1}) + u (|x_L[c]| + mean_members(E_{L-1})) + (n_c + 1) v mean_members(|x_{L-1}| + E_{L-1})
(the members carry E_{L-1}; the fp64 sum of n_c members and the division make n_c + 1 roundings of relative size v; the one rounding to fp32 is
u of the computed mean).  For unit vectors, |(x + e) / |x + e| - x / |x|| <= 2 |e| / |x| =: rho, and <a', b'> - <a, b> = <a' - a, b'> + <a, b' - b>,
so the cosine of two perturbed rows moves by at most rho_r + rho_j, and so does the a = <|a|, |b|> of the kernel's own rounding bound:
    level_bound[r, j] = g(2 K + 12) (a[r, j] + rho_r + rho_j) + rho_r + rho_j,        rho_r = 2 |E_L[r]|_2 / |x_L[r]|_2 (0 for a zero row).
The index rule holds with this bound in place of cos_bound.  The fixture inputs keep every level's smallest gap above 4 x the row's bound
(twice what the rule needs), so the device must reproduce the reference's labels exactly: held by the CPU test in float64 alone.

Segment mean.  Inputs are fp32 (exact in fp64); n fp64 additions and one division: (n + 1) v mean|x|; one rounding to fp32: half an ulp of
the result:   mean_bound = ulp32(mean64) / 2 + (n + 1) v mean64(|x|).
"""
import functools

import numpy as np

from tests import neighbors_refs as NR

U = NR.U
V = NR.V
SPAN = NR.SPAN

SELF_ROWS = (2, 3, 50, 129)
SELF_KS = (1, 33, 64)
BIG_SELF_CASE = (2 * SPAN + 3, 33)        # the diagonal crosses tile, query-block and span edges
COPIES = ((127, 128), (2047, 2048))       # exact copies across a tile / query-block edge and across a span edge
ZERO_ROW = 1000
MEAN_KS = (1, 33, 1025)
MEAN_SEGMENTS = (2, 3, 700, 1)            # (the last: a segment of one member, whose mean is the row)
ONE_ROW = (1,)                            # the whole input is one row in one segment
DEFECTS = ("self_allowed", "last_tie", "mean_of_frames", "number_by_cycle", "no_relabel")


# ---------------------------------------------------------------------------------------------------------------- components
def _cycle_min(nearest):
    """per node the smallest node on the cycle its walk ends in"""
    n = len(nearest)
    state = np.zeros(n, dtype=np.int8)        # 0 new, 1 on the current walk, 2 done
    out = np.full(n, -1, dtype=np.int64)
    for s in range(n):
        if state[s]:
            continue
        walk, i = [], s
        while state[i] == 0:
            state[i] = 1
            walk.append(i)
            i = int(nearest[i])
        if state[i] == 1:                     # the walk closed a new cycle at i
            cyc = walk[walk.index(i):]
            c = min(cyc)
        else:
            c = out[i]
        for w in walk:
            out[w] = c
            state[w] = 2
    return out


def components64(nearest, defect=None):
    """nearest (n,) -> (labels (n,) int64, K): the weakly connected components of i -> nearest[i] by union-find, numbered by rising smallest
    member.  Defect 'number_by_cycle': numbered by the smallest node of their cycle"""
    nearest = np.asarray(nearest, dtype=np.int64)
    n = nearest.shape[0]
    parent = np.arange(n)

    def find(i):
        while parent[i] != i:
            parent[i] = parent[parent[i]]
            i = parent[i]
        return i
    for i in range(n):
        a, b = find(i), find(int(nearest[i]))
        if a != b:
            parent[max(a, b)] = min(a, b)     # the root is the component's smallest member
    root = np.array([find(i) for i in range(n)], dtype=np.int64)
    key = _cycle_min(nearest) if defect == "number_by_cycle" else root
    uniq, labels = np.unique(key, return_inverse=True)
    return labels.astype(np.int64), int(uniq.shape[0])


@functools.lru_cache(maxsize=None)
def graph_cases():
    """name -> nearest (int64, read-only): the functional graphs of the components test"""
    n1, n2 = 4098, 4099
    i1, i2 = np.arange(n1), np.arange(n2)
    chain = i2 - 1
    chain[0] = 1
    star = np.zeros(1000, dtype=np.int64)
    star[0] = 1
    cases = {
        "self_loop_1": np.array([0]),
        "mutual_2": np.array([1, 0]),
        "pairs_4098": i1 ^ 1,
        "chain_4099": chain,
        "cycle_4099": (i2 + 1) % n2,
        "cycle3_tails": np.array([1, 2, 0, 0, 3, 2, 7, 6]),
        "star_1000": star,
        # {0, 5, 6} has its cycle on (5, 6) and its smallest member 0 on the tail; {1, 2}, {3, 4} lie between
        "min_off_cycle": np.array([5, 2, 1, 4, 3, 6, 5]),
        "random_100003": np.random.default_rng(4242).integers(0, 100003, 100003),
    }
    out = {}
    for name, a in cases.items():
        a = a.astype(np.int64)
        a.setflags(write=False)
        out[name] = a
    return out


# ---------------------------------------------------------------------------------------------------------------- one level
def cosine_others64(x, defect=None):
    """(n, k) -> (n, n) float64 cosines with the diagonal at -inf ('self_allowed': left in)"""
    c = NR.cosine64(x, x)
    if defect != "self_allowed":
        np.fill_diagonal(c, -np.inf)
    return c


def rho(x, err):
    n = np.sqrt((np.asarray(x, dtype=np.float64) ** 2).sum(-1))
    e = np.sqrt((err ** 2).sum(-1))
    return np.divide(2 * e, n, out=np.zeros_like(n), where=n > 0)


def level_bound(x, err=None):
    """(n, n) bound on |device cosine - float64 cosine| of the level's rows x (float64) whose device twins carry the element-wise error err"""
    k = np.asarray(x).shape[-1]
    a = NR._unit(x, True) @ NR._unit(x, True).T
    if err is None:
        return NR.gamma(2 * k + 12) * a
    r = rho(x, err)
    rr = r[:, None] + r[None, :]
    return NR.gamma(2 * k + 12) * (a + rr) + rr


def row_bound_others(bound):
    b = bound.copy()
    np.fill_diagonal(b, 0.0)
    return b.max(-1)


def next_rows(xa, err, labels, k):
    """the unweighted means of the components' rows and their error bound E"""
    new = np.stack([xa[labels == c].mean(0) for c in range(k)])
    e_mean = np.stack([err[labels == c].mean(0) for c in range(k)])
    size = np.bincount(labels, minlength=k).astype(np.float64)[:, None]
    mag = np.stack([(np.abs(xa[labels == c]) + err[labels == c]).mean(0) for c in range(k)])
    return new, e_mean + U * (np.abs(new) + e_mean) + (size + 1) * V * mag


def hcluster64(x, max_iter=32, defect=None):
    """-> dict(labels (N, levels) int64, K (int or None), levels: a list, per level, of dict(x, err, nearest, labels, k, gap, bound) with
    gap (n,) = best minus second-best cosine of every row, bound (n,) = the row's level bound)"""
    x = np.asarray(x)
    x0 = x.astype(np.float64)
    n = x.shape[0]
    xa, err = x0, np.zeros_like(x0)
    columns, levels, frame_labels, K = [], [], None, None
    for i in range(max_iter):
        c = cosine_others64(xa, defect)
        nearest = NR.argmax_first(c, defect)
        labels, k = components64(nearest, defect)
        bound = row_bound_others(level_bound(xa, err if i else None))
        levels.append(dict(x=xa, err=err, nearest=nearest, labels=labels, k=k, gap=NR.gap64(c), bound=bound))
        if frame_labels is None:
            frame_labels = labels
        elif defect == "no_relabel":
            frame_labels = labels[np.minimum(np.arange(n), labels.shape[0] - 1)]
        else:
            frame_labels = labels[frame_labels]
        columns.append(frame_labels)
        if defect == "mean_of_frames":
            xa, err = next_rows(x0, np.zeros_like(x0), frame_labels, k)
        else:
            xa, err = next_rows(xa, err, labels, k)
        if k == 1:
            K = i + 1
            break
    labels_ = np.stack(columns, 1).astype(np.int64) if columns else np.zeros((n, 0), dtype=np.int64)
    return dict(labels=labels_, K=K, levels=levels)


# ---------------------------------------------------------------------------------------------------------------- cases of the self arg-max
@functools.lru_cache(maxsize=None)
def self_case(rows, k):
    """x (rows, k) float32 (signed where k == 1, so that a row has a best other row at all), the float64 cosines with the diagonal at -inf and
    the rows' bounds - computed once, shared, read-only"""
    rng = np.random.default_rng(7000 + 131 * rows + k)
    x = NR._frames(rng, rows, k, k == 1)
    if k == 1:
        x = x + np.sign(x).astype(np.float32)           # away from 0
    c = cosine_others64(x)
    b = row_bound_others(level_bound(x))
    for a in (x, c, b):
        a.setflags(write=False)
    return x, c, b


@functools.lru_cache(maxsize=None)
def big_self_case():
    """non-negative x (2 SPAN + 3, 33) with exact copies at COPIES (each pair finds each other) and a zero row"""
    rows, k = BIG_SELF_CASE
    x = NR._frames(np.random.default_rng(7777), rows, k, False)
    for a, b in COPIES:
        x[b] = x[a]
    x[ZERO_ROW] = 0
    c = cosine_others64(x)
    b = row_bound_others(level_bound(x))
    for a in (x, c, b):
        a.setflags(write=False)
    return x, c, b


# ---------------------------------------------------------------------------------------------------------------- segment mean
@functools.lru_cache(maxsize=None)
def mean_case(k, sizes=MEAN_SEGMENTS):
    """x (n, k) signed float32, order (a seeded permutation of the rows), offsets of segments of `sizes` members, the float64 means
    (taken in the order given) and their bound"""
    rng = np.random.default_rng(8100 + k)
    n = sum(sizes)
    x = (rng.standard_normal((n, k)) * np.exp(rng.uniform(-3, 3, (n, 1)))).astype(np.float32)
    order = rng.permutation(n).astype(np.int64)
    offsets = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    x64 = x.astype(np.float64)
    want = np.stack([x64[order[a:b]].mean(0) for a, b in zip(offsets[:-1], offsets[1:])])
    mag = np.stack([np.abs(x64[order[a:b]]).mean(0) for a, b in zip(offsets[:-1], offsets[1:])])
    size = np.diff(offsets).astype(np.float64)[:, None]
    bound = 0.5 * np.spacing(np.abs(want).astype(np.float32)).astype(np.float64) + (size + 1) * V * mag
    for a in (x, order, offsets, want, bound):
        a.setflags(write=False)
    return x, order, offsets, want, bound
