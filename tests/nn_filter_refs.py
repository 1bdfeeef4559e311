"""Restatements, cases and derived bounds of the nearest-neighbour filter (include/mmk_nn_filter.h: mmk_nn_aggregate_f32;
mimikit_amd.NearestNeighborFilter), shared by tests/test_nn_filter_refs.py (CPU), tests/test_gpu_nn_filter.py and
tests/golden/make_golden_nn_filter.py.  numpy only, in the style of tests/qcluster_refs.py, whose `key64` and `key_bound` order the frames
here: u = 2^-24, v = 2^-53, every bound is derived from the roundings the computation makes, none is fitted to what the GPU returns.

The reference (mimikit/features/functionals.py:1083-1111) is librosa.decompose.nn_filter(x, aggregate, metric, sym=True, sparse=True,
k, axis=0).  librosa is not installed here; what it does is restated from its published source, from memory, for x of (n, D), frames as rows:
    1. sklearn's NearestNeighbors gives every frame's min(n - 1, k + 2) nearest OTHER frames;
    2. "the k closest" of them are kept, by an argsort of stored values that are all 1 in connectivity mode - which k survive is an accident
       of an unstable sort.  Restated here is the documented meaning, the k nearest ('k_plus_two' is the other extreme: all are kept);
    3. a link i - j stays only if each is on the other's list (rec.minimum(rec.T));
    4. out[i] = aggregate(x[neighbours of i], axis=0), a frame without a neighbour keeps its values.
`lists64` is steps 1-2 on float64 keys, `mutual_lists64` step 3 on ANY (n, t) index in the kernel's terms (a slot is empty if its value lies
outside [0, n) or is its own row number), `nn_aggregate64` step 4 with numpy's own np.median / np.max / np.min on float32 - their bits are the
demand - and `mean64` for the mean, which the kernel sums in float64 in slot order and rounds once:
    |fl32(s~ / c) - m| <= u |m| + (c + 1) v sum|x_j| / c + 2^-150:   c - 1 float64 additions and one division, each within v of its result
    (first order: (c + 1) v of sum|x_j| / c, with room for the second-order terms), one rounding to float32 (u |m|, or half the smallest
    subnormal, 2^-150, where m is subnormal).
`nn_filter64` runs all four steps and returns, with the result, the smallest float64 gap at every row's k | k + 1 boundary over the row's key
bound (`ratio`): fp32 keys order two frames as float64 does where their keys differ by more than twice the bound (qcluster_refs: index
rule), so at ratio >= 2 the device's SETS of k nearest are float64's; the fixtures keep it at 4 or more, and exact agreement is a fair demand.
"""
import functools

import numpy as np

from mimikit_amd import native
from tests import neighbors_refs as NR
from tests.qcluster_refs import key64, key_bound, order64, others

U = NR.U
V = NR.V
TOPK_MAX = native.NN_TOPK_MAX
OPS = native.NN_AGGREGATES                     # the op codes of include/mmk_nn_filter.h, in order
GOLDEN_OPS = ("median", "mean", "max")
DEFECTS = ("one_sided", "self_included", "lower_median", "upper_median", "empty_row_zero", "k_plus_two", "mean_over_slots", "empty_slot_as_row0")

# the kernel cases: host-drawn lists, independent of the search
NS = (1, 2, 3, 5, 129)                         # a single row (every slot empty), one wave of a workgroup, three, two workgroups, 33 workgroups with a tail
DS = (1, 63, 64, 65, 257)                      # below, at and past one lane stride; past two steps of 128 bins
TS = (1, 2, 15, TOPK_MAX)

# name: (frames, bins, k, metric, seed, rows without a neighbour) - tests/golden/make_golden_nn_filter.py;
# x = default_rng(seed).uniform(0, 1, (frames, bins)) as float32
FIXTURES = {
    "cos96": (96, 33, 16, "cosine", 1088, 1),
    "euc96": (96, 33, 16, "euclidean", 1084, 0),
    "cos40": (40, 12, 4, "cosine", 1084, 4),
    "euc40": (40, 12, 4, "euclidean", 1084, 2),
    "euc300": (300, 33, 8, "euclidean", 1087, 10),
    "all12": (12, 7, 16, "cosine", 1084, 0),   # n - 1 <= k: librosa's trimming is a no-op, every frame lists every other
}
MIN_RATIO = 4.0


def _ro(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays if len(arrays) > 1 else arrays[0]


@functools.lru_cache(maxsize=None)
def fixture_frames(name):
    n, d, _, _, seed, _ = FIXTURES[name]
    return _ro(np.random.default_rng(seed).uniform(0, 1, (n, d)).astype(np.float32))


# ---------------------------------------------------------------------------------------------------------------- the lists
def lists64(x, k, metric, defect=None):
    """-> (index (n, max(k, t)) int64, ratio): every frame's t = min(k, n - 1) nearest other frames by float64 key, nearest first, -1 in the
    slots behind them, and the smallest gap at the t | t + 1 boundary over the row's bound (inf where there is no t + 1-th).
    'k_plus_two': t = min(k + 2, n - 1);
    'self_included': the frame itself is a candidate (and comes first)"""
    x = np.asarray(x)
    n = x.shape[0]
    t = min(k + 2 if defect == "k_plus_two" else k, n - 1)
    full = key64(x, x, metric)
    key = full if defect == "self_included" else others(full, -np.inf)
    order = order64(key)
    ratio = np.inf
    if t < n - 1:
        b = others(key_bound(x, x, metric), 0.0).max(-1)
        s = np.take_along_axis(others(full, -np.inf), order64(others(full, -np.inf)), -1)
        ratio = float(((s[:, t - 1] - s[:, t]) / b).min())
    index = np.full((n, max(k, t)), -1, dtype=np.int64)          # as a search asked for k writes it: -1 past the last candidate
    index[:, :t] = order[:, :t]
    return index, ratio


def mutual_lists64(index, mutual=True, defect=None):
    """index (n, t) -> a list of n int64 arrays: the neighbours of every row in rising slot order.  A slot is empty if its value lies
    outside [0, n) or is its own row number; with `mutual` j counts only if some slot of row j holds i.  'one_sided': no mutual test;
    'self_included': a row's own number is a neighbour like any other; 'empty_slot_as_row0': an empty slot is read as row 0"""
    index = np.asarray(index)
    n = index.shape[0]
    rows = np.arange(n)[:, None]
    inside = (index >= 0) & (index < n)
    full = inside if defect == "self_included" else inside & (index != rows)
    if defect == "empty_slot_as_row0":
        index = np.where(full, index, 0)
        full = np.ones_like(full)
    out = []
    for i in range(n):
        nb = index[i][full[i]]
        if mutual and defect != "one_sided":
            nb = np.array([j for j in nb if (index[j][full[j]] == i).any()], dtype=np.int64)
        out.append(nb.astype(np.int64))
    return out


# ---------------------------------------------------------------------------------------------------------------- the aggregates
def mean64(rows):
    """rows (c, D) float32 -> (fl32 of the float64 mean, the bound on the kernel's |result - float64 mean|)"""
    r = np.asarray(rows, dtype=np.float64)
    c = r.shape[0]
    m = r.sum(0) / c
    bound = U * np.abs(m) + (c + 1) * V * np.abs(r).sum(0) / c + 2.0 ** -150
    return m, bound


def nn_aggregate64(x, index, op, mutual=True, defect=None):
    """-> (out (n, D), counts (n,) int32, bound (n, D)): step 4 on the lists of mutual_lists64.  median / max / min are numpy's own on
    float32 (out is float32, the bound 0); mean is the float64 mean (out is float64, the bound mean64's).  'lower_median' / 'upper_median':
    the lower / upper of the two middle values of an even count; 'empty_row_zero': a row without a neighbour becomes 0; 'mean_over_slots':
    the sum is divided by the number of slots"""
    x = np.asarray(x)
    assert x.dtype == np.float32 and op in OPS
    n, d = x.shape
    lists = mutual_lists64(index, mutual, defect)
    out = np.zeros((n, d), dtype=np.float64 if op == "mean" else np.float32)
    bound = np.zeros((n, d))
    for i, nb in enumerate(lists):
        c = nb.shape[0]
        if c == 0:
            out[i] = 0 if defect == "empty_row_zero" else x[i]
            continue
        rows = x[nb]
        if op == "mean":
            out[i], bound[i] = mean64(rows)
            if defect == "mean_over_slots":
                out[i] = out[i] * c / np.asarray(index).shape[1]
        elif op == "median":
            if c % 2 == 0 and defect in ("lower_median", "upper_median"):
                out[i] = np.sort(rows, axis=0)[c // 2 - (defect == "lower_median")]
            else:
                out[i] = np.median(rows, axis=0)
        else:
            out[i] = (np.max if op == "max" else np.min)(rows, axis=0)
    return out, np.array([nb.shape[0] for nb in lists], dtype=np.int32), bound


def nn_filter64(x, k=16, metric="cosine", aggregate="median", defect=None):
    """-> dict(out, counts, bound, index, ratio): the four steps of the module docstring"""
    index, ratio = lists64(x, k, metric, defect)
    out, counts, bound = nn_aggregate64(x, index, aggregate, True, defect)
    return dict(out=out, counts=counts, bound=bound, index=index, ratio=ratio)


@functools.lru_cache(maxsize=None)
def fixture_result(name, aggregate, defect=None):
    _, _, k, metric, _, _ = FIXTURES[name]
    res = nn_filter64(fixture_frames(name), k, metric, aggregate, defect)
    _ro(res["out"], res["counts"], res["bound"], res["index"])
    return res


def numpy_mean_bound(rows_abs_sum, c):
    """|numpy's float32 mean - the exact mean| of c float32 rows whose |.| add up to rows_abs_sum: c - 1 float32 additions in some order
    and one division, gamma(c) of sum|x_j| / c"""
    return NR.gamma(c) * rows_abs_sum / np.maximum(c, 1)


# ---------------------------------------------------------------------------------------------------------------- the kernel cases
def draw_index(rng, n, t):
    """(n, t) int64: per row min(t, n - 1) distinct OTHER rows in random slots, a random number of them blanked to -1; then one slot of
    some rows replaced by another kind of empty slot (the row's own number, n, a large value, a negative one)"""
    index = np.full((n, t), -1, dtype=np.int64)
    for i in range(n):
        m = min(t, n - 1)
        nb = rng.permutation(np.delete(np.arange(n), i))[:m]
        keep = int(rng.integers(0, m + 1))
        slots = rng.permutation(t)[:keep]
        index[i, slots] = nb[:keep]
    for i in range(0, n, 3):
        index[i, int(rng.integers(0, t))] = (i, n, 2 ** 40 + 3, -5)[(i // 3) % 4]
    return index


@functools.lru_cache(maxsize=None)
def kernel_case(n, d, t):
    """x (n, d) float32 - signed, with values repeated across rows (ties in the median: every value is one of 7 per bin where n > 7), one
    block of subnormals - and a drawn (n, t) index; in the index of a case with n >= 5 and t >= 2 row 1 names row 0 twice (a row named by
    two slots counts twice) and row 0 names row 1; computed once, read-only"""
    rng = np.random.default_rng(5000 + 1000 * n + 17 * d + t)
    x = rng.standard_normal((n, d)).astype(np.float32)
    if n > 7:
        x = x[rng.integers(0, 7, (n, d)), np.arange(d)[None, :]]
    x[: max(n // 2, 1), : max(d // 3, 1)] *= np.float32(2.0 ** -130)              # subnormal values, some of them halved by an even median
    index = draw_index(rng, n, t)
    if n >= 5 and t >= 2:
        index[1, :2] = 0
        index[0, 0] = 1
    return _ro(x, index)
