"""The scoring kernels on the MI355X (csrc/neighbors.hip) against the float64 restatements and derived bounds of tests/neighbors_refs.py: the two
entry points through the C ABI on strided, misaligned rows with NaN-filled outputs and workspace, every call made twice for the same bits, and
nearest_neighbor / NeighborScorer / cum_entropy on device tensors against the reference's results of tests/golden/neighbors.npz.  Each test
prints its worst error / bound."""
import os

import numpy as np
import pytest
import torch

import mimikit_amd as mmk
from mimikit_amd import native
from tests import neighbors_refs as R
from tests.f64_bounds import check_written
from tests.strided_inputs import FLOAT_SURROUNDS, INT_SURROUNDS, Strided, surround_rule

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

G = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "neighbors.npz"))
SPAN = native.NN_SPAN


def same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


# ------------------------------------------------------------------------------------------------------------------ arg-max kernel
@surround_rule(*FLOAT_SURROUNDS)
def nn_call(x_np, y_np, device, x_off=1, y_off=3):
    """mmk_nn_cosine_f32 on strided, misaligned rows; outputs and workspace NaN-filled (the index buffer holds -1).  -> index, cos_best (numpy)"""
    rows, k = x_np.shape
    m = y_np.shape[0]
    lib = native.lib()
    x, y = Strided.of(x_np, x_off, device), Strided.of(y_np, y_off, device)
    rx, ry = native.inv_row_norm(x.view), native.inv_row_norm(y.view)
    n_work = lib.mmk_nn_cosine_workspace_bytes(rows, m)
    assert 0 < n_work <= rows * -(-m // SPAN) * 16 + 4096
    work = torch.full((n_work // 4 + 3,), float("nan"), dtype=torch.float32, device=device)
    index = torch.full((rows + 4,), -1, dtype=torch.int64, device=device)
    best = torch.full((rows + 4,), float("nan"), dtype=torch.float32, device=device)
    native.check(lib.mmk_nn_cosine_f32(x.ptr, x.stride, rx.data_ptr(), rows, y.ptr, y.stride, ry.data_ptr(), m, k, index.data_ptr(), best.data_ptr(),
                                       work.data_ptr(), n_work, native.stream_ptr(device)))
    mask = torch.zeros(best.shape, dtype=torch.bool)
    mask[:rows] = True
    check_written(best, mask, f"cos_best {rows, m, k}")
    idx = index.cpu().numpy()
    assert (idx[rows:] == -1).all() and (idx[:rows] >= 0).all() and (idx[:rows] < m).all(), f"index {rows, m, k}"
    assert bool(torch.isnan(work[n_work // 4:]).all()), "the workspace was written beyond its size"
    return index[:rows], best[:rows]


def check_nn(x_np, y_np, c, bound, device, what):
    index, best = nn_call(x_np, y_np, device)
    again_i, again_b = nn_call(x_np, y_np, device)
    assert torch.equal(index, again_i) and same_bits(best, again_b), f"{what}: two calls differ"
    idx, got = index.cpu().numpy(), best.cpu().numpy()
    bad = R.index_rule_violations(idx, c, bound)
    assert not bad.any(), f"{what}: rows {np.nonzero(bad)[0][:8]} break the index rule"
    cb = np.take_along_axis(R.cos_bound(x_np, y_np), idx[:, None], -1)[:, 0]
    return R.assert_inside(got, np.take_along_axis(c, idx[:, None], -1)[:, 0], cb + 1e-300, what)


@pytest.mark.parametrize("k", R.KS[:-1])
def test_argmax_against_the_bound(device, k):
    worst = 0.0
    for rows, m, kk in R.argmax_cases():
        if kk != k:
            continue
        for signed in (False, True) if k > 1 and m > 1 else (False,):
            x, y, c, bound = R.nn_case(rows, m, k, signed)
            worst = max(worst, check_nn(x, y, c, bound, device, f"rows {rows}, m {m}, k {k}, signed {signed}"))
    print(f"nn_cosine k {k}: worst cosine error / bound {worst:.3f}")


def test_argmax_1025_bins(device):
    rows, m, k = R.BIG_K_CASE
    x, y, c, bound = R.nn_case(rows, m, k, True)
    worst = check_nn(x, y, c, bound, device, f"rows {rows}, m {m}, k {k}")
    print(f"nn_cosine k {k}: worst cosine error / bound {worst:.3f}")


def test_argmax_over_many_query_blocks(device):
    """values from every query block and span of a launch that has more query blocks than one group of workgroups: the numbering of the
    workgroups, the smaller last group with its idle workgroups and the workspace addresses of blocks past the first"""
    rows, m, k = R.MANY_BLOCKS_CASE
    x, y, c, bound = R.nn_case(rows, m, k, True)
    worst = check_nn(x, y, c, bound, device, f"rows {rows}, m {m}, k {k}")
    print(f"nn_cosine {rows} rows, {m} frames: worst cosine error / bound {worst:.3f}")


def test_planted_frames(device):
    """ties between exact copies in different spans go to the lower index; a query that is a corpus frame finds it at distance 0 inside the
    bound (the cosine of a frame with itself is 1 to within the roundings of the sum and the two norms, and acos is steep there); a zero
    query has cosine 0 to every frame and takes frame 0, a zero corpus frame is never the best of a non-zero query"""
    x, y, want = R.planted_case()
    index, best = nn_call(x, y, device)
    assert np.array_equal(index.cpu().numpy(), want)
    assert float(best[2]) == 0.0 and float(best[:2].min()) > 1 - 2 * R.row_bound(x, y).max()
    xd, yd = torch.from_numpy(x.copy()).to(device), torch.from_numpy(y.copy()).to(device)
    dists, nn = mmk.nearest_neighbor(xd, yd)
    assert np.array_equal(nn.cpu().numpy(), want)
    d64, _, c = R.nearest64(x, y)
    assert d64[2] == 1.0 and abs(d64[[0, 1, 3, 4]]).max() < 1e-7            # non-negative data: the factor 2, so a right angle is 1
    worst = R.assert_inside(dists.cpu().numpy(), d64, R.dist_bound(c.max(-1), R.row_bound(x, y), True), "planted distances")
    # a zero query and a zero corpus frame in a signed call: cosine exactly 0, the factor 1, so the reference's distance acos(0) / pi = 1 / 2;
    # every other frame points away from the second query, which leaves the zero frame (11) as its nearest
    ys = y[:40]
    xs = np.stack([np.zeros(64, np.float32), -y[3] - y[4] - y[6]]).astype(np.float32)
    idx_s, best_s = nn_call(xs, ys, device)
    assert np.array_equal(idx_s.cpu().numpy(), [0, 11]) and float(best_s[0]) == 0.0 and float(best_s[1]) == 0.0
    ds, ns = mmk.nearest_neighbor(torch.from_numpy(xs).to(device), torch.from_numpy(ys.copy()).to(device))
    d64s, n64s, cs = R.nearest64(xs, ys)
    assert np.array_equal(ns.cpu().numpy(), n64s) and np.array_equal(n64s, [0, 11]) and np.array_equal(d64s, [0.5, 0.5])
    R.assert_inside(ds.cpu().numpy(), d64s, R.dist_bound(cs.max(-1), R.row_bound(xs, ys), False), "signed planted distances")
    print(f"planted: worst distance error / bound {worst:.3f}")


def test_python_peak_allocation(device):
    rows, m, k = 2000, 20000, 64
    gen = torch.Generator().manual_seed(3)
    x, y = torch.rand(rows, k, generator=gen).to(device), torch.rand(m, k, generator=gen).to(device)
    scorer = mmk.NeighborScorer(y)
    torch.cuda.synchronize(device)
    torch.cuda.reset_peak_memory_stats(device)
    before = torch.cuda.memory_allocated(device)
    dists, nn = scorer(x)
    torch.cuda.synchronize(device)
    peak = torch.cuda.max_memory_allocated(device) - before
    assert peak < rows * m * 4 / 10, f"peak {peak} bytes against a matrix of {rows * m * 4}"
    assert dists.shape == nn.shape == (rows,)
    xn, yn = x.cpu().numpy(), y.cpu().numpy()
    d64, _, c = R.nearest64(xn, yn)
    bound = R.row_bound(xn, yn)
    assert not R.index_rule_violations(nn.cpu().numpy(), c, bound).any()
    worst = R.assert_inside(dists.cpu().numpy(), d64, R.dist_bound(c.max(-1), bound, True), "distances of the 2000 x 20000 call")
    print(f"peak allocation {peak} bytes, the matrix would be {rows * m * 4} (peak / cap {peak / (rows * m * 4 / 10):.3f}); "
          f"worst distance error / bound {worst:.3f}")


# ------------------------------------------------------------------------------------------------------------------ Python paths
@pytest.mark.parametrize("name", ("nonneg", "signed"))
def test_nearest_neighbor_against_the_fixture(device, name):
    x, y = G[f"nn_{name}_x"], G[f"nn_{name}_y"]
    d64, _, c = R.nearest64(x, y)
    bound = R.row_bound(x, y)
    nonneg = name == "nonneg"
    db = R.dist_bound(c.max(-1), bound, nonneg)
    xd, yd = torch.from_numpy(x.copy()).to(device), torch.from_numpy(y.copy()).to(device)
    scorer = mmk.NeighborScorer(yd)
    worst = 0.0
    for dists, nn in (mmk.nearest_neighbor(xd, yd), scorer(xd)):
        assert dists.device.type == "cuda" and dists.dtype == torch.float32 and nn.dtype == torch.int64 and dists.shape == nn.shape == (50,)
        assert not R.index_rule_violations(nn.cpu().numpy(), c, bound).any()
        worst = max(worst, R.assert_inside(dists.cpu().numpy(), d64, db, f"distances, {name}"))
        # the reference's own results carry the same kind of bound: the two agree within both
        R.assert_inside(dists.cpu().numpy(), G[f"nn_{name}_dists"].astype(np.float64), 2 * db, f"distances against the reference, {name}")
        wide = R.gap64(c) > 2 * bound
        assert np.array_equal(nn.cpu().numpy()[wide], G[f"nn_{name}_index"][wide])
    d2, n2 = scorer(xd)
    d3, n3 = scorer(xd.reshape(5, 10, -1))
    d4, n4 = scorer(torch.cat([xd, xd]).reshape(2, 50, -1))
    assert d3.shape == n3.shape == (5, 10) and same_bits(d3.reshape(-1), d2) and torch.equal(n3.reshape(-1), n2)
    assert same_bits(d4[1], d2) and same_bits(d4[0], d2) and torch.equal(n4[1], n2)
    print(f"nearest_neighbor {name}: worst distance error / bound {worst:.3f}")


# ------------------------------------------------------------------------------------------------------------------ cumulative entropy
@surround_rule(*INT_SURROUNDS)
def entropy_call(items_np, device, per_step=True, off=1):
    batch, t = items_np.shape
    it = Strided.of(items_np, off, device, decoy=(int(items_np.min()), int(items_np.max()) + 2))      # (any int64 is an item: decoys from the rows' own range)
    total = torch.full((batch + 3,), float("nan"), dtype=torch.float32, device=device)
    e = Strided((batch, t), 3, device, float("nan"))
    native.check(native.lib().mmk_cum_entropy_i64(it.ptr, it.stride, batch, t, total.data_ptr(), e.ptr if per_step else None, e.stride,
                                                  native.stream_ptr(device)))
    mask = torch.zeros(total.shape, dtype=torch.bool)
    mask[:batch] = True
    check_written(total, mask, f"total {batch, t}")
    if per_step:
        check_written(e.buf, e.mask(), f"e {batch, t}")
    else:
        assert bool(torch.isnan(e.buf).all())
    return total[:batch], e.view


@pytest.mark.parametrize("t", R.ENTROPY_TS)
def test_cum_entropy_against_the_bound(device, t):
    items, e64 = R.entropy_case(t)
    worst = 0.0
    for batch in R.ENTROPY_BATCHES:
        total, e = entropy_call(items[:batch], device)
        again_t, again_e = entropy_call(items[:batch], device)
        assert same_bits(total, again_t) and same_bits(e, again_e), f"T {t}, batch {batch}: two calls differ"
        only_total, _ = entropy_call(items[:batch], device, per_step=False)
        assert same_bits(only_total, total)
        assert float(e.min()) >= 0 and float(total.min()) >= 0
        for b in range(batch):
            worst = max(worst, R.assert_inside(e[b].cpu().numpy(), e64[b], R.entropy_bound(e64[b]) + 1e-300, f"e, T {t}, row {b}"))
            tb = R.total_bound(e64[b])
            err = abs(float(total[b]) - e64[b].sum())
            assert err <= tb, f"total, T {t}, row {b}: error {err:.3e} > bound {tb:.3e}"
            worst = max(worst, err / max(tb, 1e-300))
    print(f"cum_entropy T {t}: worst error / bound {worst:.3f}")


def test_cum_entropy_python(device):
    worst = 0.0
    for name in ("random", "same", "distinct"):
        items = G[f"ce_{name}_items"]
        e64 = R.cum_entropy64(items)
        n = torch.from_numpy(items.copy()).to(device)
        total, e = mmk.cum_entropy(n), mmk.cum_entropy(n, reduce="none")
        assert total.shape == () and e.shape == (40,) and total.dtype == e.dtype == torch.float32 and total.device.type == "cuda"
        worst = max(worst, R.assert_inside(e.cpu().numpy(), e64, R.entropy_bound(e64) + 1e-300, f"e, {name}"))
        assert abs(float(total) - e64.sum()) <= R.total_bound(e64)
        # ... and the reference's own fp32 results, with the term for its sum over the distinct items
        R.assert_inside(e.cpu().numpy(), G[f"ce_{name}_none"].astype(np.float64), R.entropy_bound(e64) + R.ref_entropy_bound(items, e64), f"e against the reference, {name}")
        assert abs(float(total) - float(G[f"ce_{name}_sum"])) <= R.total_bound(e64) + R.ref_total_bound(items, e64)
        assert float(e.min()) >= 0
        if name == "same":
            assert bool((e == 0).all()) and float(total) == 0.0
        if name == "distinct":
            R.assert_inside(e.cpu().numpy(), np.log(np.arange(1, 41)), R.entropy_bound(e64) + 1e-300, "e of distinct items against log(t + 1)")
        nb = torch.stack([n, n.flip(0), n])
        tb, eb = mmk.cum_entropy(nb), mmk.cum_entropy(nb, reduce="none")
        assert tb.shape == (3,) and eb.shape == (3, 40) and same_bits(tb[0], total) and same_bits(eb[0], e) and same_bits(tb[2], total)
    long_same = torch.full((2, 2584), 77, dtype=torch.int64, device=device)
    assert bool((mmk.cum_entropy(long_same, reduce="none") == 0).all()) and bool((mmk.cum_entropy(long_same) == 0).all())
    distinct = torch.randperm(2584, generator=torch.Generator().manual_seed(5)).to(device)
    e = mmk.cum_entropy(distinct, reduce="none").cpu().numpy()
    want = np.log(np.arange(1, 2585))
    worst = max(worst, R.assert_inside(e, want, R.entropy_bound(want) + 1e-300, "2584 distinct items against log(t + 1)"))
    with pytest.raises(NotImplementedError):
        mmk.cum_entropy(distinct, neg_diff=True)
    print(f"cum_entropy: worst error / bound {worst:.3f}")


def test_k_bests_is_the_order_of_a_float64_scoring(device):
    gen = np.random.default_rng(77)
    y = R.nn_case(50, 200, 33)[1]
    # clips that wander over fewer or more corpus frames: noisy copies of frames drawn from pools of different sizes
    pools = (1, 3, 10, 40, 100, 200)
    x = np.stack([y[gen.integers(0, p, 30) * (200 // p)] * np.float32(1.5) + 0.01 * gen.uniform(0, 1, (30, 33)).astype(np.float32) for p in pools])[::-1].copy()
    scorer = mmk.NeighborScorer(torch.from_numpy(y.copy()).to(device))
    xd = torch.from_numpy(x).to(device)
    _, nn = scorer(xd)
    scores64 = np.array([R.cum_entropy64(r).sum() for r in nn.cpu().numpy()])
    assert np.diff(np.sort(scores64)).min() > 4 * max(R.total_bound(R.cum_entropy64(r)) for r in nn.cpu().numpy())
    e = scorer.entropy(xd)
    tb = max(R.total_bound(R.cum_entropy64(r)) for r in nn.cpu().numpy())
    assert e.shape == (6,) and np.abs(e.cpu().numpy() - scores64).max() <= tb
    for k in (1, 3, 6):
        order, scores = scorer.k_bests(xd, k)
        assert np.array_equal(order.cpu().numpy(), np.argsort(scores64, kind="stable")[:k]) and same_bits(scores, e[order])
    assert same_bits(torch.stack([mmk.cum_entropy(n, neg_diff=False) for n in nn]), e)        # the demo's loop, clip by clip
    print(f"k_bests: worst score error / bound {np.abs(e.cpu().numpy() - scores64).max() / tb:.3f}")
