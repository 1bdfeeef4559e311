"""The k-best and edge-component kernels on the MI355X (csrc/qcluster.hip, csrc/hcluster.hip) against the float64 restatements and derived
bounds of tests/qcluster_refs.py: the entry points through the C ABI on strided, misaligned rows with poisoned outputs and workspace, every
call made twice for the same bits, and QCluster on device tensors against the reference's results of tests/golden/qcluster.npz.  Each test
prints its worst error / bound."""
import os

import numpy as np
import pytest
import torch

import mimikit_amd as mmk
from mimikit_amd import native
from tests import neighbors_refs as NR
from tests import qcluster_refs as Q
from tests.f64_bounds import check_written
from tests.strided_inputs import FLOAT_SURROUNDS, INT_SURROUNDS, Strided, surround_rule

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

G = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "qcluster.npz"))
SPAN = native.NN_SPAN
POISON = -7
LIMITS = {"cosine": (-1.0, 1.0), "euclidean": (float("-inf"), float("inf"))}      # key_min, key_max: a cosine is clamped, as nn_cosine clamps it


def same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def scales(rows, metric, device):
    """(scale, shift) of the frames `rows` as a corpus: inverse norms and 0, or 1 and -|y|^2 / 2 through mmk_half_neg_sqnorm_f32 (into a
    NaN-filled buffer)"""
    if metric == "cosine":
        return native.inv_row_norm(rows.view), torch.zeros((rows.rows,), dtype=torch.float32, device=device)
    shift = torch.full((rows.rows + 3,), float("nan"), dtype=torch.float32, device=device)
    native.check(native.lib().mmk_half_neg_sqnorm_f32(rows.ptr, rows.stride, rows.rows, rows.k, shift.data_ptr(), native.stream_ptr(device)))
    mask = torch.zeros(shift.shape, dtype=torch.bool)
    mask[:rows.rows] = True
    check_written(shift, mask, "half_neg_sqnorm")
    return torch.ones((rows.rows,), dtype=torch.float32, device=device), shift[:rows.rows]


@surround_rule(*FLOAT_SURROUNDS)
def topk_call(x_np, y_np, t, metric, device):
    """mmk_nn_topk_f32 on strided, misaligned rows (y_np None: self_exclude); outputs and workspace poisoned"""
    lib = native.lib()
    x = Strided.of(x_np, 1, device)
    y = x if y_np is None else Strided.of(y_np, 2, device)
    rows, k, m = x.rows, x.k, y.rows
    cscale, cshift = scales(y, metric, device)
    qscale = cscale if y_np is None else scales(x, metric, device)[0]
    n_work = lib.mmk_nn_topk_workspace_bytes(rows, m, t)
    assert n_work == rows * -(-m // SPAN) * t * 8
    work = torch.full((n_work // 4 + 3,), float("nan"), dtype=torch.float32, device=device)
    index = torch.full((rows * t + 4,), POISON, dtype=torch.int64, device=device)
    key = torch.full((rows * t + 4,), float("nan"), dtype=torch.float32, device=device)
    native.check(lib.mmk_nn_topk_f32(x.ptr, x.stride, qscale.data_ptr(), rows, y.ptr, y.stride, cscale.data_ptr(), cshift.data_ptr(), *LIMITS[metric], m, k, t,
                                     1 if y_np is None else 0, index.data_ptr(), key.data_ptr(), work.data_ptr(), n_work,
                                     native.stream_ptr(device)))
    mask = torch.zeros(key.shape, dtype=torch.bool)
    mask[:rows * t] = True
    check_written(key, mask, f"key {rows, m, k, t}")
    assert index[rows * t:].cpu().tolist() == [POISON] * 4 and not bool((index[:rows * t] == POISON).any()), f"index {rows, m, k, t}"
    assert bool(torch.isnan(work[n_work // 4:]).all()), "the workspace was written beyond its size"
    return index[:rows * t].reshape(rows, t), key[:rows * t].reshape(rows, t)


def check_topk(x_np, y_np, key64, bound, t, metric, device, what):
    index, key = topk_call(x_np, y_np, t, metric, device)
    again_i, again_k = topk_call(x_np, y_np, t, metric, device)
    assert torch.equal(index, again_i) and same_bits(key, again_k), f"{what}: two calls differ"
    idx, got = index.cpu().numpy(), key.cpu().numpy().astype(np.float64)
    bad = Q.topk_rule_violations(idx, key64, bound, t)
    assert not bad.any(), f"{what}: rows {np.nonzero(bad)[0][:8]} break the index rule: {idx[bad][:2]}"
    valid = idx >= 0
    assert (got[~valid] == -np.inf).all(), f"{what}: an empty slot does not hold -inf"
    falling = (got[:, :-1] > got[:, 1:]) | ((got[:, :-1] == got[:, 1:]) & ((idx[:, :-1] < idx[:, 1:]) | ~valid[:, 1:]))
    assert falling.all(), f"{what}: a list is not in falling key, rising index order"
    at = np.clip(idx, 0, None)
    want, b = np.take_along_axis(key64, at, -1), np.take_along_axis(bound, at, -1)
    return idx, NR.assert_inside(got[valid], want[valid], b[valid] + 1e-300, what) if valid.any() else 0.0


# ------------------------------------------------------------------------------------------------------------------ k-best kernel
@pytest.mark.parametrize("k", Q.SELF_KS)
@pytest.mark.parametrize("metric", Q.METRICS)
def test_topk_self_against_the_bound(device, metric, k):
    worst = 0.0
    for rows in Q.SELF_ROWS:
        x, key64, bound = Q.self_case(rows, k, metric)
        for t in Q.TS:
            idx, w = check_topk(x, None, key64, bound, t, metric, device, f"{metric}, rows {rows}, k {k}, T {t}")
            worst = max(worst, w)
            assert (idx != np.arange(rows)[:, None]).all(), "a row is in its own list"
            assert (idx[:, min(t, rows - 1):] == -1).all() and (idx[:, :min(t, rows - 1)] >= 0).all()      # fewer candidates than T
            if metric == "cosine" and t == 1:
                assert np.array_equal(idx[:, 0], native.nn_cosine_self(torch.from_numpy(x.copy()).to(device))[0].cpu().numpy())
    print(f"nn_topk self {metric} k {k}: worst key error / bound {worst:.3f}")


@pytest.mark.parametrize("case", Q.CROSS_CASES)
@pytest.mark.parametrize("metric", Q.METRICS)
def test_topk_against_a_corpus(device, metric, case):
    x, y, key64, bound = Q.cross_case(*case, metric)
    worst = 0.0
    for t in Q.TS:
        idx, w = check_topk(x, y, key64, bound, t, metric, device, f"{metric}, {case}, T {t}")
        worst = max(worst, w)
        assert (idx[:, min(t, case[1]):] == -1).all() and (idx[:, :min(t, case[1])] >= 0).all()
        if metric == "cosine" and t == 1:
            yd = torch.from_numpy(y.copy()).to(device)
            assert np.array_equal(idx[:, 0], native.nn_cosine(torch.from_numpy(x.copy()).to(device), yd, native.inv_row_norm(yd))[0].cpu().numpy())
    print(f"nn_topk {metric} {case}: worst key error / bound {worst:.3f}")


@pytest.mark.parametrize("metric", Q.METRICS)
def test_topk_where_the_diagonal_crosses_every_edge(device, metric):
    x, key64, bound = Q.big_case(metric)
    idx, worst = check_topk(x, None, key64, bound, 9, metric, device, f"{metric}, rows {x.shape[0]}, k {x.shape[1]}")
    for a, b in Q.COPIES:
        assert idx[a, 0] == b and idx[b, 0] == a, f"the copies {a, b} do not find each other in slot 0: {idx[a, 0], idx[b, 0]}"
        assert np.array_equal(idx[a, 1:], idx[b, 1:]), "two identical rows have different lists"
    assert (idx != np.arange(x.shape[0])[:, None]).all()
    if metric == "cosine":
        assert idx[Q.ZERO_ROW].tolist() == list(range(9)), "a zero row has cosine 0 to everything: the first frames"
        xd = torch.from_numpy(x.copy()).to(device)
        first, _ = native.nn_topk(xd, xd, 1, "cosine", self_exclude=True)
        assert torch.equal(first[:, 0], native.nn_cosine_self(xd)[0]), "T = 1 differs from nn_cosine_self"
        assert np.array_equal(first[:, 0].cpu().numpy(), idx[:, 0])
    print(f"nn_topk self {metric} {x.shape[0]} rows: worst key error / bound {worst:.3f}")


@pytest.mark.parametrize("metric", Q.METRICS)
def test_topk_of_zero_rows_and_the_wrapper(device, metric):
    zeros = np.zeros((5, 9), dtype=np.float32)
    index, key = topk_call(zeros, None, 9, metric, device)
    for r in range(5):
        assert index[r].cpu().tolist() == [j for j in range(5) if j != r] + [-1] * 5
    assert bool((key[:, :4] == 0).all()) and bool((key[:, 4:] == float("-inf")).all())
    x, y, key64, bound = Q.cross_case(*Q.CROSS_CASES[1], metric)
    want_i, want_k = topk_call(x, y, 9, metric, device)
    xd, yd = torch.from_numpy(x.copy()).to(device), torch.from_numpy(y.copy()).to(device)
    got_i, got_k = native.nn_topk(xd, yd, 9, metric)
    assert got_i.dtype == torch.int64 and got_k.dtype == torch.float32 and got_i.shape == got_k.shape == (200, 9)
    assert torch.equal(got_i, want_i) and same_bits(got_k, want_k)
    with pytest.raises(NotImplementedError, match=str(native.NN_TOPK_MAX)):
        native.nn_topk(xd, yd, native.NN_TOPK_MAX + 1, metric)
    with pytest.raises(NotImplementedError):
        native.nn_topk(xd, yd, 2, "manhattan")
    with pytest.raises(ValueError):
        native.nn_topk(xd, yd, 2, metric, self_exclude=True)
    with pytest.raises(ValueError):
        native.nn_topk(xd, yd[:, :5], 2, metric)
    with pytest.raises(RuntimeError):
        native.nn_topk(xd.cpu(), yd, 2, metric)
    print(f"nn_topk {metric} zero rows, wrapper: worst error / bound 0.000")


# ------------------------------------------------------------------------------------------------------------------ edge components
@surround_rule(*INT_SURROUNDS, may_place_nothing=True)
def components_call(src_np, dst_np, n, device):
    lib = native.lib()
    e = src_np.shape[0]
    # (contiguous lists: decoy frames of the case in front and behind; an empty list is a NULL pointer)
    src, dst = (Strided.of(a.reshape(1, e), 4, device, row_stride=e, decoy=(0, n)).view[0] if e else torch.from_numpy(a.copy()).to(device) for a in (src_np, dst_np))
    n_work = lib.mmk_edge_components_workspace_bytes(n)
    assert 0 < n_work <= 13 * n + 8
    work = torch.full((n_work // 4 + 3,), POISON, dtype=torch.int32, device=device)
    labels = torch.full((n + 4,), POISON, dtype=torch.int64, device=device)
    count = torch.full((3,), POISON, dtype=torch.int64, device=device)
    native.check(lib.mmk_edge_components_i64(src.data_ptr() if e else None, dst.data_ptr() if e else None, e, n, labels.data_ptr(),
                                             count.data_ptr() + 8, work.data_ptr(), n_work, native.stream_ptr(device)))
    assert labels[n:].cpu().tolist() == [POISON] * 4 and count.cpu()[[0, 2]].tolist() == [POISON] * 2
    assert work[n_work // 4:].cpu().tolist() == [POISON] * 3, "the workspace was written beyond its size"
    assert np.array_equal(src.cpu().numpy(), src_np) and np.array_equal(dst.cpu().numpy(), dst_np), "the input was written"
    return labels[:n], int(count[1])


@pytest.mark.parametrize("name", sorted(Q.edge_cases()))
def test_edge_components_are_integer_exact(device, name):
    src, dst, n = Q.edge_cases()[name]
    want, want_k = Q.edge_components64(src, dst, n)
    labels, k = components_call(src, dst, n, device)
    again, again_k = components_call(src, dst, n, device)
    assert torch.equal(labels, again) and k == again_k
    wrong = int((labels.cpu().numpy() != want).sum())
    assert k == want_k and wrong == 0, f"{name}: {k} components (want {want_k}), {wrong} labels differ"
    print(f"edge_components {name}: {k} components, worst error / bound 0.000 (integers)")


def test_edge_components_python_wrapper(device):
    src, dst, n = Q.edge_cases()["repeated_reversed_9"]
    labels, count = native.edge_components(torch.from_numpy(src.copy()).to(device), torch.from_numpy(dst.copy()).to(device), n)
    assert labels.dtype == count.dtype == torch.int64 and count.shape == () and count.device.type == "cuda"
    assert labels.cpu().tolist() == [0, 1, 1, 2, 3, 4, 5, 6, 6] and int(count) == 7
    empty = torch.zeros((0,), dtype=torch.int64, device=device)
    labels, count = native.edge_components(empty, empty, 3)
    assert labels.cpu().tolist() == [0, 1, 2] and int(count) == 3
    with pytest.raises(TypeError):
        native.edge_components(empty.int(), empty, 3)
    with pytest.raises(RuntimeError):
        native.edge_components(empty.cpu(), empty.cpu(), 3)


# ------------------------------------------------------------------------------------------------------------------ QCluster
@pytest.mark.parametrize("name", sorted(Q.FIXTURES))
def test_qcluster_against_the_fixture(device, name):
    metric, params = Q.FIXTURES[name][3:]
    x = torch.from_numpy(G[f"{name}_x"].copy()).to(device)
    q = mmk.QCluster(metric=metric, **params).fit(x)
    assert q.labels_.device.type == "cuda" and q.labels_.dtype == torch.int64 and q.labels_.shape == (x.shape[0],) and type(q.K_) is int
    assert q.is_core_.device.type == "cuda" and q.is_core_.dtype == torch.bool and q.is_core_.shape == (x.shape[0],)
    wrong = int((q.labels_.cpu().numpy() != G[f"{name}_labels"]).sum())
    wrong_cores = int((q.is_core_.cpu().numpy() != G[f"{name}_is_core"]).sum())
    print(f"QCluster {name}: K_ {q.K_} (want {int(G[f'{name}_K'])}), {wrong} labels and {wrong_cores} cores differ from the reference's")
    assert wrong == 0 and wrong_cores == 0 and q.K_ == int(G[f"{name}_K"])
    again = mmk.QCluster(metric=metric, **params)
    assert torch.equal(again(x), q.labels_) and again.K_ == q.K_ and torch.equal(again.is_core_, q.is_core_)


def test_qcluster_edges(device):
    x = torch.from_numpy(G["between_x"].copy()).to(device)
    with pytest.raises(NotImplementedError, match="manhattan"):
        mmk.QCluster(metric="manhattan").fit(x)
    with pytest.raises(NotImplementedError, match=str(native.NN_TOPK_MAX)):
        mmk.QCluster(n_neighbors=native.NN_TOPK_MAX + 1).fit(x)
    with pytest.raises(NotImplementedError, match=str(native.NN_TOPK_MAX)):
        mmk.QCluster(n_neighbors=None).fit(torch.zeros(((native.NN_TOPK_MAX + 1) ** 2, 2), device=device))
    with pytest.raises(ValueError):
        mmk.QCluster().fit(x[:8])                    # N <= n
    with pytest.raises(RuntimeError):
        mmk.QCluster().fit(x.cpu())
    with pytest.raises(NotImplementedError):
        mmk.QCluster().np_func(G["between_x"])
    q = mmk.QCluster().fit(x[:9])                    # the smallest corpus n = 8 takes: every list is all the other frames
    assert q.K_ == int(q.labels_.max()) + 1 and bool(q.is_core_.any())
    one = mmk.QCluster(cores_prop=0.0).fit(x)        # the largest in-degree alone is a core (here one frame): the reference raises
    if int(one.is_core_.sum()) == 1:
        assert one.K_ == 1 and bool((one.labels_ == 0).all())
    print("QCluster edges: worst error / bound 0.000 (integers)")


def test_qcluster_of_12000_frames_allocates_no_matrix(device):
    n, d = 12000, 32
    g = torch.Generator().manual_seed(12)
    centres = torch.rand(7, d, generator=g) * 2 - 1
    x = (centres[torch.randint(0, 7, (n,), generator=g)] + 0.3 * torch.randn(n, d, generator=g)).to(device)
    mmk.QCluster().fit(x[:300])                                      # (the allocator's first blocks and the library are in place)
    torch.cuda.synchronize(device)
    torch.cuda.reset_peak_memory_stats(device)
    before = torch.cuda.memory_allocated(device)
    q = mmk.QCluster().fit(x)
    torch.cuda.synchronize(device)
    peak = torch.cuda.max_memory_allocated(device) - before
    assert peak < n * n * 4 / 10, f"peak {peak} bytes against a matrix of {n * n * 4}"
    uniq = torch.unique(q.labels_)
    assert q.labels_.shape == (n,) and torch.equal(uniq, torch.arange(q.K_, device=device)), "the labels do not use exactly 0 .. K_ - 1"
    print(f"QCluster of {n} frames: K_ {q.K_}, {int(q.is_core_.sum())} cores, peak allocation {peak} bytes, the matrix would be {n * n * 4} "
          f"(peak / cap {peak / (n * n * 4 / 10):.3f})")
