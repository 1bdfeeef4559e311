"""The clustering kernels on the MI355X (csrc/nn_search.h nn_search_kernel<1, true, NnCosineKey>, csrc/hcluster.hip) against the float64 restatements and
derived bounds of tests/hcluster_refs.py: the three entry points through the C ABI on strided, misaligned rows with NaN-filled (poisoned)
outputs and workspace, every call made twice for the same bits, and HCluster / ArgMax on device tensors against the reference's results of
tests/golden/clusters.npz.  Each test prints its worst error / bound."""
import os

import numpy as np
import pytest
import torch

import mimikit_amd as mmk
from mimikit_amd import native
from tests import hcluster_refs as H
from tests import neighbors_refs as NR
from tests.f64_bounds import check_written
from tests.strided_inputs import FLOAT_SURROUNDS, INT_SURROUNDS, MONOTONE, Strided, surround_rule

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

G = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "clusters.npz"))
SPAN = native.NN_SPAN
POISON = -7


def same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


# ------------------------------------------------------------------------------------------------------------------ self arg-max kernel
@surround_rule(*FLOAT_SURROUNDS)
def self_call(x_np, device, x_off=1):
    """mmk_nn_cosine_self_f32 on strided, misaligned rows; outputs and workspace NaN-filled (the index buffer holds -1)"""
    rows, k = x_np.shape
    lib = native.lib()
    x = Strided.of(x_np, x_off, device)
    rx = native.inv_row_norm(x.view)
    n_work = lib.mmk_nn_cosine_workspace_bytes(rows, rows)
    assert 0 < n_work <= rows * -(-rows // SPAN) * 16 + 4096
    work = torch.full((n_work // 4 + 3,), float("nan"), dtype=torch.float32, device=device)
    index = torch.full((rows + 4,), -1, dtype=torch.int64, device=device)
    best = torch.full((rows + 4,), float("nan"), dtype=torch.float32, device=device)
    native.check(lib.mmk_nn_cosine_self_f32(x.ptr, x.stride, rx.data_ptr(), rows, k, index.data_ptr(), best.data_ptr(), work.data_ptr(), n_work,
                                            native.stream_ptr(device)))
    mask = torch.zeros(best.shape, dtype=torch.bool)
    mask[:rows] = True
    check_written(best, mask, f"cos_best {rows, k}")
    idx = index.cpu().numpy()
    assert (idx[rows:] == -1).all() and (idx[:rows] >= 0).all() and (idx[:rows] < rows).all(), f"index {rows, k}"
    assert bool(torch.isnan(work[n_work // 4:]).all()), "the workspace was written beyond its size"
    return index[:rows], best[:rows]


def check_self(x_np, c, bound, device, what):
    index, best = self_call(x_np, device)
    again_i, again_b = self_call(x_np, device)
    assert torch.equal(index, again_i) and same_bits(best, again_b), f"{what}: two calls differ"
    idx, got = index.cpu().numpy(), best.cpu().numpy()
    assert (idx != np.arange(idx.shape[0])).all(), f"{what}: a row is its own nearest"
    bad = NR.index_rule_violations(idx, c, bound)
    assert not bad.any(), f"{what}: rows {np.nonzero(bad)[0][:8]} break the index rule"
    cb = np.take_along_axis(H.level_bound(x_np), idx[:, None], -1)[:, 0]
    return idx, NR.assert_inside(got, np.take_along_axis(c, idx[:, None], -1)[:, 0], cb + 1e-300, what)


@pytest.mark.parametrize("k", H.SELF_KS)
def test_self_argmax_against_the_bound(device, k):
    worst = 0.0
    for rows in H.SELF_ROWS:
        x, c, bound = H.self_case(rows, k)
        worst = max(worst, check_self(x, c, bound, device, f"rows {rows}, k {k}")[1])
    print(f"nn_cosine_self k {k}: worst cosine error / bound {worst:.3f}")


def test_self_argmax_where_the_diagonal_crosses_every_edge(device):
    x, c, bound = H.big_self_case()
    idx, worst = check_self(x, c, bound, device, f"rows {x.shape[0]}, k {x.shape[1]}")
    for a, b in H.COPIES:
        assert idx[a] == b and idx[b] == a, f"the copies {a, b} do not find each other: {idx[a], idx[b]}"
    assert idx[H.ZERO_ROW] == 0 and not (idx == H.ZERO_ROW).any()
    index, best = self_call(x, device)
    assert float(best[H.ZERO_ROW]) == 0.0
    print(f"nn_cosine_self {x.shape[0]} rows: worst cosine error / bound {worst:.3f}")


def test_self_argmax_of_zero_rows(device):
    for rows in (2, 5, 131):
        index, best = self_call(np.zeros((rows, 9), dtype=np.float32), device)
        assert index.cpu().tolist() == [1] + [0] * (rows - 1) and bool((best == 0).all())
    print("nn_cosine_self of zero rows: worst cosine error / bound 0.000")


# ------------------------------------------------------------------------------------------------------------------ components kernel
@surround_rule(*INT_SURROUNDS)
def components_call(nearest_np, device):
    n = nearest_np.shape[0]
    lib = native.lib()
    nearest = Strided.of(nearest_np.reshape(1, n), 4, device, row_stride=n, decoy=(0, n)).view[0]      # (a contiguous list between decoy frames)
    n_work = lib.mmk_nn_components_workspace_bytes(n)
    work = torch.full((n_work // 4 + 3,), POISON, dtype=torch.int32, device=device)
    labels = torch.full((n + 4,), POISON, dtype=torch.int64, device=device)
    count = torch.full((3,), POISON, dtype=torch.int64, device=device)
    native.check(lib.mmk_nn_components_i64(nearest.data_ptr(), n, labels.data_ptr(), count.data_ptr() + 8, work.data_ptr(), n_work,
                                           native.stream_ptr(device)))
    assert labels[n:].cpu().tolist() == [POISON] * 4 and count.cpu()[[0, 2]].tolist() == [POISON] * 2
    assert work[n_work // 4:].cpu().tolist() == [POISON] * 3, "the workspace was written beyond its size"
    assert torch.equal(nearest.cpu(), torch.from_numpy(nearest_np.copy())), "the input was written"
    return labels[:n], int(count[1])


@pytest.mark.parametrize("name", sorted(H.graph_cases()))
def test_components_are_integer_exact(device, name):
    nearest = H.graph_cases()[name]
    want, want_k = H.components64(nearest)
    labels, k = components_call(nearest, device)
    again, again_k = components_call(nearest, device)
    assert torch.equal(labels, again) and k == again_k
    wrong = int((labels.cpu().numpy() != want).sum())
    assert k == want_k and wrong == 0, f"{name}: {k} components (want {want_k}), {wrong} labels differ"
    print(f"nn_components {name}: {k} components, worst error / bound 0.000 (integers)")


def test_components_python_wrapper(device):
    nearest = H.graph_cases()["min_off_cycle"]
    labels, count = native.nn_components(torch.from_numpy(nearest.copy()).to(device))
    assert labels.dtype == count.dtype == torch.int64 and count.shape == () and count.device.type == "cuda"
    assert labels.cpu().tolist() == [0, 1, 1, 2, 2, 0, 0] and int(count) == 3


# ------------------------------------------------------------------------------------------------------------------ segment mean
@surround_rule(*FLOAT_SURROUNDS)
def mean_call(x_np, order_np, offsets_np, device):
    """mmk_segment_mean_f32 on strided, misaligned rows; order and offsets are contiguous lists with decoys (frames of the case, the first
    and the last offset) in front and behind"""
    (n, k), segments = x_np.shape, offsets_np.shape[0] - 1
    x = Strided.of(x_np, 3, device)
    order = Strided.of(order_np[None], 4, device, row_stride=n, decoy=(0, n))
    offsets = Strided.of(offsets_np[None], 4, device, row_stride=segments + 1, decoy=MONOTONE)
    out = Strided((segments, k), 1, device, float("nan"))
    native.check(native.lib().mmk_segment_mean_f32(x.ptr, x.stride, n, k, order.ptr, offsets.ptr, segments, out.ptr, out.stride,
                                                   native.stream_ptr(device)))
    check_written(out.buf, out.mask(), f"segment means, k {k}")
    return out.view.clone()


@pytest.mark.parametrize("k", H.MEAN_KS)
def test_segment_mean_against_the_bound(device, k):
    worst = 0.0
    for sizes in (H.MEAN_SEGMENTS, H.ONE_ROW):             # segments of 2, 3, 700 and 1 members; one row in one segment
        x_np, order_np, offsets_np, want, bound = H.mean_case(k, sizes)
        n, segments = x_np.shape[0], offsets_np.shape[0] - 1
        outs = [mean_call(x_np, order_np, offsets_np, device) for _ in range(2)]
        order, offsets = torch.from_numpy(order_np.copy()).to(device), torch.from_numpy(offsets_np.copy()).to(device)
        assert same_bits(outs[0], outs[1]), "two calls differ"
        worst = max(worst, NR.assert_inside(outs[0].cpu().numpy(), want, bound, f"segment means, k {k}, segments of {sizes}"))
        got = native.segment_mean(torch.from_numpy(x_np.copy()).to(device), order, offsets)
        assert got.shape == (segments, k) and same_bits(got, outs[0])
        single = np.diff(offsets_np) == 1                  # a segment of one member is that row, bit for bit
        assert np.array_equal(outs[0].cpu().numpy()[single].view(np.int32), x_np[order_np[offsets_np[:-1][single]]].view(np.int32))
    print(f"segment_mean k {k}: worst error / bound {worst:.3f}")


# ------------------------------------------------------------------------------------------------------------------ Python paths
@pytest.mark.parametrize("name", ("a", "b", "c", "d"))
def test_hcluster_against_the_fixture(device, name):
    x = torch.from_numpy(G[f"h_{name}_x"].copy()).to(device)
    h = mmk.HCluster().fit(x)
    assert h.labels_.device.type == "cuda" and h.labels_.dtype == torch.int64 and type(h.K_) is int
    wrong = int((h.labels_.cpu().numpy() != G[f"h_{name}_labels"]).sum()) if h.labels_.shape == G[f"h_{name}_labels"].shape else -1
    assert wrong == 0 and h.K_ == int(G[f"h_{name}_K"]), f"{name}: {wrong} labels differ, K_ {h.K_} (want {int(G[f'h_{name}_K'])})"
    again = mmk.HCluster()
    assert torch.equal(again(x), h.labels_) and again.K_ == h.K_
    # every level's rows as the device has them, against the restatement's within the derived element-wise error
    worst, xa = 0.0, x
    for lv in H.hcluster64(G[f"h_{name}_x"])["levels"]:
        if lv["err"].any():
            worst = max(worst, NR.assert_inside(xa.cpu().numpy(), lv["x"], lv["err"], f"{name}: rows of a level"))
        if lv["k"] > 1:
            labels = torch.from_numpy(lv["labels"]).to(device)
            offsets = torch.zeros((lv["k"] + 1,), dtype=torch.int64, device=device)
            offsets[1:] = torch.cumsum(torch.bincount(labels, minlength=lv["k"]), 0)
            xa = native.segment_mean(xa, torch.sort(labels, stable=True)[1], offsets)
    print(f"HCluster {name}: {h.K_} levels equal to the reference's, worst centroid error / bound {worst:.3f}")


def test_hcluster_edges(device):
    x = torch.from_numpy(G["h_two_x"].copy()).to(device)
    h = mmk.HCluster(max_iter=2).fit(x)
    assert h.K_ is None and h.labels_.shape == (64, 2) and np.array_equal(h.labels_.cpu().numpy(), G["h_two_labels"])
    assert int(h.labels_[:, 1].max()) + 1 == 4
    h = mmk.HCluster(max_iter=0).fit(x)
    assert h.K_ is None and h.labels_.shape == (64, 0) and h.labels_.dtype == torch.int64 and h.labels_.device.type == "cuda"
    h = mmk.HCluster().fit(x[:1])
    assert h.K_ == 1 and h.labels_.shape == (1, 1) and int(h.labels_[0, 0]) == 0 and h.labels_.device.type == "cuda"
    a = mmk.ArgMax()
    labels = a(x)
    assert np.array_equal(labels.cpu().numpy(), G["argmax_labels"]) and a.K_ == int(G["argmax_K"]) and type(a.K_) is int
    assert labels.dtype == torch.int64 and labels.device.type == "cuda"
    print("HCluster edges, ArgMax: worst error / bound 0.000 (integers)")


def test_hcluster_of_12000_frames_allocates_no_matrix(device):
    n, d = 12000, 32
    x = torch.rand(n, d, generator=torch.Generator().manual_seed(11)).to(device)
    mmk.HCluster().fit(x[:300])                                      # (the allocator's first blocks and the library are in place)
    torch.cuda.synchronize(device)
    torch.cuda.reset_peak_memory_stats(device)
    before = torch.cuda.memory_allocated(device)
    h = mmk.HCluster().fit(x)
    torch.cuda.synchronize(device)
    peak = torch.cuda.max_memory_allocated(device) - before
    assert peak < n * n * 4 / 10, f"peak {peak} bytes against a matrix of {n * n * 4}"
    labels = h.labels_
    assert labels.shape[0] == n and labels.dtype == torch.int64 and h.K_ == labels.shape[1]
    ks = []
    for i in range(labels.shape[1]):
        col = labels[:, i]
        uniq = torch.unique(col)
        ks.append(int(uniq.shape[0]))
        assert torch.equal(uniq, torch.arange(ks[-1], device=device)), f"column {i} does not use exactly 0 .. K - 1"
        if i:           # column i - 1 refines column i: a label of the level before goes with ONE label of this level
            pairs = torch.unique(labels[:, i - 1] * ks[-1] + col)
            assert pairs.shape[0] == ks[-2], f"column {i - 1} does not refine column {i}"
    assert all(b < a for a, b in zip(ks[:-1], ks[1:])) and ks[0] <= n // 2 and ks[-1] == 1 and bool((labels[:, -1] == 0).all())
    print(f"HCluster of {n} frames: clusters per level {ks}, peak allocation {peak} bytes, the matrix would be {n * n * 4} "
          f"(peak / cap {peak / (n * n * 4 / 10):.3f})")
