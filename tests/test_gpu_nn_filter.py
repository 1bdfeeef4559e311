"""The nearest-neighbour filter on the MI355X (csrc/nn_filter.hip, include/mmk_nn_filter.h) against tests/nn_filter_refs.py: the entry point
through the C ABI on host-drawn lists (independent of the search), x and out as row-strided, misaligned views into longer poisoned
buffers, every call made twice for the same bits - median / max / min and the counts bit for bit numpy's, the mean against its derived
bound; the wrapper's refusals; the stream contract by the method of tests/stream_cases.py; NearestNeighborFilter on device tensors against
the recorded sklearn / numpy results of tests/golden/nn_filter.npz; and the chain from a signal to labels.  Each test prints its worst
error / bound."""
import os

import numpy as np
import pytest
import torch

import mimikit_amd as mmk
from mimikit_amd import native
from tests import nn_filter_refs as R
from tests import stream_cases as S
from tests.f64_bounds import check_written
from tests.neighbors_refs import assert_inside
from tests.strided_inputs import FLOAT_SURROUNDS, Strided, surround_rule

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

G = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "nn_filter.npz"))
POISON = -7
NAN = float("nan")


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


@surround_rule(*FLOAT_SURROUNDS)
def aggregate_call(x_np, index_np, op, mutual, device, want_count=True):
    """mmk_nn_aggregate_f32 on strided, misaligned rows -> (out (n, d) float32 numpy, counts int32 numpy or None)"""
    lib = native.lib()
    n, d = x_np.shape
    t = index_np.shape[1]
    x, out = Strided.of(x_np, 1, device), Strided((n, d), 3, device, NAN)
    index = Strided.of(index_np, 4, device, row_stride=t, decoy=(0, n)).view                # (contiguous lists: decoy frames in front and behind)
    cbuf = torch.full((n + 3,), POISON, dtype=torch.int32, device=device)
    count = cbuf[1:1 + n]
    native.check(lib.mmk_nn_aggregate_f32(x.ptr, x.stride, n, d, index.data_ptr(), t, 1 if mutual else 0, native.NN_AGGREGATES.index(op), out.ptr,
                                          out.stride, count.data_ptr() if want_count else None, native.stream_ptr(device)), "mmk_nn_aggregate_f32")
    what = f"nn_aggregate {n, d, t} {op} mutual={mutual}"
    check_written(out.buf, out.mask(), what)
    edge = torch.cat([cbuf[:1], cbuf[1 + n:]]).cpu()
    assert bool((edge == POISON).all()), f"{what}: written outside count"
    if not want_count:
        assert bool((cbuf == POISON).all()), f"{what}: count was written though NULL was passed"
    assert np.array_equal(bits(x.view.cpu().numpy()), bits(x_np)) and np.array_equal(index.cpu().numpy(), index_np), f"{what}: an input was written"
    return out.view.cpu().numpy(), count.cpu().numpy() if want_count else None


def check_aggregate(x_np, index_np, op, mutual, device):
    """two calls, the same bits; the counts; selections bit for bit, the mean inside its bound -> worst error / bound"""
    what = f"nn_aggregate {x_np.shape + index_np.shape[1:]} {op} mutual={mutual}"
    got, counts = aggregate_call(x_np, index_np, op, mutual, device)
    again, none = aggregate_call(x_np, index_np, op, mutual, device, want_count=False)
    assert none is None and np.array_equal(bits(got), bits(again)), f"{what}: two calls differ"
    want, want_counts, bound = R.nn_aggregate64(x_np, index_np, op, mutual)
    assert np.array_equal(counts, want_counts), f"{what}: counts of rows {np.nonzero(counts != want_counts)[0][:8]} differ"
    if op != "mean":
        bad = bits(got) != bits(want)
        assert not bad.any(), f"{what}: {int(bad.sum())} values are not numpy's bits, first at {tuple(int(a[0]) for a in np.nonzero(bad))}"
        return 0.0
    empty = want_counts == 0
    assert np.array_equal(bits(got[empty]), bits(x_np[empty])), f"{what}: a row without a neighbour does not keep its bits"
    return assert_inside(got.astype(np.float64), want, bound, what)


# ------------------------------------------------------------------------------------------------------------------ the kernel
@pytest.mark.parametrize("op", R.OPS)
@pytest.mark.parametrize("n", R.NS)
def test_aggregate_on_drawn_lists(device, n, op):
    worst = 0.0
    for d in R.DS:
        for t in R.TS:
            x, index = R.kernel_case(n, d, t)
            for mutual in (True, False):
                worst = max(worst, check_aggregate(x, index, op, mutual, device))
    print(f"nn_aggregate n {n} {op}: {len(R.DS) * len(R.TS) * 2} cases, worst error / bound {worst:.3f}")


@surround_rule(*FLOAT_SURROUNDS)
def wrapper_on_placed_rows(x_np, index, op, device):
    """native.nn_aggregate on columns 3 .. 3 + d of rows 80 floats wide"""
    rows = Strided.of(x_np, 3, device, row_stride=80, tail=80 - 3 - x_np.shape[1])
    return native.nn_aggregate(rows.view, index, op).cpu().numpy()


@surround_rule(*FLOAT_SURROUNDS)
def filter_on_placed_clips(clips_np, op, device):
    """NearestNeighborFilter on (2, 96, 33) clips that are rows 2 .. 98 and columns 5 .. 38 of clips of 100 rows of 40 floats"""
    padded = Strided.of(clips_np, 2 * 40 + 5, device, row_stride=40, batch_stride=100 * 40)
    return mmk.NearestNeighborFilter(aggregate=op)(padded.view)


def test_aggregate_contiguous_rows_and_a_single_row_list(device):
    """the wrapper (contiguous x, torch's own out) against the C ABI call on strided rows, and lists that leave every row empty"""
    x_np, index_np = R.kernel_case(129, 65, 16)
    x, index = torch.from_numpy(x_np.copy()).to(device), torch.from_numpy(index_np.copy()).to(device)
    for op in R.OPS:
        want, want_counts = aggregate_call(x_np, index_np, op, True, device)
        out, count = native.nn_aggregate(x, index, op, mutual=True, return_count=True)
        assert np.array_equal(bits(out.cpu().numpy()), bits(want)) and np.array_equal(count.cpu().numpy(), want_counts), op
        assert count.dtype == torch.int32 and out.dtype == torch.float32 and out.shape == x.shape
        assert np.array_equal(bits(wrapper_on_placed_rows(x_np, index, op, device)), bits(want)), f"{op}: a row-strided x through the wrapper"
    nothing = torch.full((129, 3), -1, dtype=torch.int64, device=device)
    out, count = native.nn_aggregate(x, nothing, "median", return_count=True)
    assert np.array_equal(bits(out.cpu().numpy()), bits(x_np)) and int(count.abs().sum()) == 0
    one_sided = torch.arange(1, 130, dtype=torch.int64, device=device).reshape(129, 1) % 129          # i names i + 1: no link is mutual
    out, count = native.nn_aggregate(x, one_sided, "max", mutual=True, return_count=True)
    assert np.array_equal(bits(out.cpu().numpy()), bits(x_np)) and int(count.sum()) == 0
    out, count = native.nn_aggregate(x, one_sided, "max", mutual=False, return_count=True)
    assert np.array_equal(bits(out.cpu().numpy()), bits(np.roll(x_np, -1, axis=0))) and int(count.sum()) == 129
    print("nn_aggregate wrapper: worst error / bound 0.000 (bits)")


def test_wrappers_refuse_what_the_header_refuses(device):
    x = torch.zeros((40, 5), device=device)
    index = torch.zeros((40, 3), dtype=torch.int64, device=device)
    with pytest.raises(NotImplementedError, match=str(native.NN_TOPK_MAX)):
        native.nn_aggregate(x, torch.zeros((40, native.NN_TOPK_MAX + 1), dtype=torch.int64, device=device))
    with pytest.raises(TypeError):
        native.nn_aggregate(x, index.int())
    with pytest.raises(TypeError):
        native.nn_aggregate(x.double(), index)
    with pytest.raises(ValueError):
        native.nn_aggregate(x, index[:39])
    with pytest.raises(ValueError):
        native.nn_aggregate(x, index[:, :0])
    with pytest.raises(ValueError):
        native.nn_aggregate(x, index[0])
    with pytest.raises(ValueError, match="median, mean, max, min"):
        native.nn_aggregate(x, index, "sum")
    with pytest.raises(RuntimeError, match="MI355X"):
        native.nn_aggregate(x, index.cpu())
    lib = native.lib()
    out = torch.zeros_like(x)
    args = (x.data_ptr(), 5, 40, 5, index.data_ptr())
    assert lib.mmk_nn_aggregate_f32(*args, native.NN_TOPK_MAX + 1, 1, 0, out.data_ptr(), 5, None, native.stream_ptr(device)) == -3
    assert lib.mmk_nn_aggregate_f32(*args, 3, 1, 4, out.data_ptr(), 5, None, native.stream_ptr(device)) == -3
    assert lib.mmk_nn_aggregate_f32(*args, 3, 1, 0, x.data_ptr(), 5, None, native.stream_ptr(device)) == -1
    nf = mmk.NearestNeighborFilter
    with pytest.raises(ValueError, match="two frames"):
        nf()(x[:1])
    with pytest.raises(ValueError, match="n_neighbors"):
        nf(n_neighbors=0)(x)
    with pytest.raises(NotImplementedError, match=str(native.NN_TOPK_MAX)):
        nf(n_neighbors=native.NN_TOPK_MAX + 1)(x)
    with pytest.raises(NotImplementedError, match="manhattan"):
        nf(metric="manhattan")(x)
    with pytest.raises(ValueError, match="aggregate"):
        nf(aggregate="sum")(x)
    with pytest.raises(RuntimeError, match="MI355X"):
        nf()(x.cpu())
    with pytest.raises(NotImplementedError):
        nf()(x.cpu().numpy())
    print("nn_filter wrappers: worst error / bound 0.000 (refusals)")


# ------------------------------------------------------------------------------------------------------------------ the stream contract
SN, SD, ST = 129, 129, 9          # 33 workgroups with a tail, one past a step of 128 bins, an odd number of slots


def _stream_aggregate():
    def build(seed):
        g = S.gen(seed)
        index = torch.stack([torch.randperm(SN, generator=S.gen(31 + i))[:ST] for i in range(SN)])      # (the lists stay, the frames are late)
        return dict(x=S.uni(g, SN, SD), index=index)

    def call(L, a, s):
        return L.mmk_nn_aggregate_f32(S.P(a["x"]), SD, SN, SD, S.P(a["index"]), ST, 0, 0, S.P(a["out"]), SD, S.P(a["count"]), s)
    return S.Case("mmk_nn_aggregate_f32", build, lambda L, i: dict(out=((SN, SD), torch.float32), count=((SN,), torch.int32)), call)


STREAM_CASES = [_stream_aggregate()]


@pytest.mark.parametrize("case", STREAM_CASES, ids=[c.id for c in STREAM_CASES])
def test_entry_point_behind_a_busy_side_stream(device, case):
    """tests/test_gpu_streams.py's method: the real input twice on the default stream (the same bits), the stale input once (other bits),
    then behind a delay and a late write of the input on a side stream: the default-stream bits, and the call came back while the stream
    was still busy"""
    bound = S.Bound(case, device)
    want = bound.run_default("real")
    again = bound.run_default("real")
    assert not S.differs(want, again), (case.id, "two default-stream calls disagree")
    bound.check_surround(case.id + " on the default stream")
    stale = bound.run_default("stale")
    assert S.differs(want, stale), (case.id, "the stale input gives the real input's bits: the case proves nothing")
    got, busy, host = S.late_input(bound, S.side_stream(device))
    print(f"[streams] {case.id}: host time of the call {host * 1e3:.3f} ms, busy on return: {busy}")
    assert not S.differs(want, got), (case.id, "behind a late input on a side stream the outputs differ from the default-stream run")
    bound.check_surround(case.id + " on the side stream")
    assert busy, (case.id, f"the call waited for its stream (or took {host * 1e3:.1f} ms on the host)")


# ------------------------------------------------------------------------------------------------------------------ end to end
@pytest.mark.parametrize("name", sorted(R.FIXTURES))
def test_filter_against_the_golden(device, name):
    _, _, k, metric, _, _ = R.FIXTURES[name]
    x_np = R.fixture_frames(name)
    x = torch.from_numpy(x_np.copy()).to(device)
    worst = 0.0
    for op in R.OPS:
        got = mmk.NearestNeighborFilter(n_neighbors=k, metric=metric, aggregate=op)(x)
        assert got.device.type == "cuda" and got.dtype == torch.float32 and got.shape == x.shape
        got = got.cpu().numpy()
        if op == "mean":
            res = R.fixture_result(name, "mean")
            worst = assert_inside(got.astype(np.float64), res["out"], res["bound"], f"{name} mean")
        elif op == "min":
            assert np.array_equal(bits(got), bits(R.fixture_result(name, "min")["out"])), f"{name} min: not numpy's bits on the restatement's lists"
        else:
            bad = bits(got) != bits(G[f"{name}_{op}"])
            assert not bad.any(), f"{name} {op}: {int(bad.sum())} of {bad.size} values differ from the golden, rows {np.unique(np.nonzero(bad)[0])[:8]}"
    index, _ = native.nn_topk(x, x, min(k, x.shape[0] - 1), metric, self_exclude=True)
    _, count = native.nn_aggregate(x, index, "median", return_count=True)
    assert np.array_equal(count.cpu().numpy(), G[f"{name}_counts"]), f"{name}: neighbour counts"
    assert np.array_equal(x.cpu().numpy(), x_np), "the filter wrote its input"
    print(f"NearestNeighborFilter {name}: median / max / min exact, mean worst error / bound {worst:.3f}")


def test_filter_on_a_batch_is_its_clips_one_by_one(device):
    names = ("cos96", "euc96")
    clips = torch.from_numpy(np.stack([R.fixture_frames(n) for n in names])).to(device)
    for op in ("median", "mean"):
        nf = mmk.NearestNeighborFilter(aggregate=op)
        got = nf(clips)
        assert got.shape == clips.shape and got.device.type == "cuda"
        for b in range(2):
            assert S.same_bits(got[b], nf(clips[b])), f"{op}: clip {b} of the batch differs from the clip alone"
        assert S.same_bits(filter_on_placed_clips(clips.cpu().numpy(), op, device), got), f"{op}: a strided batch differs"      # clips and rows at a stride
        if op == "median":
            assert np.array_equal(bits(got[0].cpu().numpy()), bits(G["cos96_median"])), "neighbours crossed the clips"
    print("NearestNeighborFilter batch: worst error / bound 0.000 (bits)")


def test_filter_between_magspec_and_pca_stays_on_the_device(device):
    g = torch.Generator().manual_seed(3)
    t = torch.arange(48000) / 16000.0
    wave = torch.cat([torch.sin(2 * torch.pi * f * t[:12000]) for f in (220.0, 880.0, 1760.0, 3520.0)]) + 0.05 * torch.randn(48000, generator=g)
    chain = mmk.Compose(mmk.MagSpec(), mmk.NearestNeighborFilter(), mmk.PCA(16), mmk.KMeans(8))
    labels = chain(wave.to(device))
    assert labels.device.type == "cuda" and labels.dtype == torch.int64 and labels.dim() == 1
    spec = mmk.MagSpec()(wave.to(device))
    smooth = mmk.NearestNeighborFilter()(spec)
    assert smooth.device.type == "cuda" and smooth.shape == spec.shape == (labels.shape[0], 1025)
    assert torch.equal(mmk.Compose(mmk.PCA(16), mmk.KMeans(8))(smooth), labels), "the filter inside a chain differs from the filter on the chain's input"
    index, _ = native.nn_topk(spec, spec, 16, "cosine", self_exclude=True)
    want, counts, _ = R.nn_aggregate64(spec.cpu().numpy(), index.cpu().numpy(), "median")
    assert np.array_equal(bits(smooth.cpu().numpy()), bits(want)), "the filter differs from numpy's median on the device's own lists"
    print(f"Compose(MagSpec, NearestNeighborFilter, PCA(16), KMeans(8)): {labels.shape[0]} frames of 1025 bins, {int((counts == 0).sum())} without a mutual "
          f"neighbour, mean count {counts.mean():.2f}, sizes {torch.bincount(labels).cpu().tolist()}; worst error / bound 0.000 (bits)")
