"""NearestNextNeighbor's alignment on the MI355X (csrc/nnn.hip) against the restatements and derived bounds of tests/nnn_refs.py: the cost
kernel against float64 through the C ABI on strided, offset rows; the DTW kernel bit for bit against the sequential fp32 loop; both
together against float64 (last row within the bound, end column the float64 argmin or within twice the bound of it, and exactly the
planted column where one is planted); the class; one NNN event and a mixed stream through EnsembleGenerator."""
import numpy as np
import pytest
import torch

import mimikit_amd as mmk
from mimikit_amd import native
from mimikit_amd.models import NearestNextNeighbor
from tests import helpers as H
from tests import nnn_refs as R
from tests.strided_inputs import FLOAT_SURROUNDS, Strided, surround_rule

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)


def placed(a, row_pad, device):
    """the (.., rows, k) array `a` as an input of the call: base one float in, rows k + row_pad apart, clips a further 5"""
    a3 = np.ascontiguousarray(a if a.ndim == 3 else a[None])
    rs = a3.shape[2] + row_pad
    return Strided.of(a3, 1, device, row_stride=rs, batch_stride=a3.shape[1] * rs + 5, tail=3)


@surround_rule(*FLOAT_SURROUNDS)
def cost_through_abi(x, y, device):
    """mmk_inv_row_norm_f32 twice and mmk_cosine_cost_f32 on strided, offset operands -> the whole (batch, m, n_pad) cost buffer"""
    batch, n, k = x.shape
    m = y.shape[0]
    xs, ys = placed(x, 3, device), placed(y, 5, device)
    rx = torch.full((batch * n,), float("nan"), dtype=torch.float32, device=device)
    ry = torch.full((m,), float("nan"), dtype=torch.float32, device=device)
    st = native.stream_ptr(device)
    native.check(native.lib().mmk_inv_row_norm_f32(xs.ptr, xs.clip, xs.stride, batch, n, k, rx.data_ptr(), st))
    native.check(native.lib().mmk_inv_row_norm_f32(ys.ptr, 0, ys.stride, 1, m, k, ry.data_ptr(), st))
    cost = torch.full((batch, m, R.n_pad(n)), float("nan"), dtype=torch.float32, device=device)
    native.check(native.lib().mmk_cosine_cost_f32(xs.ptr, xs.clip, xs.stride, rx.data_ptr(), batch, n, ys.ptr, ys.stride, ry.data_ptr(), m, k, cost.data_ptr(), st))
    return cost.cpu().numpy()


def assert_inside(got, want, bound, what):
    bad = R.outside(got, want, bound)
    if bad.any():
        i = tuple(int(a[0]) for a in np.nonzero(bad))
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.size} outside the derived bound; at {i}: got {float(got[i]):.9g}, want {want[i]:.9g}, "
                             f"error {abs(float(got[i]) - want[i]):.3e} > bound {bound[i]:.3e}")


@pytest.mark.parametrize("k", R.KS)
def test_cost_kernel_within_the_bound_of_float64(device, k):
    """signed inputs (|.| on load), rows strided and offset by one float with NaN between them, a zero row on each side"""
    for batch in R.BATCHES:
        for n in R.NS:
            for m in R.MS_COST:
                x, y, want, bound = R.cost_case(batch, n, m, k)
                got = cost_through_abi(x, y, device)
                what = f"cost B={batch} N={n} M={m} K={k}"
                assert_inside(got[:, :, :n].transpose(0, 2, 1), want, bound, what)
                assert np.array_equal(got[:, :, n:], np.ones_like(got[:, :, n:])), f"{what}: padding"
                if n > 1:
                    assert np.array_equal(got[-1, :, n // 2], np.ones(m, dtype=np.float32)), f"{what}: zero prompt row"
                if m > 1:
                    assert np.array_equal(got[:, m // 2, :n], np.ones((batch, n), dtype=np.float32)), f"{what}: zero corpus row"


def random_cost(batch, n, m, seed):
    """(batch, m, n_pad) fp32 costs in [0, 2) with NaN in the padding lanes, and the same as (batch, n, m)"""
    rng = np.random.default_rng(seed)
    c = np.full((batch, m, R.n_pad(n)), np.nan, dtype=np.float32)
    c[:, :, :n] = rng.uniform(0, 2, size=(batch, m, n)).astype(np.float32)
    return c, np.ascontiguousarray(c[:, :, :n].transpose(0, 2, 1))


def dtw_on_device(cost, n, device):
    end, dist, row = native.dtw_subseq(torch.from_numpy(cost).to(device), n, last_row=True)
    return end.cpu().numpy(), dist.cpu().numpy(), row.cpu().numpy()


@pytest.mark.parametrize("n", R.NS)
def test_dtw_kernel_is_the_float32_loop_bit_for_bit(device, n):
    """given a cost tensor: the last row bit-identical, the end column the loop's first minimum; M around the look-ahead depth, M < N, M = 4099;
    NaN in the padding lanes must not reach the result"""
    for m in R.MS_DTW:
        cost, c = random_cost(3, n, m, 1000 * n + m)
        want = R.dtw_last_row(c)
        end, dist, row = dtw_on_device(cost, n, device)
        assert np.array_equal(row.view(np.uint32), want.view(np.uint32)), f"N={n} M={m}"
        assert np.array_equal(end, R.end_column(want)), f"N={n} M={m}"
        assert np.array_equal(dist, want.min(-1)), f"N={n} M={m}"


@pytest.mark.parametrize("n", (1, 16, 64))
def test_dtw_kernel_ties_go_to_the_first_column(device, n):
    m = 100
    cost = np.full((2, m, R.n_pad(n)), 0.5, dtype=np.float32)
    end, dist, _ = dtw_on_device(cost, n, device)
    assert np.array_equal(end, [0, 0]) and np.array_equal(dist, np.full(2, 0.5 * n, dtype=np.float32))
    # the same zero-cost diagonal at two offsets: the earlier copy wins
    cost = np.ones((1, m, R.n_pad(n)), dtype=np.float32)
    for o in (7, 23):
        cost[0, o + np.arange(n), np.arange(n)] = 0
    end, dist, row = dtw_on_device(cost, n, device)
    assert row[0, 7 + n - 1] == 0 and row[0, 23 + n - 1] == 0
    assert end[0] == 7 + n - 1 and dist[0] == 0


@pytest.mark.parametrize("k", (64, 513))
def test_alignment_against_float64(device, k):
    """both kernels: (a) the last row within the derived bound of float64; (b) the end column is float64's, or one whose float64 D lies
    within twice the bound of float64's minimum"""
    for n in R.NS:
        for m in R.MS_COST:
            x = R.frames(3 * n, k, 400 + n).reshape(3, n, k)
            y = R.frames(m, k, 500 + m)
            xd, yd = torch.from_numpy(x.copy()).to(device), torch.from_numpy(y.copy()).to(device)
            cost = native.cosine_cost(xd, yd, native.inv_row_norm(yd))
            end, dist, row = native.dtw_subseq(cost, n, last_row=True)
            end, row = end.cpu().numpy(), row.cpu().numpy()
            last64 = R.dtw_last_row(R.cosine_distances(x, y))
            bound = R.dtw_bound(last64, n, R.cost_bound(x, y).max(axis=(-1, -2)))
            assert_inside(row, last64, bound, f"last row N={n} M={m} K={k}")
            for b in range(3):
                j = int(end[b])
                assert j == R.end_column(last64[b]) or last64[b, j] - last64[b].min() <= 2 * bound[b].max(), f"end column N={n} M={m} K={k}"
            assert np.array_equal(dist.cpu().numpy(), row[np.arange(3), end])


@pytest.mark.parametrize("index", range(len(R.PLANTED)))
def test_planted_prompt_is_found_exactly(device, index):
    """a positive-gain copy of the prompt at a known offset: well-posed in float64 first (the gap exceeds twice the bound), then the end
    column must be the planted one with no allowance - through the class, one clip per offset"""
    n, m, plants = R.PLANTED[index]
    x, y, last64, ends = R.planted_case(index)
    gaps, twice = R.planted_gap(index)
    assert (gaps > twice).all() and np.array_equal(R.end_column(last64), ends), "ill-posed planted case"
    nnn = NearestNextNeighbor.from_frames(torch.from_numpy(y.copy()).to(device))
    starts = nnn.predict_start_frames(torch.from_numpy(x.copy()).to(device))
    assert starts.dtype == torch.int64 and starts.is_cuda
    assert np.array_equal(starts.cpu().numpy(), ends + 1)
    assert int(nnn.predict_start_frame(torch.from_numpy(x[1].copy()).to(device))) == ends[1] + 1


def test_class_steps_block_and_clamp(device):
    n, m, plants = R.PLANTED[0]                 # copies at 0, 100 and 241 of 257 frames: the last one ends on the corpus' last frame
    x, y, _, ends = R.planted_case(0)
    yd, xd = torch.from_numpy(y.copy()).to(device), torch.from_numpy(x.copy()).to(device)
    nnn = NearestNextNeighbor.from_frames(yd)
    clamp = lambda idx: np.minimum(idx, m - 1)
    outs = [nnn.generate_step(t, (xd,), None) for t in (5, 6, 7)]
    for s, out in enumerate(outs):
        assert out.shape == (3, 1, R.PLANT_K)
        assert np.array_equal(out[:, 0].cpu().numpy(), y[clamp(ends + 1 + s)])
    assert np.array_equal(outs[0][2, 0].cpu().numpy(), y[m - 1])       # the clamp: start 257 of 257 repeats the last frame
    # a jump in t re-aligns, here on other prompts
    out = nnn.generate_step(20, xd[[1, 0]])
    assert np.array_equal(out[:, 0].cpu().numpy(), y[ends[[1, 0]] + 1])
    # no jump: the cursors go on whatever the inputs are
    out = nnn.generate_step(21, xd[[2, 2]])
    assert np.array_equal(out[:, 0].cpu().numpy(), y[ends[[1, 0]] + 2])
    block = nnn.generate_block(xd, 20)
    assert block.shape == (3, 20, R.PLANT_K)
    nnn2 = NearestNextNeighbor.from_frames(yd)
    steps = torch.cat([nnn2.generate_step(t, xd) for t in range(20)], dim=1)
    assert torch.equal(block, steps)
    assert np.array_equal(block.cpu().numpy(), y[clamp(ends[:, None] + 1 + np.arange(20))])
    with pytest.raises(NotImplementedError, match="65"):
        nnn.predict_start_frames(torch.zeros(1, 65, R.PLANT_K, device=device))
    with pytest.raises(ValueError):
        nnn.predict_start_frames(torch.zeros(1, 4, R.PLANT_K + 1, device=device))


def test_abi_refuses_bad_sizes_with_the_field_named(device):
    z = torch.zeros(64, device=device)
    zi = torch.zeros(8, dtype=torch.int64, device=device)
    st = native.stream_ptr(device)
    p = z.data_ptr()

    def cost(batch, n, m, k):
        return native.lib().mmk_cosine_cost_f32(p, 0, 0, p, batch, n, p, 0, p, m, k, p, st)
    for args, code, word in (((1, 0, 1, 1), -1, "n = 0"), ((1, 65, 1, 1), -3, "n = 65"), ((1, 1, 0, 1), -1, "m = 0"), ((1, 1, 1, 0), -1, "k = 0"),
                             ((0, 1, 1, 1), -1, "batch = 0")):
        assert cost(*args) == code and word in native.lib().mmk_last_error().decode()
    assert native.lib().mmk_dtw_subseq_f32(p, 1, 65, 1, zi.data_ptr(), p, None, st) == -3
    assert native.lib().mmk_dtw_subseq_f32(p, 0, 1, 1, zi.data_ptr(), p, None, st) == -1
    assert native.lib().mmk_inv_row_norm_f32(p, 0, 0, 1, 1, 0, p, st) == -1


def _corpus(sr=16000, seconds=0.5):
    t = torch.arange(int(sr * seconds), dtype=torch.float32) / sr
    f = 300 + 2500 * t / seconds                          # a rising tone: every frame differs from its neighbours
    return 0.5 * torch.sin(2 * torch.pi * torch.cumsum(f, 0) / sr)


def test_ensemble_runs_an_nnn_event(device):
    sr, base_sr, feature = 16000, 22050, mmk.MagSpec(256, 64)
    nnn = NearestNextNeighbor(feature, _corpus(sr), sr=sr, device=device)
    assert nnn.snd.is_cuda and nnn.n_bins == 129 and nnn.n_frames == nnn.snd_inv_norm.shape[0]
    prompt = mmk.Resample(sr, base_sr)(_corpus(sr)[None, 1000:2500].to(device))       # a stretch of the corpus, at the base rate
    seen = []
    block = nnn.generate_block
    nnn.generate_block = lambda inputs, n_steps: seen.append((inputs, block(inputs, n_steps))) or seen[-1][1]
    seconds = 0.1
    eg = mmk.EnsembleGenerator(prompt, max_seconds=0.3, base_sr=base_sr, stream=iter([dict(generator=nnn, seconds=seconds, temperature=0.3),
                                                                                       dict(generator=nnn, seconds=10.0)]), device=device)
    torch.manual_seed(31)                                  # (Griffin-Lim draws its initial phases from the device generator)
    out = eg.run()
    n0 = prompt.shape[1]
    assert out.shape == (1, int(0.3 * base_sr)) and bool(torch.isfinite(out).all())
    assert torch.equal(out[:, :n0], prompt)
    assert len(seen) == 1
    frames_in, frames_out = seen[0]
    n_frames = int(sr * seconds) // 64 + 1                 # get_n_steps for a framed target
    assert frames_in.shape[0] == 1 and frames_in.shape[1] <= native.NNN_MAX_ROWS and frames_out.shape == (1, n_frames, 129)
    want_in = feature(mmk.Resample(base_sr, sr)(prompt))
    assert torch.equal(frames_in, want_in)
    start = int(NearestNextNeighbor.from_frames(nnn.snd).predict_start_frames(want_in)[0])
    index = torch.arange(start, start + n_frames).clamp(max=nnn.n_frames - 1)
    assert torch.equal(frames_out, nnn.snd[index.to(device)][None])
    assert 1 <= start <= nnn.n_frames
    n_new = mmk.Resample(sr, base_sr)(torch.zeros(1, (n_frames - 1) * 64, device=device)).shape[1]
    region = out[:, n0:n0 + n_new]
    assert float(region.abs().max()) > 0
    assert float(out[:, n0 + n_new:].abs().max()) == 0.0   # the second event does not fit: the tail stays blank
    # the audio itself, bit for bit: the re-walk of the clip along the restated timeline, phases redrawn under the same seed
    from tests import caller_refs as cr
    events = [cr.Ev("nnn", sr, seconds, 256, 64), cr.Ev("nnn", sr, 10.0, 256, 64)]
    tl = cr.timeline(n0, base_sr, 0.3, events)
    assert tl.slots[0].fits and not tl.slots[1].fits and (tl.slots[0].at, tl.slots[0].written) == (n0, n_new)
    again, _ = cr.rewalk(out, n0, [cr.Player(ev, nnn) for ev in events], tl, seed=31)
    assert torch.equal(again[:, n0:n0 + n_new], region) and torch.equal(again, out)


def test_ensemble_mixes_a_network_and_an_nnn_event(device):
    srnn, _, _ = H.srnn("gru")
    nnn = NearestNextNeighbor(mmk.MagSpec(256, 64), _corpus(), sr=16000, device=device)
    prompt = (torch.rand(2, 2205, generator=torch.Generator().manual_seed(6)) * 2 - 1) * 0.5
    stream = iter([dict(generator=srnn, seconds=0.02), dict(generator=nnn, seconds=0.05), dict(generator=srnn, seconds=1.0)])
    torch.manual_seed(32)
    out = mmk.EnsembleGenerator(prompt, max_seconds=0.25, base_sr=22050, stream=stream, device=device).run().cpu()
    torch.set_grad_enabled(False)
    assert out.shape == (2, int(0.25 * 22050)) and bool(torch.isfinite(out).all())
    assert torch.equal(out[:, :2205], prompt)
    seg_net, seg_nnn = out[:, 2205:2205 + 441], out[:, 2205 + 441:2205 + 441 + 1000]
    assert float(seg_net.abs().max()) > 0 and float(seg_nnn.abs().max()) > 0
    # both regions bit for bit, and silence where the third event did not fit
    from tests import caller_refs as cr
    events = [cr.Ev("class", 16000, 0.02), cr.Ev("nnn", 16000, 0.05, 256, 64), cr.Ev("class", 16000, 1.0)]
    tl = cr.timeline(2205, 22050, 0.25, events)
    assert [(s.at, s.written) for s in tl.slots] == [(2205, 441), (2646, 1059), (3705, 5512 - 3705)]
    players = [cr.Player(ev, net) for ev, net in zip(events, (srnn.to(device), nnn, srnn))]
    again, _ = cr.rewalk(out.to(device), 2205, players, tl, seed=32)
    assert torch.equal(again.cpu(), out) and float(out[:, cr.silence_mask(tl)].abs().max()) == 0.0
