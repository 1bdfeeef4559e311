"""The segmentation kernels on the MI355X (csrc/novelty.hip) against the float64 restatements and derived bounds of tests/segment_refs.py:
mmk_novelty_f32 and mmk_novelty_finish_f32 through the C ABI on strided, misaligned clips with NaN-filled outputs and workspace, every call
made twice for the same bits, the picker against the reference's results of tests/golden/segment.npz, and the public functions of
mimikit_amd.extract.segment against the float64 cuts of a corpus on which those cuts are robust.  Each test prints its worst error / bound."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import mimikit_amd as mmk
from mimikit_amd import native
from tests import segment_refs as R
from tests.f64_bounds import check_written
from tests.strided_inputs import FLOAT_SURROUNDS, PAD, Strided, surround_rule
from tests.golden import make_golden_segment as M

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

G = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "segment.npz"))
OFFSET = 1                               # the first row 4 bytes in
NAN = float("nan")


def same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def out_buffer(n, device):
    """n floats to be written, one float in (misaligned for anything wider than 4 bytes), NaN around them"""
    buf = torch.full((n + 9,), NAN, dtype=torch.float32, device=device)
    mask = torch.zeros(buf.shape, dtype=torch.bool)
    mask[1:1 + n] = True
    return buf, mask


def halves_array(halves):
    return (C.c_int32 * len(halves))(*halves)


@surround_rule(*FLOAT_SURROUNDS)
def novelty_call(x_np, halves, device, own_norms, gap=None):
    """mmk_novelty_f32 then mmk_novelty_finish_f32 -> raw (B, n, T), scores (B, n, T), dg (B, T) as torch tensors"""
    lib = native.lib()
    B, T, D = x_np.shape
    clips = Strided.of(np.array(x_np), OFFSET, device, batch_stride=None if gap is None else (T - 1) * (D + PAD) + D + gap)
    n = len(halves)
    inv = None if own_norms else native.inv_row_norm(clips.view)
    raw, raw_mask = out_buffer(B * n * T, device)
    native.check(lib.mmk_novelty_f32(clips.ptr, clips.clip, clips.stride, native.ptr(inv), B, T, D, halves_array(halves), n, raw.data_ptr() + 4,
                                     native.stream_ptr(device)), "mmk_novelty_f32")
    what = f"B {B}, T {T}, D {D}, halves {halves}"
    check_written(raw, raw_mask, f"raw ({what})")
    assert clips.untouched(), f"{what}: the input was written"
    scores, s_mask = out_buffer(B * n * T, device)
    dg, g_mask = out_buffer(B * T, device)
    n_work = lib.mmk_novelty_finish_workspace_floats(B, n, T)
    assert 0 < n_work <= B * n * (T // 4096 + 1)
    work = torch.full((n_work + 3,), NAN, dtype=torch.float32, device=device)
    native.check(lib.mmk_novelty_finish_f32(raw.data_ptr() + 4, B, n, T, scores.data_ptr() + 4, dg.data_ptr() + 4, work.data_ptr(), n_work,
                                            native.stream_ptr(device)), "mmk_novelty_finish_f32")
    check_written(scores, s_mask, f"scores ({what})")
    check_written(dg, g_mask, f"dg ({what})")
    assert bool(torch.isnan(work[n_work:]).all()), "the workspace was written beyond its size"
    return raw[1:1 + B * n * T].reshape(B, n, T), scores[1:1 + B * n * T].reshape(B, n, T), dg[1:1 + B * T].reshape(B, T)


def check_case(T, D, halves, device, batch=1):
    x = R.frames_case(T, D, batch)
    got = novelty_call(x, halves, device, own_norms=False)
    again = novelty_call(x, halves, device, own_norms=False)
    own = novelty_call(x, halves, device, own_norms=True)
    what = f"B {batch}, T {T}, D {D}, halves {halves}"
    for a, b, c in zip(got, again, own):
        assert same_bits(a, b), f"{what}: two calls differ"
        assert same_bits(a, c), f"{what}: the kernel's own norms differ from inv_row_norm's"
    worst = 0.0
    for clip in range(batch):
        raw, scores, dg, rb, sb, gb = R.case_bounds(T, D, tuple(halves), batch, clip)
        worst = max(worst, R.assert_inside(got[0][clip].cpu().numpy(), raw, rb, f"raw ({what}, clip {clip})"),
                    R.assert_inside(got[1][clip].cpu().numpy(), scores, sb, f"scores ({what}, clip {clip})"),
                    R.assert_inside(got[2][clip].cpu().numpy(), dg, gb, f"dg ({what}, clip {clip})"))
    return worst, got


@pytest.mark.parametrize("T", R.TS)
def test_scores_against_the_bound(device, T):
    """every size around the tile, every bin count around the chunk of 32, every kernel instance (3, 4 and 5 blocks of rows); the cases hold
    a zero frame at index 0 and in the middle and two identical neighbouring frames"""
    worst = 0.0
    for D in R.DS:
        for halves in R.HALVES:
            w, got = check_case(T, D, halves, device)
            worst = max(worst, w)
            if len(halves) == 3:              # a half-width's bits do not depend on the others of the call
                for q, h in enumerate(halves):
                    alone = novelty_call(R.frames_case(T, D), [h], device, own_norms=False)[0]
                    assert same_bits(alone[:, 0], got[0][:, q]), f"T {T}, D {D}: h = {h} alone differs from h among {halves}"
    print(f"novelty T {T}: worst error / bound {worst:.3f}")


def test_two_clips_with_a_gap(device):
    worst = max(check_case(R.TILE + 1, 33, [1, 6, R.MAX_HALF], device, batch=2)[0], check_case(5, 31, [6], device, batch=2)[0])
    x = R.frames_case(R.TILE + 1, 33, 2)
    both = novelty_call(x, [6, 12], device, own_norms=False)
    for clip in range(2):
        one = novelty_call(x[clip:clip + 1], [6, 12], device, own_norms=False)
        assert all(same_bits(a[clip], b[0]) for a, b in zip(both, one)), "a clip's result depends on its neighbour"
    for T, D, halves in ((5, 31, [6]), (R.TILE + 1, 33, [6, 12])):      # the clips end to end: behind a clip's last frame lies the next clip's first
        x = R.frames_case(T, D, 2)
        assert all(same_bits(a, b) for a, b in zip(novelty_call(x, halves, device, False), novelty_call(x, halves, device, False, gap=0)))
    print(f"novelty, two clips: worst error / bound {worst:.3f}")


def test_error_codes(device):
    lib = native.lib()
    x = torch.ones(80, 8, device=device)
    raw = torch.zeros(8 * 80, device=device)
    st = native.stream_ptr(device)

    def nov(frames=80, bins=8, batch=1, halves=(6,), n=None, xp=x.data_ptr(), rp=raw.data_ptr(), stride=8):
        return lib.mmk_novelty_f32(xp, frames * stride, stride, None, batch, frames, bins, halves_array(list(halves)), len(halves) if n is None else n,
                                   rp, st)

    assert nov() == 0
    assert nov(frames=1) == -1 and nov(bins=0) == -1 and nov(batch=0) == -1 and nov(halves=(0,)) == -1 and nov(n=0) == -1
    assert nov(xp=None) == -1 and nov(rp=None) == -1 and nov(stride=-1) == -1 and nov(xp=x.data_ptr() + 2) == -1
    assert nov(halves=(native.NOVELTY_MAX_HALF + 1,)) == -3 and nov(halves=(1,) * (native.NOVELTY_MAX_KERNELS + 1)) == -3
    assert nov(halves=(native.NOVELTY_MAX_HALF,) * native.NOVELTY_MAX_KERNELS) == 0
    work = torch.zeros(16, device=device)
    sc, dg = torch.zeros(8 * 80, device=device), torch.zeros(80, device=device)

    def fin(n=1, frames=80, n_work=16, wp=work.data_ptr()):
        return lib.mmk_novelty_finish_f32(raw.data_ptr(), 1, n, frames, sc.data_ptr(), dg.data_ptr(), wp, n_work, st)

    assert fin() == 0 and fin(n=0) == -1 and fin(frames=0) == -1 and fin(wp=None) == -1
    assert fin(n=native.NOVELTY_MAX_KERNELS + 1) == -3 and fin(n=2, n_work=1) == -4
    picked = torch.zeros(80, dtype=torch.uint8, device=device)
    pw = torch.zeros(82, dtype=torch.int32, device=device)

    def pick(n=80, wb=4, wa=4, ms=0.02, n_work=82 * 4):
        return lib.mmk_pick_peaks_f32(dg.data_ptr(), n, wb, wa, ms, picked.data_ptr(), pw.data_ptr(), n_work, st)

    assert pick() == 0 and pick(n=0) == -1 and pick(wb=-1) == -1 and pick(wb=0, wa=0) == -1 and pick(ms=NAN) == -1
    assert pick(wb=native.NOVELTY_MAX_WAIT + 1) == -3 and pick(n_work=81 * 4) == -4 and pick(wb=native.NOVELTY_MAX_WAIT, wa=0) == 0
    torch.cuda.synchronize(device)
    for call, kind in ((lambda: native.novelty(x.double(), [6]), TypeError), (lambda: native.novelty(x.cpu(), [6]), RuntimeError),
                       (lambda: native.novelty(x[:1], [6]), ValueError), (lambda: native.novelty(x, [33]), NotImplementedError),
                       (lambda: native.novelty(x, [6], torch.zeros(79, device=device)), ValueError),
                       (lambda: mmk.discontinuity_scores(x[:1], [6]), ValueError), (lambda: mmk.from_recurrence_matrix(x[None]), ValueError),
                       (lambda: native.pick_peaks(dg, 0, 0), ValueError), (lambda: native.pick_peaks(dg.cpu(), 4, 4), RuntimeError)):
        with pytest.raises(kind):
            call()


def test_a_view_equals_the_contiguous_call(device):
    x = R.frames_case(2 * R.TILE + 3, 33, 2)
    wide = torch.full((2, x.shape[1], 50), 9.0, device=device)
    wide[:, :, 3:36] = torch.from_numpy(np.array(x)).to(device)
    view = wide[:, :, 3:36]
    assert not view.is_contiguous()
    want = mmk.discontinuity_scores(view.contiguous(), [6, 12])
    assert want.shape == (2, 2, x.shape[1]) and want.dtype == torch.float32 and want.is_cuda
    assert same_bits(mmk.discontinuity_scores(view, [6, 12]), want)
    assert same_bits(mmk.discontinuity_scores(view[1], [6, 12]), want[1])
    assert same_bits(mmk.discontinuity_scores(view.transpose(1, 2).contiguous().transpose(1, 2), [6, 12]), want)       # bins not contiguous: copied
    assert float(want.min(-1).values.abs().max()) == 0.0
    _, scores, _, _, sb, _ = R.case_bounds(2 * R.TILE + 3, 33, (6, 12), 2, 1)
    print(f"discontinuity_scores: worst error / bound {R.assert_inside(want[1].cpu().numpy(), scores, sb, 'scores of a view'):.3f}")


def test_picker_returns_the_reference_indices(device):
    for name, (_, n, wb, wa, ms) in M.PICKS.items():
        x = torch.from_numpy(G[f"pick_{name}_x"]).to(device)
        got = mmk.pick_globally_sorted_maxes(x, wb, wa, ms)
        assert got.dtype == torch.int64 and got.is_cuda
        assert got.cpu().tolist() == G[f"pick_{name}_out"].tolist(), f"picker input {name}"
        assert torch.equal(mmk.pick_globally_sorted_maxes(x, wb, wa, ms), got)
    # equal values: the lower index first; a long chain of candidates, each inside the next one's window (one more round each)
    x = torch.tensor([0, 3, 0, 3, 0, 0, 0, 0], dtype=torch.float32, device=device)
    assert mmk.pick_globally_sorted_maxes(x, 3, 3).cpu().tolist() == [1]
    saw = np.tile(np.float32([0.0, 1.0]), 1500) + np.arange(3000, dtype=np.float32) * np.float32(0.01)
    got = mmk.pick_globally_sorted_maxes(torch.from_numpy(saw).to(device), 3, 3, 0.0).cpu().numpy()
    assert np.array_equal(got, R.picker64(saw, 3, 3, 0.0)) and len(got) > 700


def test_cuts_of_the_corpus(device):
    """the float64 cuts are robust against any error inside the bound (tests/test_segment_refs.py), so the device path must return them"""
    x_np = R.corpus_case()
    x = torch.from_numpy(np.array(x_np)).to(device)
    cuts, scores = mmk.from_recurrence_matrix(x, R.CORPUS_HALVES, R.CORPUS_MIN_DUR, R.CORPUS_MIN_STRENGTH)
    assert cuts.dtype == torch.int64 and cuts.is_cuda and cuts.cpu().tolist() == R.CORPUS_BOUNDS
    _, s64, _, _, sb, _ = R.bounds(x_np, R.CORPUS_HALVES)
    worst = R.assert_inside(scores.cpu().numpy(), s64, sb, "corpus scores")
    seg = mmk.CutsFromRecurrenceMatrix(6, [1., 2.], R.CORPUS_MIN_DUR, R.CORPUS_MIN_STRENGTH)
    assert seg(x).cpu().tolist() == R.CORPUS_BOUNDS and seg.mx.cpu().tolist() == R.CORPUS_BOUNDS and same_bits(seg.diagonals, scores)
    assert mmk.CutsFromRecurrenceMatrix(min_dur=R.CORPUS_MIN_DUR, min_strength=R.CORPUS_MIN_STRENGTH)(x).cpu().tolist() == R.CORPUS_BOUNDS
    assert mmk.from_recurrence_matrix(x)[0].cpu().tolist() == R.CORPUS_BOUNDS
    print(f"corpus: worst score error / bound {worst:.3f}")


def test_a_constant_corpus_has_no_cuts(device):
    x = torch.from_numpy(R.constant_case()).to(device)
    cuts, scores = mmk.from_recurrence_matrix(x, [6, 12])
    assert cuts.shape == (0,) and cuts.dtype == torch.int64 and not bool(scores.any())
    assert mmk.pick_globally_sorted_maxes(torch.full((50,), 2.5, device=device), 4, 4).shape == (0,)
