"""AutoConvolve and F0Filter on the MI355X (csrc/spec_filter.hip, include/mmk_spec_filter.h) against tests/spec_filter_refs.py: both entry
points through the C ABI on clips and rows that are strided, misaligned views into longer poisoned buffers, every call made twice for the
same bits; the recorded numpy / scipy results of tests/golden/spec_filter.npz (F0Filter inside its derived bound, AutoConvolve by the ulp
rule); the sizes at which the kernel can go wrong (2 bins, one past a stride of 256, the maximum; a clip shorter than the window, one
frame more and one fewer than a workgroup takes); batches; rows beyond 2^32 bytes by the method of tests/far_cases.py; the stream contract
by the method of tests/stream_cases.py; every refusal of the header; and the two functionals inside a Compose.  Each test prints its
worst error / bound."""
import os

import numpy as np
import pytest
import torch

import mimikit_amd as mmk
from mimikit_amd import native
from tests import far_cases as FC
from tests import spec_filter_refs as R
from tests import stream_cases as S
from tests.f64_bounds import check_written
from tests.strided_inputs import FLOAT_SURROUNDS, PAD, Strided, surround_rule

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

G = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "spec_filter.npz"))
NAN = float("nan")


def draw(seed, *shape, lo=0.05, hi=3.0):
    """|N(0, 1)| as float32 times a per-frame scale U(lo, hi): no zero frame, products of a few values stay far from overflow"""
    rng = np.random.default_rng(seed)
    s = np.abs(rng.standard_normal(shape)).astype(np.float32)
    return s * rng.uniform(lo, hi, size=shape[:-1] + (1,)).astype(np.float32)


@surround_rule(*FLOAT_SURROUNDS)
def abi_once(entry, s3, params, gap, device):
    """the entry point on strided, misaligned clips, a clip `gap` elements behind the last frame of the one before it (None: GAP)"""
    lib = native.lib()
    s = Strided.of(s3, 1, device, batch_stride=None if gap is None else (s3.shape[1] - 1) * (s3.shape[2] + PAD) + s3.shape[2] + gap)
    out = Strided(s3.shape, 3, device, NAN)
    fn = lib.mmk_auto_convolve_f32 if entry == "ac" else lib.mmk_f0_filter_f32
    rc = fn(s.ptr, s.strides[0], s.strides[1], *s3.shape, *params, out.ptr, out.strides[0], out.strides[1], native.stream_ptr(device))
    native.check(rc, entry)
    what = f"{entry} {s3.shape} {params}"
    check_written(out.buf, out.mask(), what)
    assert np.array_equal(R.bits(s.view.cpu().numpy()), R.bits(s3)), f"{what}: the input was written"
    return out.view.cpu().numpy()


def abi_call(entry, s_np, params, device):
    """abi_once twice -> (B, T, F) float32 numpy; nothing but the frames of out is written.  Clips of a batch are also laid end to end
    (a gap of 0: the frame behind a clip's last is the next clip's first) for the same bits"""
    s3 = s_np if s_np.ndim == 3 else s_np[None]
    got = [abi_once(entry, s3, params, None, device) for _ in range(2)]
    what = f"{entry} {s3.shape} {params}"
    assert np.array_equal(R.bits(got[0]), R.bits(got[1])), f"{what}: two calls differ"
    if s3.shape[0] > 1:
        assert np.array_equal(R.bits(abi_once(entry, s3, params, 0, device)), R.bits(got[0])), f"{what}: clips end to end give other bits"
    return got[0].reshape(s_np.shape)


def f0_check(s_np, n_over, n_under, modes, device, what, gold_y=None):
    """the device inside the bound around the restatement, and around scipy's recorded result where there is one -> worst error / bound"""
    worst = 0.0
    for soft, normalize in modes:
        got = abi_call("f0", s_np, (n_over, n_under, int(soft), int(normalize)), device)
        want, bound = R.f0_filter64(s_np, n_over, n_under, soft, normalize)
        worst = max(worst, R.assert_inside(got, want, bound, f"{what} soft={soft} normalize={normalize} against the restatement"))
        if gold_y is not None:
            gold = R.f0_from_y(s_np, gold_y, soft, normalize)
            worst = max(worst, R.assert_inside(got, gold, bound, f"{what} soft={soft} normalize={normalize} against scipy"))
            if not soft:
                assert np.array_equal(got != 0, gold != 0), f"{what}: the hard mask differs from scipy's"
    return worst


# ------------------------------------------------------------------------------------------------------------------ the goldens
@pytest.mark.parametrize("name", sorted(R.F0_SHAPES))
def test_f0_filter_against_the_golden(device, name):
    s = R.f0_fixture(name)
    worst = max(f0_check(s, a, b, R.MODES, device, f"{name} ({a}, {b})", G[f"y_{name}_{a}_{b}"]) for a, b in R.F0_RECORDED[name])
    print(f"F0Filter {name}: {len(R.F0_RECORDED[name])} parameter pairs x 4 modes, worst error / bound {worst:.3f}")


@pytest.mark.parametrize("name", sorted(R.AC_SHAPES))
def test_auto_convolve_against_the_golden(device, name):
    s = R.ac_fixture(name)
    n = sum(R.ulp_rule(abi_call("ac", s, (k,), device), G[f"ac_{name}_k{k}"], f"{name} k={k}") for k in R.AC_WINDOWS[name])
    print(f"AutoConvolve {name}: windows {R.AC_WINDOWS[name]}, {n} elements off by one ulp; worst error / bound {float(n > 0):.3f} (ulp rule)")


# ------------------------------------------------------------------------------------------------------------------ the sizes
BINS = (2, 65, 513, 1025, 1026, R.MAX_BINS)
SOFT = ((True, True), (True, False))       # (on drawn frames no gap is asserted: the hard masks are held to the fixtures and the zero case)


@pytest.mark.parametrize("bins", BINS)
def test_bins_from_two_to_the_maximum(device, bins):
    s = draw(bins, 3, bins)
    worst = f0_check(s, 4, 4, SOFT, device, f"f0 {bins} bins")
    if bins in (2, 65, R.MAX_BINS):           # (2 and 65 bins: every harmonic but the first few lies beyond the spectrum)
        worst = max(worst, f0_check(s, R.MAX_OVERTONE, R.MAX_UNDERTONE, SOFT, device, f"f0 {bins} bins, both counts at their maximum"))
    n = R.ulp_rule(abi_call("ac", s, (3,), device), R.auto_convolve_numpy(s, 3).astype(np.float32), f"ac {bins} bins")
    print(f"{bins} bins: f0 worst error / bound {worst:.3f}, auto_convolve {n} elements off by one ulp")


@pytest.mark.parametrize("k", (2, 3, R.MAX_WINDOW))
def test_auto_convolve_frames_around_the_window_and_the_tile(device, k):
    n = 0
    for frames in (1, 2, R.TILE_FRAMES - 1, R.TILE_FRAMES + 1, 2 * R.TILE_FRAMES + 1):
        s = draw(100 * k + frames, frames, 65)
        n += R.ulp_rule(abi_call("ac", s, (k,), device), R.auto_convolve_numpy(s, k).astype(np.float32), f"ac k={k}, {frames} frames")
    # clips shorter than the window, in a batch: a window that leaves a clip meets the next clip's frames (abi_call lays them end to end too)
    short = draw(300 + k, 3, 2, 65)
    want = np.stack([R.auto_convolve_numpy(c, k) for c in short]).astype(np.float32)
    n += R.ulp_rule(abi_call("ac", short, (k,), device), want, f"ac k={k}, three clips of 2 frames")
    # longer than the longest window: frames that see a whole window and both edges.  The geometric mean of |N(0, 1)| is 0.53: scales
    # around 1.9 keep a product of 64 values within a few powers of e^9 of 1, so that log(1 + p) is neither p nor log(p) everywhere
    long = draw(7, 70, 65, lo=1.7, hi=2.1)
    n += R.ulp_rule(abi_call("ac", long, (k,), device), R.auto_convolve_numpy(long, k).astype(np.float32), f"ac k={k}, 70 frames")
    print(f"auto_convolve k={k}: T = 1, 2, {R.TILE_FRAMES - 1}, {R.TILE_FRAMES + 1}, {2 * R.TILE_FRAMES + 1}, 70: {n} elements off by one ulp; worst error / bound {float(n > 0):.3f}")


def test_f0_empty_ranges_and_each_count_at_its_maximum(device):
    s = draw(11, 2, 1025)
    for soft, normalize in R.MODES:
        got = abi_call("f0", s, (1, 2, int(soft), int(normalize)), device)
        assert not got.any() and (R.bits(got) == 0).all(), f"n_overtone = 1 with n_undertone = 2 must be all zeros (soft={soft}, normalize={normalize})"
    assert not abi_call("f0", s, (0, 0, 1, 1), device).any()
    worst = max(f0_check(s, R.MAX_OVERTONE, 4, SOFT, device, "f0 n_overtone at its maximum"),
                f0_check(s, 4, R.MAX_UNDERTONE, SOFT, device, "f0 n_undertone at its maximum"),
                f0_check(s, R.MAX_OVERTONE, 2, R.MODES, device, "f0 overtones alone"))       # y > 0 wherever z > 0: no decision is close
    only_under = abi_call("f0", s, (1, R.MAX_UNDERTONE, 1, 1), device)
    assert not only_under.any(), "undertones alone give y <= 0 everywhere"
    print(f"f0 empty ranges and maxima: worst error / bound {worst:.3f}")


# ------------------------------------------------------------------------------------------------------------------ batches, views, wrappers
def test_a_clip_does_not_depend_on_its_neighbours_or_its_place(device):
    clips = draw(5, 3, R.TILE_FRAMES + 1, 65)
    x = torch.from_numpy(clips).to(device)
    for fn in (mmk.AutoConvolve(3), mmk.AutoConvolve(4), mmk.F0Filter(), mmk.F0Filter(8, 6, False, True)):
        got = fn(x)
        assert got.shape == x.shape and got.device.type == "cuda" and got.dtype == torch.float32
        for b in range(3):
            assert S.same_bits(got[b], fn(x[b])), f"{fn}: clip {b} of the batch differs from the clip alone"
        assert S.same_bits(fn(x.flip(0)).flip(0), got), f"{fn}: a clip's place in the batch shows"
        if isinstance(fn, mmk.F0Filter):
            assert S.same_bits(fn(x[0, :3])[:1], fn(x[0, :1])), f"{fn}: a frame depends on T"
        entry, params = ("ac", (fn.window_size,)) if isinstance(fn, mmk.AutoConvolve) else ("f0", (fn.n_overtone, fn.n_undertone, int(fn.soft), int(fn.normalize)))
        assert np.array_equal(R.bits(abi_call(entry, clips, params, device)), R.bits(got.cpu().numpy())), f"{fn}: the wrapper differs from the C ABI on strided clips"
    poisoned = x.clone()
    poisoned[1] = NAN
    got = mmk.AutoConvolve(3)(poisoned)
    assert bool(torch.isfinite(got[0]).all()) and bool(torch.isfinite(got[2]).all()), "the window crossed a clip"
    assert S.same_bits(got[0], mmk.AutoConvolve(3)(x[0])) and S.same_bits(got[2], mmk.AutoConvolve(3)(x[2]))
    print("batches: worst error / bound 0.000 (bits)")


def test_a_view_of_a_wider_tensor_is_filtered_in_place(device):
    clips = torch.from_numpy(draw(6, 2, 9, 65)).to(device)
    wide = torch.zeros((2, 12, 80), device=device)
    view = wide[:, 2:11, 5:70]
    view.copy_(clips)
    for fn in (mmk.AutoConvolve(), mmk.F0Filter()):
        assert S.same_bits(fn(view), fn(clips)), f"{fn}: a strided view"
        assert S.same_bits(fn(view[1]), fn(clips[1])), f"{fn}: a strided (T, F) view"
        assert S.same_bits(fn(clips.transpose(1, 2).contiguous().transpose(1, 2)), fn(clips)), f"{fn}: bins not contiguous"
        assert S.same_bits(fn(clips[:, :1].expand(2, 9, 65)), fn(clips[:, :1].repeat(1, 9, 1))), f"{fn}: a row stride of 0"
    assert torch.equal(view, clips), "a filter wrote its input"
    view.zero_()
    assert not bool(wide.any()), "a filter wrote beside its input"
    print("views: worst error / bound 0.000 (bits)")


# ------------------------------------------------------------------------------------------------------------------ beyond 2^32 bytes
FAR_SHAPE = (2, 3, 65)


def _stream_case(entry, shape):
    def build(seed):
        return dict(s=torch.from_numpy(draw(seed, *shape)))

    def call(L, a, s):
        x, out = a["s"], a["out"]
        if entry == "mmk_auto_convolve_f32":
            return L.mmk_auto_convolve_f32(S.P(x), x.stride(0), x.stride(1), *shape, 3, S.P(out), out.stride(0), out.stride(1), s)
        return L.mmk_f0_filter_f32(S.P(x), x.stride(0), x.stride(1), *shape, 4, 4, 1, 1, S.P(out), out.stride(0), out.stride(1), s)
    return S.Case(entry, build, lambda L, i: dict(out=(shape, torch.float32)), call)


def _far_case(entry):
    case = _stream_case(entry, FAR_SHAPE)
    return FC.FarCase(case, dict(s=2, out=2), case.call, ("s_row_stride", "out_row_stride"))


FAR_CASES = [_far_case(e) for e in native.SPEC_FILTER_SYMBOLS]


@pytest.fixture(scope="module")
def canvas(device):
    free, total = torch.cuda.mem_get_info(device)
    need = FC.CANVAS * FC.WORD + 2 ** 30
    if free < need:
        pytest.skip(f"the far-offset canvas needs {need / 2 ** 30:.1f} GiB of free device memory; torch.cuda.mem_get_info reports "
                    f"{free / 2 ** 30:.1f} GiB free of {total / 2 ** 30:.1f}")
    buf = torch.empty(FC.CANVAS, dtype=torch.float32, device=device)
    buf.fill_(NAN)
    torch.cuda.synchronize()
    yield buf
    del buf
    torch.cuda.empty_cache()


@pytest.mark.parametrize("fc", FAR_CASES, ids=[c.id for c in FAR_CASES])
def test_rows_beyond_four_gib_give_the_near_twin_bits(canvas, device, fc):
    """tests/test_gpu_far_offsets.py's method on one layout: the rows of s and out 2^33 bytes apart and more, bases one element in, odd
    strides; the near twin with the same residues gives the same bits, and nothing but the rows is written anywhere in the canvas"""
    from tests import test_gpu_far_offsets as FO
    runner = FO.Runner(fc, device)
    lay = FC.build_layout(fc.specs(runner.L), "rows", "far", 1)
    assert all(p.last_row_words() * FC.WORD > 2 ** 32 for p in lay.far) and not FC.problems(lay.far, FC.CANVAS)
    what = f"{fc.id} {lay.id}"
    twin = FO.twin_buffer(lay.twin_words, device)
    rc, near = runner.run(lay.twin, twin, what + " near twin")
    assert rc == 0, (what, rc, runner.L.mmk_last_error())
    FO.assert_clean(twin, what + " near twin")
    rc, far = runner.run(lay.far, canvas, what)
    assert rc == 0, (what, rc, runner.L.mmk_last_error())
    FO.assert_clean(canvas, what)
    FO.assert_same_bits(far, near, what)
    s = runner.host["s"].numpy()
    if fc.case.entry == "mmk_auto_convolve_f32":
        want = np.stack([R.auto_convolve_numpy(c, 3) for c in s]).astype(np.float32)
        worst = float(R.ulp_rule(far["out"].numpy(), want, what) > 0)
    else:
        worst = max(R.assert_inside(far["out"].numpy()[b], *R.f0_filter64(s[b], 4, 4, True, True), what) for b in range(s.shape[0]))
    print(f"{fc.id} far rows: worst error / bound {worst:.3f}")


# ------------------------------------------------------------------------------------------------------------------ the stream contract
STREAM_CASES = [_stream_case(e, (2, 2 * R.TILE_FRAMES + 1, 257)) for e in native.SPEC_FILTER_SYMBOLS]


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


# ------------------------------------------------------------------------------------------------------------------ refusals
def test_every_refusal_of_the_header_on_device_pointers(device):
    from tests.test_spec_filter_refs import refusals
    lib = native.lib()
    s = torch.rand(2048, device=device)
    out = torch.full((2048,), NAN, device=device)
    rows = refusals(lib, s.data_ptr(), out.data_ptr())
    for name, call, code, word in rows:
        assert call() == code, (name, word)
        text = lib.mmk_last_error().decode()
        assert name in text and word in text, (name, word, text)
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all()), "a refused call wrote its output"
    x = torch.rand(5, 9, device=device)
    with pytest.raises(ValueError, match="window_size"):
        mmk.AutoConvolve(1)(x)
    with pytest.raises(NotImplementedError, match=str(native.AUTO_CONVOLVE_MAX_WINDOW)):
        native.auto_convolve(x, native.AUTO_CONVOLVE_MAX_WINDOW + 1)
    with pytest.raises(NotImplementedError, match="F0_FILTER_MAX_UNDERTONE"):
        native.f0_filter(x, 4, native.F0_FILTER_MAX_UNDERTONE + 1)
    with pytest.raises(RuntimeError, match="MI355X"):
        mmk.F0Filter()(x.cpu())
    print(f"spec_filter refusals: {len(rows)} through the C ABI; worst error / bound 0.000 (refusals)")


# ------------------------------------------------------------------------------------------------------------------ end to end
def test_filters_inside_a_compose_stay_on_the_device(device):
    g = torch.Generator().manual_seed(3)
    t = torch.arange(48000) / 16000.0
    wave = torch.cat([torch.sin(2 * torch.pi * f * t[:12000]) for f in (220.0, 880.0, 1760.0, 3520.0)]) + 0.05 * torch.randn(48000, generator=g)
    wave = wave.to(device)
    spec = mmk.MagSpec()(wave)
    reduced = mmk.Compose(mmk.MagSpec(), mmk.F0Filter(), mmk.PCA(16))(wave)
    assert reduced.device.type == "cuda" and reduced.dtype == torch.float32 and reduced.shape == (spec.shape[0], 16)
    filtered = mmk.F0Filter()(spec)
    assert filtered.device.type == "cuda" and filtered.shape == spec.shape == (reduced.shape[0], 1025)
    assert torch.equal(mmk.PCA(16)(filtered), reduced), "the filter inside a chain differs from the filter on the chain's input"
    spec_np = spec.cpu().numpy()
    worst = R.assert_inside(filtered.cpu().numpy(), *R.f0_filter64(spec_np, 4, 4, True, True), "F0Filter on a spectrogram")
    conv = mmk.Compose(mmk.MagSpec(), mmk.AutoConvolve())(wave)
    assert conv.device.type == "cuda" and conv.dtype == torch.float32 and conv.shape == spec.shape
    assert S.same_bits(conv, mmk.AutoConvolve()(spec))
    n = R.ulp_rule(conv.cpu().numpy(), R.auto_convolve_numpy(spec_np, 3).astype(np.float32), "AutoConvolve on a spectrogram")
    assert bool(torch.equal(spec, mmk.MagSpec()(wave))), "a filter wrote its input"
    print(f"Compose(MagSpec, F0Filter, PCA(16)) and Compose(MagSpec, AutoConvolve): {spec.shape[0]} frames of 1025 bins; F0Filter worst error / bound "
          f"{worst:.3f}, AutoConvolve {n} of {conv.numel()} elements off by one ulp")
