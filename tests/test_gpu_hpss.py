"""The HPSS kernel on the MI355X (csrc/hpss.hip) against the restatements and derived bounds of tests/hpss_refs.py: mmk_hpss_f32 through the
C ABI on strided, misaligned clips with NaN-filled outputs, and HarmonicSource / PercussiveSource on device tensors against
tests/golden/hpss.npz.  Medians and the hard mask are compared bit for bit; each test prints its worst error / bound."""
import itertools
import os

import numpy as np
import pytest
import torch

import mimikit_amd as mmk
from mimikit_amd import native
from mimikit_amd.features.functionals import HarmonicSource, MagSpec, PercussiveSource
from tests import hpss_refs as R
from tests.f64_bounds import check_written
from tests.strided_inputs import FLOAT_SURROUNDS, PAD, Strided, surround_rule

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

G = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "hpss.npz"))
TF, TB = native.HPSS_TILE_FRAMES, native.HPSS_TILE_BINS
INF = float("inf")
OUTPUTS = ("harmonic", "percussive", "harm_median", "perc_median")


@surround_rule(*FLOAT_SURROUNDS)
def hpss_call(x_np, kernel_size, power, margin, wanted, device, what, gap=None):
    """-> {name: (batch, frames, bins) numpy} of the outputs in `wanted`; confirms that each was written exactly, and nothing else.  gap: the
    floats between a clip's last frame and the next clip's first (None: a row's padding and GAP; 0: the clips end to end)"""
    (wh, wp), (mh, mp) = R.pair(kernel_size), R.pair(margin)
    _, frames, bins = x_np.shape
    s = Strided.of(x_np, 1, device, batch_stride=None if gap is None else (frames - 1) * (bins + PAD) + bins + gap)
    outs = {name: Strided(x_np.shape, 3, device, float("nan")) for name in wanted}
    first = outs[wanted[0]]
    native.check(native.lib().mmk_hpss_f32(s.ptr, s.clip, s.stride, *x_np.shape, wh, wp, power, mh, mp,
                                           *(outs[name].ptr if name in outs else None for name in OUTPUTS), first.clip, first.stride,
                                           native.stream_ptr(device)), what)
    for name, o in outs.items():
        check_written(o.buf, o.mask(), f"{what}: {name}")
    assert s.untouched(), f"{what}: the input changed"
    return {name: o.view.cpu().numpy() for name, o in outs.items()}


def check_case(kind, batch, frames, bins, kernel_size, device, power=1.0, margin=1.0, wanted=OUTPUTS):
    what = f"{kind} {batch} x {frames} x {bins}, windows {kernel_size}, power {power}, margin {margin}"
    x = R.case_input(kind, batch, frames, bins)
    harm, perc, hm, pm, bad = R.reference(kind, batch, frames, bins, kernel_size, power, margin)
    got = hpss_call(x, kernel_size, power, margin, wanted, device, what)
    if batch > 1:                       # a window that leaves a clip meets the next clip's frames, not padding
        packed = hpss_call(x, kernel_size, power, margin, wanted, device, what, gap=0)
        assert all(R.same_bits(packed[name], got[name]) for name in wanted), f"{what}: clips end to end give other bits"
    worst = 0.0
    for name, want in (("harm_median", hm), ("perc_median", pm)):
        if name in got:
            assert R.same_bits(got[name], want), f"{what}: {name} is not scipy's, {int((got[name] != want).sum())} of {want.size} differ"
    for name, want in (("harmonic", harm), ("percussive", perc)):
        if name in got:
            if np.isinf(power):
                assert R.same_bits(got[name], want.astype(np.float32)), f"{what}: hard {name} differs"
            else:
                worst = max(worst, R.assert_inside(got[name], want, R.hpss_bound(want, x, power), f"{what}: {name}"))
    if "harmonic" in got and "percussive" in got and power == 1.0 and margin == 1.0:
        total = got["harmonic"].astype(np.float64) + got["percussive"]
        # the two masks add up to one outside `bad`; each output is inside its bound, so the sum is inside the sum of the bounds
        both = R.hpss_bound(harm, x, 1.0) + R.hpss_bound(perc, x, 1.0)
        assert bool((np.abs(total - x)[~bad] <= both[~bad]).all()), f"{what}: harmonic + percussive is not the spectrogram"
    return worst


@pytest.mark.parametrize("frames,bins", list(R.SMALL_CASES))
def test_small_axes_with_their_largest_windows(device, frames, bins):
    worst = 0.0
    for kernel_size, kind, batch in itertools.product(R.SMALL_CASES[(frames, bins)], R.KINDS, (1, 3)):
        worst = max(worst, check_case(kind, batch, frames, bins, kernel_size, device))
        check_case(kind, batch, frames, bins, kernel_size, device, INF, 1.5, ("harmonic", "percussive"))
    print(f"hpss {frames} x {bins}: worst error / bound {worst:.3f}")


@pytest.mark.parametrize("frames,bins", R.tile_shapes(TF, TB))
def test_tile_edges(device, frames, bins):
    worst = 0.0
    for i, kernel_size in enumerate(R.TILE_WINDOWS):
        for j, kind in enumerate(R.KINDS):
            batch = 3 if (i + j) % 2 else 1
            worst = max(worst, check_case(kind, batch, frames, bins, kernel_size, device))
        check_case(R.KINDS[i % 4], 1, frames, bins, kernel_size, device, INF, (1.0, 3.0), ("harmonic", "percussive"))
    print(f"hpss {frames} x {bins}: worst error / bound {worst:.3f}")


@pytest.mark.parametrize("frames,bins", list(R.LARGE_CASES))
def test_many_tiles(device, frames, bins):
    worst = 0.0
    for i, kernel_size in enumerate(R.LARGE_CASES[(frames, bins)]):
        worst = max(worst, check_case(R.KINDS[i], 3 if i == 0 else 1, frames, bins, kernel_size, device))
        check_case(R.KINDS[i + 1], 1, frames, bins, kernel_size, device, INF, 1.0, ("harmonic", "percussive"))
    print(f"hpss {frames} x {bins}: worst error / bound {worst:.3f}")


@pytest.mark.parametrize("power", R.POWERS)
def test_powers_and_margins(device, power):
    worst = 0.0
    for margin, kind in itertools.product(R.MARGINS, ("uniform", "zeros")):
        worst = max(worst, check_case(kind, 3, TF + 1, TB + 1, (31, 31), device, power, margin, ("harmonic", "percussive")))
        worst = max(worst, check_case(kind, 1, 15, 15, (31, 5), device, power, margin))
        check_case(kind, 3, TF + 1, TB + 1, (4, 63), device, INF, margin, ("harmonic", "percussive"))
    print(f"hpss power {power}: worst error / bound {worst:.3f}")


def test_each_subset_of_the_outputs_writes_only_those(device):
    subsets = [(n,) for n in OUTPUTS] + [("harmonic", "percussive"), ("percussive", "harm_median"), ("harm_median", "perc_median"), OUTPUTS]
    for wanted in subsets:
        for kernel_size in ((31, 31), (4, 63)):
            check_case("zeros", 3, TF + 1, TB - 1, kernel_size, device, 1.0, 1.0, wanted)
            check_case("ties", 1, TF + 1, TB - 1, kernel_size, device, 2.0, 1.5, wanted)


def test_two_calls_agree_and_clips_do_not_mix(device):
    x = R.case_input("uniform", 3, TF + 1, TB + 1)
    a = hpss_call(x, 31, 1.0, 1.0, OUTPUTS, device, "first")
    b = hpss_call(x, 31, 1.0, 1.0, OUTPUTS, device, "second")
    for name in OUTPUTS:
        assert R.same_bits(a[name], b[name]), name
        for clip in range(3):           # a clip alone gives what it gives inside the batch
            alone = hpss_call(x[clip:clip + 1], 31, 1.0, 1.0, (name,), device, "alone")[name]
            assert R.same_bits(alone[0], a[name][clip]), (name, clip)


def name_of(v):
    return "_".join(f"{x:g}" for x in v) if isinstance(v, tuple) else f"{v:g}"


def test_functionals_against_native_and_the_golden(device):
    s = G["hpss_x"]
    sd = torch.from_numpy(s.copy()).to(device)
    worst = 0.0
    for power in R.POWERS + (INF,):
        for margin in R.MARGINS:
            harm, perc = native.hpss(sd, 31, power, margin)
            want = R.hpss64(s, 31, power, margin)
            for cls, nat, w64, key in ((HarmonicSource, harm, want[0], "harm"), (PercussiveSource, perc, want[1], "perc")):
                got = cls(31, power, margin)(sd)
                assert got.device.type == "cuda" and got.dtype == torch.float32 and got.shape == sd.shape
                assert torch.equal(got.view(torch.int32), nat.view(torch.int32)), (cls.__name__, power, margin)
                gold = G[f"{key}_31_p{name_of(power)}_m{name_of(margin)}"]
                if np.isinf(power):
                    assert R.same_bits(got.cpu().numpy(), gold), (cls.__name__, margin)
                else:
                    bound = R.hpss_bound(w64, s, power)
                    what = f"{cls.__name__}(31, {power}, {margin})"
                    worst = max(worst, R.assert_inside(got.cpu().numpy(), w64, bound, what))
                    # the golden is a float32 evaluation inside the same bound of the same float64 values: two bounds apart at most
                    R.assert_inside(got.cpu().numpy(), gold.astype(np.float64), 2 * bound, what + " against the float32 golden")
    got = HarmonicSource((9, 5))(sd)
    R.assert_inside(got.cpu().numpy(), G["harm_9_5_p1_m1"].astype(np.float64), 2 * R.hpss_bound(R.hpss64(s, (9, 5))[0], s, 1.0), "HarmonicSource((9, 5))")
    # (B, T, F): clip by clip; a view with strides is taken in place
    sb = torch.stack([sd, sd.flip(0), 0.5 * sd])
    gb = PercussiveSource(31, 2.0, 1.5)(sb)
    assert gb.shape == sb.shape and torch.equal(gb[0], PercussiveSource(31, 2.0, 1.5)(sd))
    wide = torch.zeros(3, 20, 40, device=device)
    wide[:, :, 5:29] = sb
    assert torch.equal(PercussiveSource(31, 2.0, 1.5)(wide[:, :, 5:29]), gb)
    hm, pm = native.hpss(sd, (31, 5), harmonic=False, percussive=False, medians=True)
    want = R.medians(s, (31, 5))
    assert R.same_bits(hm.cpu().numpy(), want[0]) and R.same_bits(pm.cpu().numpy(), want[1])
    assert len(native.hpss(sd, medians=True)) == 4 and len(native.hpss(sd, percussive=False)) == 1
    print(f"HarmonicSource / PercussiveSource: worst error / bound {worst:.3f}")


def test_compose_with_magspec(device):
    x = torch.from_numpy(np.random.default_rng(5).uniform(-1, 1, size=(2, 64 * 40)).astype(np.float32)).to(device)
    mag = MagSpec(256, 64)(x)
    out = mmk.Compose(MagSpec(256, 64), HarmonicSource())(x)
    assert out.shape == mag.shape and out.device.type == "cuda" and bool(torch.isfinite(out).all())
    assert torch.equal(out, native.hpss(mag, percussive=False)[0])
    h, p = native.hpss(mag)
    assert bool(((h + p - mag).abs() <= 12 * R.U * mag + 1e-30).all())          # two outputs of 5 u each and their sum
    m = mag.cpu().numpy()
    R.assert_inside(out.cpu().numpy(), R.hpss64(m)[0], R.hpss_bound(R.hpss64(m)[0], m, 1.0), "Compose(MagSpec, HarmonicSource)")
    one = mmk.Compose(MagSpec(256, 64), PercussiveSource())(x[0])
    assert one.shape == mag.shape[1:] and torch.equal(one, p[0])


def test_limits_and_bad_arguments_raise(device):
    x = torch.rand(40, 33, device=device)
    with pytest.raises(NotImplementedError):
        native.hpss(x, kernel_size=native.HPSS_MAX_KERNEL + 1)
    with pytest.raises(NotImplementedError):
        native.hpss(torch.zeros(40, 33, dtype=torch.complex64, device=device))
    with pytest.raises(ValueError):
        HarmonicSource(31)(x[:14])
    with pytest.raises(ValueError):
        PercussiveSource((31, 63))(x[:, :30])
    for kw in (dict(kernel_size=0), dict(margin=0.5), dict(margin=(1.0, 0.5)), dict(power=0.0), dict(power=float("nan")),
               dict(harmonic=False, percussive=False)):
        with pytest.raises(ValueError):
            native.hpss(x, **kw)
    with pytest.raises(TypeError):
        native.hpss(x.double())
    # the library's own checks, on device pointers
    lib = native.lib()
    o = torch.empty_like(x)
    args = (x.data_ptr(), 40 * 33, 33, 1, 40, 33)
    tail = (o.data_ptr(), None, None, None, 40 * 33, 33, native.stream_ptr(device))
    assert lib.mmk_hpss_f32(*args, 31, 64, 1.0, 1.0, 1.0, *tail) == -3
    assert lib.mmk_hpss_f32(*args, 31, 31, 1.0, 0.5, 1.0, *tail) == -1
    assert lib.mmk_hpss_f32(*args, 31, 31, 0.0, 1.0, 1.0, *tail) == -1
    assert lib.mmk_hpss_f32(*args, 31, 31, 1.0, 1.0, 1.0, None, None, None, None, 40 * 33, 33, native.stream_ptr(device)) == -1
    with pytest.raises(NotImplementedError):
        native.check(lib.mmk_hpss_f32(*args, 64, 31, 1.0, 1.0, 1.0, *tail), "mmk_hpss_f32")
    # bins outside the contract (negative, NaN) come back without a fault
    y = x.clone()
    y[3, 4], y[7, 9] = -1.0, float("nan")
    out = native.hpss(y, medians=True)
    torch.cuda.synchronize(device)
    assert all(t.shape == y.shape for t in out)
