"""HPSS without a GPU: the restatements of tests/hpss_refs.py against scipy's own medians and the float32 restatement of librosa's masks
(tests/golden/hpss.npz), the bounds against near misses, the exports, and the argument checks of mmk_hpss_f32, which return before any
launch."""
import dataclasses as dtc
import math
import os

import numpy as np
import pytest
import torch

import mimikit_amd as mmk
from mimikit_amd import build, native
from mimikit_amd.features.functionals import HarmonicSource, Identity, MagSpec, PercussiveSource
from mimikit_amd.features.item_spec import Frame
from tests import hpss_refs as R
from tests.f64_bounds import check_near_miss

G = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "hpss.npz"))
GOLDEN_POWERS = R.POWERS + (float("inf"),)
torch.set_grad_enabled(False)


def name(v):
    return "_".join(f"{x:g}" for x in v) if isinstance(v, tuple) else f"{v:g}"


def test_median_rule_is_scipy_s():
    x = G["med_x"]                                           # (bins, frames), as librosa sees it
    assert np.any(x == 0) and np.any((x > 0) & (x < R.TINY)) and x.min() >= 0
    for w in R.WINDOWS:
        assert R.same_bits(R.median_reflect(x, w, 1), G[f"med_time_{w}"]), w
        assert R.same_bits(R.median_reflect(x, w, 0), G[f"med_freq_{w}"]), w
        harm, perc = R.medians(x.T, (w, w))                  # time-major, as the kernel takes it
        assert R.same_bits(harm.T, G[f"med_time_{w}"]) and R.same_bits(perc.T, G[f"med_freq_{w}"])
    with pytest.raises(ValueError):
        R.median_reflect(x[:3], 8, 0)


def test_restatement_against_the_float32_golden():
    s = G["hpss_x"]
    worst = 0.0
    for power in GOLDEN_POWERS:
        for margin in R.MARGINS:
            harm, perc, _, _, bad = R.hpss64(s, 31, power, margin)
            for which, want in (("harm", harm), ("perc", perc)):
                got = G[f"{which}_31_p{name(power)}_m{name(margin)}"]
                if math.isinf(power):
                    assert R.same_bits(got, want.astype(np.float32)), (which, margin)
                else:
                    worst = max(worst, R.assert_inside(got, want, R.hpss_bound(want, s, power), f"{which}, power {power}, margin {margin}"))
            assert math.isinf(power) or (bad.any() and not bad.all() and (s[bad] > 0).any())
    harm, perc, _, _, _ = R.hpss64(s, (9, 5), 1.0, 1.0)
    R.assert_inside(G["harm_9_5_p1_m1"], harm, R.hpss_bound(harm, s, 1.0), "harm, kernel (9, 5)")
    R.assert_inside(G["perc_9_5_p1_m1"], perc, R.hpss_bound(perc, s, 1.0), "perc, kernel (9, 5)")
    print(f"float32 numpy against hpss64: worst error / bound {worst:.3f}")


def test_the_parts_add_up_to_the_spectrogram():
    x = R.case_input("uniform", 1, 40, 33)
    harm, perc, _, _, bad = R.hpss64(x, 31, 1.0, 1.0)
    assert not bad.any() and np.allclose(harm + perc, x, rtol=1e-12, atol=0)


# which case shows which defect: (kind, batch, frames, bins, kernel_size, power, margin)
NEAR_MISSES = {
    "swapped_axes": ("uniform", 1, 40, 33, (31, 5), 1.0, 1.0),
    "lower_median": ("uniform", 1, 40, 33, (32, 4), 1.0, 1.0),
    "window_right": ("uniform", 1, 40, 33, (31, 31), 1.0, 1.0),
    "clamped_edge": ("uniform", 1, 40, 33, (31, 31), 1.0, 1.0),
    "whole_sample": ("uniform", 1, 40, 33, (31, 31), 1.0, 1.0),
    "margin_side": ("uniform", 1, 40, 33, (31, 31), 1.0, (1.0, 3.0)),
    "no_split_zeros": ("zeros", 1, 40, 33, (31, 31), 1.0, 1.0),
    "tiny_zero": ("zeros", 1, 40, 33, (31, 31), 1.0, 1.5),
    "crosses_clips": ("uniform", 3, 40, 33, (31, 31), 1.0, 1.0),
}


@pytest.mark.parametrize("defect", R.DEFECTS)
def test_bounds_reject_near_misses(defect):
    kind, batch, frames, bins, kernel_size, power, margin = NEAR_MISSES[defect]
    x = R.case_input(kind, batch, frames, bins)
    harm, perc, hm, pm, _ = R.hpss64(x, kernel_size, power, margin)
    dharm, dperc, dhm, dpm, _ = R.hpss64(x, kernel_size, power, margin, defect)
    if defect in ("swapped_axes", "lower_median", "window_right", "clamped_edge", "whole_sample", "crosses_clips"):
        assert not (R.same_bits(dhm, hm) and R.same_bits(dpm, pm)), f"{defect}: the medians do not show it"
    want, got = np.stack([harm, perc]), np.stack([dharm, dperc])          # (a margin of (1, 3) on the wrong side moves one output only)
    check_near_miss(torch.from_numpy(got), torch.from_numpy(want), torch.from_numpy(R.hpss_bound(want, np.stack([x, x]), power)), defect)
    # ... and the hard mask shows every defect of the medians and the margins bit for bit
    if defect not in ("no_split_zeros", "tiny_zero"):
        hard = R.hpss64(x, kernel_size, float("inf"), margin)
        dhard = R.hpss64(x, kernel_size, float("inf"), margin, defect)
        assert not (R.same_bits(hard[0], dhard[0]) and R.same_bits(hard[1], dhard[1])), defect
    assert set(NEAR_MISSES) == set(R.DEFECTS)


def test_every_case_of_the_gpu_test_has_its_branches():
    tf, tb = native.HPSS_TILE_FRAMES, native.HPSS_TILE_BINS
    for (frames, bins), windows in {**R.SMALL_CASES, **R.LARGE_CASES}.items():
        for wh, wp in windows:
            assert wh // 2 <= frames and wp // 2 <= bins and max(wh, wp) <= native.HPSS_MAX_KERNEL
    assert any(wh // 2 == f for (f, b), ws in R.SMALL_CASES.items() for wh, wp in ws)
    assert set(w for w, _ in R.TILE_WINDOWS[:8]) == set(R.WINDOWS)
    assert (tf + 1, tb - 1) in R.tile_shapes(tf, tb) and len(R.tile_shapes(tf, tb)) == 8
    z = R.case_input("zeros", 3, tf + 1, tb + 1)
    _, _, hm, pm, bad = R.hpss64(z, (31, 31), 1.0, 1.0)
    assert bad.any() and (z[bad] > 0).any() and ((z > 0) & (z < R.TINY)).any()
    assert not np.array_equal(z[0], z[1])


def test_exports_and_constants():
    header = open(os.path.join(os.path.dirname(native._HERE), "include", "mmk.h")).read()
    assert f"#define MMK_HPSS_MAX_KERNEL {native.HPSS_MAX_KERNEL}\n" in header and native.HPSS_MAX_KERNEL == 63
    assert f"#define MMK_HPSS_TILE_FRAMES {native.HPSS_TILE_FRAMES}\n" in header
    assert f"#define MMK_HPSS_TILE_BINS {native.HPSS_TILE_BINS}\n" in header
    assert "#define MMK_ABI_VERSION 6 " in header and native.ABI_VERSION == 6
    assert "int mmk_hpss_f32(const float* s, int64_t s_batch_stride, int64_t s_row_stride, int32_t batch, int64_t frames, int32_t bins," in header
    assert "hpss.hip" in build.SOURCES
    i32, i64, f32, vp = native.i32, native.i64, native.f32, native.vp
    assert native._SIGNATURES["mmk_hpss_f32"] == (i32, [vp, i64, i64, i32, i64, i32, i32, i32, f32, f32, f32, vp, vp, vp, vp, i64, i64, vp])
    assert "mmk_hpss_f32" in native.EXPORTED_SYMBOLS
    lib = native.load_library()
    assert lib.mmk_abi_version() == 6 and hasattr(lib, "mmk_hpss_f32")
    for cls in ("HarmonicSource", "PercussiveSource"):
        assert cls in mmk.features.functionals.__all__ and getattr(mmk, cls) is getattr(mmk.features.functionals, cls)


def test_configs():
    for cls in (HarmonicSource, PercussiveSource):
        f = cls()
        assert [x.name for x in dtc.fields(f) if x.name != "type"] == ["kernel_size", "power", "margin"]
        assert (f.kernel_size, f.power, f.margin) == (31, 1., 1.)
        assert f.unit is None and f.elem_type is None and f.inv == Identity()
        with pytest.raises(NotImplementedError):
            f.np_func(np.zeros((40, 33), dtype=np.float32))
        with pytest.raises(NotImplementedError):
            f(np.zeros((40, 33), dtype=np.float32))
        chain = mmk.Compose(MagSpec(256, 64), cls((31, 5), 2., (1., 3.)))
        assert chain.unit == Frame(256, 64, padding=True) and chain.elem_type == MagSpec(256, 64).elem_type
    assert HarmonicSource() != PercussiveSource() and HarmonicSource(5) == HarmonicSource(5)


def test_refusals_without_a_gpu():
    x = torch.zeros(40, 33)
    with pytest.raises(RuntimeError, match="HIP device|MI355X"):
        HarmonicSource()(x)
    with pytest.raises(RuntimeError, match="HIP device|MI355X"):
        native.hpss(x.reshape(1, 40, 33), medians=True)
    with pytest.raises(NotImplementedError, match="complex"):
        native.hpss(torch.zeros(40, 33, dtype=torch.complex64))
    with pytest.raises(NotImplementedError, match=str(native.HPSS_MAX_KERNEL)):
        PercussiveSource(kernel_size=(31, 64))(x)
    with pytest.raises(TypeError, match="float32"):
        native.hpss(x.double())
    for kw in (dict(kernel_size=0), dict(kernel_size=(31, 0)), dict(kernel_size=(1, 2, 3)), dict(margin=0.5), dict(margin=(1.0, 0.99)),
               dict(power=0.0), dict(power=-1.0), dict(power=float("nan")), dict(harmonic=False, percussive=False)):
        with pytest.raises(ValueError):
            native.hpss(x, **kw)
    with pytest.raises(ValueError):
        native.hpss(x[:14], kernel_size=31)                  # 14 frames < 31 // 2
    with pytest.raises(ValueError):
        native.hpss(x[:, :30], kernel_size=(31, 63))         # 30 bins < 63 // 2
    with pytest.raises(ValueError):
        native.hpss(torch.zeros(33))


def test_argument_checks_of_the_library_return_before_a_launch():
    """(pointer arguments are never dereferenced by the checks: every call below returns before a launch)"""
    lib = native.load_library()
    inf = float("inf")

    def call(s=16, batch=1, frames=40, bins=33, wh=31, wp=31, power=1.0, mh=1.0, mp=1.0, outs=(1024, None, None, None), row=33):
        return lib.mmk_hpss_f32(s, frames * row, row, batch, frames, bins, wh, wp, power, mh, mp, *outs, frames * row, row, None)

    assert call(wh=0) == -1 and b"hpss" in lib.mmk_last_error()
    assert call(wp=0) == -1 and call(wh=-3) == -1
    assert call(wh=native.HPSS_MAX_KERNEL + 1) == -3 and b"hpss" in lib.mmk_last_error()
    assert call(wp=native.HPSS_MAX_KERNEL + 1) == -3
    assert call(frames=14) == -1 and call(frames=15, outs=(None, None, None, None)) == -1       # 14 < 31 // 2; no output
    assert call(bins=14, row=14) == -1
    assert call(mh=0.5) == -1 and call(mp=0.999) == -1 and call(mh=float("nan")) == -1
    assert call(power=0.0) == -1 and call(power=-2.0) == -1 and call(power=float("nan")) == -1
    assert call(outs=(None, None, None, None)) == -1 and b"no output" in lib.mmk_last_error()
    assert call(frames=0) == -1 and call(bins=0) == -1 and call(batch=0) == -1
    assert call(s=None) == -1
    assert call(s=18) == -1 and call(outs=(None, 1026, None, None)) == -1                       # 4-byte alignment
    assert call(row=32) == -1                                                                   # rows overlap
    assert call(power=inf, outs=(None, None, None, None)) == -1
