"""The envelope family without a GPU: the float64 restatements of tests/envelope_refs.py against the reference's own results
(tests/golden/envelope.npz), the numpy paths of Interpolate and Derivative, the configs, the refusals, and the bounds against near misses."""
import dataclasses as dtc
import math
import os

import numpy as np
import pytest
import torch

import mimikit_amd as mmk
from mimikit_amd import native
from mimikit_amd.features.functionals import Continuous, Derivative, Envelop, EnvelopBank, Identity, Interpolate, MagSpec
from mimikit_amd.features.item_spec import Frame, Sample
from tests import envelope_refs as R
from tests.f64_bounds import check_near_miss

G = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "envelope.npz"))
LAGS = (1, 3, 9, 33)
TARGETS = {"length100": dict(length=100), "length13": dict(length=13), "length37": dict(length=37), "factor3": dict(factor=3)}
torch.set_grad_enabled(False)


def test_derivative_restatement_against_the_reference():
    x = G["deriv_x"]
    x64 = x.astype(np.float64)
    worst = 0.0
    for lag in LAGS:
        want, bound = R.derivative_ref(x64, lag), R.derivative_bound(x64, lag)
        for kind in ("torch", "np"):
            worst = max(worst, R.assert_inside(G[f"deriv_{kind}_2d_{lag}"], want, bound, f"derivative_{kind}, 2-D, max_lag {lag}"))
            R.assert_inside(G[f"deriv_{kind}_1d_{lag}"], want[0], bound[0], f"derivative_{kind}, 1-D, max_lag {lag}")
        # the sequential fp32 restatement makes the reference's roundings in the reference's order
        assert np.array_equal(R.derivative_ref(x, lag), G[f"deriv_torch_2d_{lag}"])
    print(f"reference derivative: worst error / bound {worst:.3f}")


def test_derivative_np_func_is_the_reference_s():
    x = G["deriv_x"]
    for lag in LAGS:
        assert np.array_equal(Derivative(max_lag=lag).np_func(x.copy()), G[f"deriv_np_2d_{lag}"])
        assert np.array_equal(Derivative(max_lag=lag)(x[0].copy()), G[f"deriv_np_1d_{lag}"])
    got = Derivative(max_lag=3, normalize=True).np_func(x.copy())
    assert np.array_equal(got, G["deriv_np_normalized_3"]) and got.dtype == np.float32
    assert np.abs(got).max(-1).tolist() == [1.0, 1.0, 1.0]
    with pytest.raises(ValueError, match="1 or 2 dimensions"):
        Derivative().np_func(np.zeros((2, 2, 8), dtype=np.float32))


def scipy_knot_term(x64, n_out):
    """scipy's own rounding where a position is a knot k: it evaluates (y[k] - y[k-1]) * 1 + y[k-1] with the difference taken in float32"""
    n = x64.shape[-1]
    pos = np.linspace(0, n - 1, n_out)
    k = np.floor(pos).astype(np.int64)
    at_knot = (pos == k) & (k >= 1)
    return at_knot * R.U * (np.abs(x64[..., np.maximum(k - 1, 0)]) + np.abs(x64[..., k]))


def test_interpolation_restatement_against_the_reference():
    x = G["interp_x"]
    x64 = x.astype(np.float64)
    for key, kw in TARGETS.items():
        n_out = kw.get("length", 3 * x.shape[-1])
        want, bound = R.interp_ref(x64, n_out, "linear", 1)
        R.assert_inside(G[f"interp_np_linear_{key}"], want, bound + scipy_knot_term(x64, n_out) + R.U * np.abs(want), f"scipy linear, {key}")
        assert np.array_equal(R.interp_ref(x, n_out, "previous", 1, np.float32)[0], G[f"interp_np_previous_{key}"]), key
        want, bound = R.interp_ref(x64, n_out, "linear", 0)
        R.assert_inside(G[f"interp_torch_2d_{key}"], want, bound, f"torch linear, 2-D, {key}")
        R.assert_inside(G[f"interp_torch_1d_{key}"], want[0], bound[0], f"torch linear, 1-D, {key}")
        for mode in ("linear", "previous"):      # np_func: the same scipy call
            got = Interpolate(mode=mode, **kw).np_func(x.copy())
            assert np.array_equal(got, G[f"interp_np_{mode}_{key}"]) and got.dtype == np.float32
    # the restated positions are torch's at the sizes of the GPU test as well
    for n, n_out in R.INTERP_SIZES:
        xc = R.case_input(n)
        t = torch.nn.functional.interpolate(torch.from_numpy(xc.copy())[None], n_out, mode="linear")[0].numpy()
        want, bound = R.interp_ref(xc.astype(np.float64), n_out, "linear", 0)
        R.assert_inside(t, want, bound, f"torch linear {n} -> {n_out}")


def test_envelop_by_parts_restatement():
    """the steps after the transform, over the float64 frame sums of the fixture: interpolation at scipy's positions, division by the maximum"""
    T = G["env_x"].shape[0]
    for n_fft, hop in ((256, 64), (1024, 256)):
        e = G[f"env_{n_fft}_sum"]
        keep = MagSpec(n_fft, hop, center=True, pad_mode="reflect").stft.fixed_length(T)
        assert keep == int(G[f"env_{n_fft}_fixed_length"]) and e.shape == (R.n_frames(keep, n_fft, hop, 1),)
        want, bound = R.interp_ref(e, T, "linear", 1)
        R.assert_inside(G[f"env_{n_fft}_interp"], want, bound, f"Envelop {n_fft}: Interpolate(length=T)")
        R.assert_inside(G[f"env_{n_fft}_interp_normalized"], want / want.max(), 2 * R.U * want / want.max() + bound / want.max(), f"Envelop {n_fft}: / max")
        # the frame sums themselves are the energy restatement's
        x64 = torch.from_numpy(G["env_x"][-keep:].astype(np.float64))[None]
        s, sb = R.energy_ref(x64, n_fft, hop, 1, 1)
        assert np.allclose(s[0].numpy(), e, rtol=1e-12, atol=0)


def test_sequential_fp32_restatements_stay_inside_the_bounds():
    worst = {"derivative": 0.0, "interp align 1": 0.0, "interp align 0": 0.0, "energy": 0.0}
    for L, n in R.DERIV_CASES:
        want, bound = R.derivative_reference(L, n)
        worst["derivative"] = max(worst["derivative"], R.assert_inside(R.derivative_ref(R.case_input(n, seed=L), L), want, bound, f"derivative {L}, {n}"))
    for n, n_out in R.INTERP_SIZES:
        x = R.case_input(n)
        for align in (1, 0):
            want, bound = R.interp_ref(x.astype(np.float64), n_out, "linear", align)
            got = R.interp_ref(x, n_out, "linear", align, np.float32)[0]
            worst[f"interp align {align}"] = max(worst[f"interp align {align}"], R.assert_inside(got, want, bound, f"interp {n} -> {n_out}, align {align}"))
    for n_fft in (64, 1024):
        for hop, center, reflect, n in R.energy_cases(n_fft):
            want, bound = R.energy_reference(n_fft, hop, center, reflect, n)
            S, _ = R.B.stft_ref(torch.from_numpy(R.case_input(n).copy()), n_fft, hop, bool(center), "reflect" if reflect else "constant",
                                window=R.B.hann64(n_fft).float())
            worst["energy"] = max(worst["energy"], R.assert_inside(S.abs().sum(-1).numpy(), want, bound, f"energy {n_fft}, {hop}, {center}, {reflect}, {n}"))
    print(worst)
    assert max(worst.values()) <= 0.5          # (the constants carry a factor 2 over what a sequential fp32 evaluation needs)


def test_bounds_reject_near_misses():
    for L, n in ((3, 4), (9, 10), (33, 5000), (R.MAX_LAG, 2 * R.TILE + 5)):
        x64 = R.case_input(n, seed=L).astype(np.float64)
        want, bound = R.derivative_reference(L, n)
        for defect in ("even", "no_1/d"):
            check_near_miss(torch.from_numpy(R.derivative_ref(x64, L, defect)), torch.from_numpy(want), torch.from_numpy(bound), f"derivative {L}, {n}: {defect}")
    for n, n_out in ((2, 5), (300, 4097), (100, 13)):
        x64 = R.case_input(n).astype(np.float64)
        for align in (1, 0):
            want, bound = R.interp_ref(x64, n_out, "linear", align)
            swapped = R.interp_ref(x64, n_out, "linear", 1 - align)[0]
            check_near_miss(torch.from_numpy(swapped), torch.from_numpy(want), torch.from_numpy(bound), f"interp {n} -> {n_out}: align swapped")
    for n_fft in (64, 256, 1024, 2048, 4096):
        hop = n_fft // 4
        n = 66 * hop + 1
        x64 = torch.from_numpy(R.case_input(n).astype(np.float64))
        want, bound = R.energy_ref(x64, n_fft, hop, 1, 1)
        for defect in ("shift", "symmetric", "nyquist"):
            check_near_miss(R.energy_ref(x64, n_fft, hop, 1, 1, defect)[0], want, bound, f"energy {n_fft}: {defect}")


def test_constants_are_the_header_s():
    header = open(os.path.join(os.path.dirname(native._HERE), "include", "mmk.h")).read()
    assert f"#define MMK_DERIV_MAX_LAG {native.DERIV_MAX_LAG}" in header and native.DERIV_MAX_LAG >= 64
    assert f"#define MMK_DERIV_TILE {native.DERIV_TILE}" in header
    assert f"#define MMK_INTERP_LINEAR {native.INTERP_MODES['linear']}" in header
    assert f"#define MMK_INTERP_PREVIOUS {native.INTERP_MODES['previous']}" in header
    assert "#define MMK_ABI_VERSION 6 " in header and native.ABI_VERSION == 6


def test_configs():
    def names(cfg):          # (Config adds its own `type` tag in front)
        return [f.name for f in dtc.fields(cfg) if f.name != "type"]

    e = Envelop()
    assert names(e) == ["n_fft", "hop_length", "normalize", "window", "interp_to_time_domain"]
    assert (e.n_fft, e.hop_length, e.normalize, e.window, e.interp_to_time_domain) == (2048, 512, True, "hann", True)
    assert e.fft == MagSpec(2048, 512, center=True, window="hann", pad_mode="reflect")
    assert e.unit == Sample(None) and e.elem_type == Continuous(0., 1., 1) and e.inv == Identity()
    e = Envelop(256, 64, normalize=False, interp_to_time_domain=False)
    assert e.unit == Frame(256, 64, padding=True) and e.elem_type == Continuous(0., float("inf"), 1)
    with pytest.raises(NotImplementedError):
        e.np_func(np.zeros(1000, dtype=np.float32))
    b = EnvelopBank((256, 1024), (64, 256), normalize=False)
    assert names(b) == ["n_fft", "hop_length", "normalize"] and EnvelopBank().n_fft == (2048,)
    assert b.envelops == (Envelop(256, 64, False, "hann", True), Envelop(1024, 256, False, "hann", True))
    assert b.unit == Sample(None) and b.elem_type == Continuous(0., float("inf"), 2) and b.inv == Identity()
    i = Interpolate()
    assert (i.axis, i.mode, i.length, i.factor, i.metadata_key) == (-1, "linear", None, None, "n_samples")
    assert i.unit is None and i.elem_type == Continuous(-float("inf"), float("inf"), 1) and i.inv == Identity()
    assert Interpolate(factor=3)._get_target_length(np.zeros((2, 5))) == 15 and Interpolate(length=7, factor=3)._get_target_length(np.zeros(5)) == 7
    with pytest.raises(ValueError, match="No target length provided"):
        Interpolate()._get_target_length(torch.zeros(5))
    meta = np.zeros(5, dtype=np.dtype(np.float32, metadata={"n_samples": 11}))
    assert Interpolate()._get_target_length(meta) == 11
    d = Derivative()
    assert (d.max_lag, d.normalize) == (3, False) and d.unit is None and d.inv == Identity()
    assert d.elem_type == Continuous(-float("inf"), float("inf"), 1)
    chain = mmk.Compose(MagSpec(256, 64), Derivative(2))
    assert chain.unit == Frame(256, 64, padding=True) and chain.elem_type == d.elem_type
    assert mmk.Compose(mmk.FileToSignal(16000), Envelop(256, 64)).unit == Sample(None)
    for name in ("Envelop", "EnvelopBank", "Interpolate", "Derivative"):
        assert name in mmk.features.functionals.__all__


def test_refusals_without_a_gpu():
    x = torch.zeros(3, 16)
    with pytest.raises(NotImplementedError, match="cubic"):
        Interpolate(mode="cubic", length=4)(x)
    with pytest.raises(NotImplementedError, match="axis=0"):
        Interpolate(axis=0, length=4)(x)
    with pytest.raises(NotImplementedError, match=str(native.DERIV_MAX_LAG)):
        native.derivative(torch.zeros(200), native.DERIV_MAX_LAG + 1)
    with pytest.raises(ValueError, match="max_lag"):
        native.derivative(torch.zeros(5), 0)
    with pytest.raises(RuntimeError, match="HIP device|MI355X"):
        Derivative(3)(x)
    with pytest.raises(RuntimeError, match="HIP device|MI355X"):
        Interpolate(length=4)(x)
    with pytest.raises(RuntimeError, match="HIP device|MI355X"):
        Envelop(64, 16)(torch.zeros(100))
    with pytest.raises(TypeError, match="float32"):
        native.interp1d(x.double(), 4)
    with pytest.raises(ValueError, match="previous"):
        native.interp1d(x, 4, "previous", align=False)
    lib = native.load_library()
    # (pointer arguments are never dereferenced by the checks: every call below returns before a launch)
    assert lib.mmk_derivative_f32(16, 8, 1, 8, native.DERIV_MAX_LAG + 1, 1024, 8, None) == -3 and b"derivative" in lib.mmk_last_error()
    assert lib.mmk_derivative_f32(16, 8, 1, 3, 3, 1024, 8, None) == -1            # n <= max_lag
    assert lib.mmk_derivative_f32(16, 8, 1, 8, 0, 1024, 8, None) == -1
    assert lib.mmk_derivative_f32(None, 8, 1, 8, 3, 1024, 8, None) == -1
    assert lib.mmk_derivative_f32(16, 8, 2, 9, 3, 1024, 8, None) == -1            # rows of y overlap
    assert lib.mmk_derivative_f32(16, 8, 1, 8, 3, 1026, 8, None) == -1            # y not 4-byte aligned
    assert lib.mmk_interp1d_f32(16, 8, 1, 1, 1024, 8, 4, 0, 1, None) == -1 and b"interp1d" in lib.mmk_last_error()      # n < 2
    assert lib.mmk_interp1d_f32(16, 8, 1, 8, 1024, 8, 0, 0, 1, None) == -1        # n_out < 1
    assert lib.mmk_interp1d_f32(16, 8, 1, 8, 1024, 8, 4, 2, 1, None) == -1        # mode
    assert lib.mmk_interp1d_f32(16, 8, 1, 8, 1024, 8, 4, 1, 0, None) == -1        # previous with align 0
    assert lib.mmk_interp1d_f32(16, 8, 2, 8, 1024, 3, 4, 0, 1, None) == -1        # rows of y overlap
    assert lib.mmk_stft_energy_f32(16, 100, 1, 100, 96, 24, 1, 1, 1024, None) == -3 and b"stft_energy" in lib.mmk_last_error()
    assert lib.mmk_stft_energy_f32(16, 100, 1, 100, 8192, 24, 1, 1, 1024, None) == -3
    assert lib.mmk_stft_energy_f32(16, 100, 1, 32, 64, 16, 1, 1, 1024, None) == -1      # reflect needs more than n_fft / 2 samples
    assert lib.mmk_stft_energy_f32(16, 100, 1, 63, 64, 16, 0, 0, 1024, None) == -1      # shorter than a frame
    assert lib.mmk_stft_energy_f32(16, 100, 1, 100, 64, 64, 1, 1, 1024, None) == -1     # hop
    assert lib.mmk_stft_energy_f32(None, 100, 1, 100, 64, 16, 1, 1, 1024, None) == -1
