"""The envelope kernels on the MI355X (csrc/envelope.hip and the frame-energy epilogue of the STFT kernels) against the float64
restatements and derived bounds of tests/envelope_refs.py: the three entry points through the C ABI on strided, misaligned rows with
NaN-filled outputs, and Envelop / EnvelopBank / Interpolate / Derivative on device tensors against the reference's results of
tests/golden/envelope.npz.  Each test prints its worst error / bound."""
import os

import numpy as np
import pytest
import torch

from mimikit_amd import native
from mimikit_amd.features.functionals import Derivative, Envelop, EnvelopBank, Interpolate, MagSpec
from tests import envelope_refs as R
from tests.f64_bounds import check_written
from tests.strided_inputs import FLOAT_SURROUNDS, PAD, Strided, surround_rule

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

G = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "envelope.npz"))
OFFSETS = ((1, 3), (3, 0))                # element offsets of the first row of x and of y in their buffers


def same_bits(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


# ------------------------------------------------------------------------------------------------------------------------ energy
@surround_rule(*FLOAT_SURROUNDS)
def energy_call(x_np, n_fft, hop, center, reflect, x_off, device, pad=PAD):
    batch, n = x_np.shape
    frames = R.n_frames(n, n_fft, hop, center)
    x = Strided.of(x_np, x_off, device, row_stride=n + pad)
    out = torch.full((batch * frames + 9,), float("nan"), dtype=torch.float32, device=device)
    native.check(native.lib().mmk_stft_energy_f32(x.ptr, x.stride, batch, n, n_fft, hop, center, reflect, out.data_ptr(), native.stream_ptr(device)))
    mask = torch.zeros(out.shape, dtype=torch.bool)
    mask[:batch * frames] = True
    return out, mask, frames


@pytest.mark.parametrize("n_fft", (64, 256, 1024, 2048, 4096))
def test_stft_energy_against_the_bound(device, n_fft):
    worst = 0.0
    for hop, center, reflect, n in R.energy_cases(n_fft):
        want, bound = R.energy_reference(n_fft, hop, center, reflect, n)
        for batch, x_off in ((1, 0), (3, 1)):
            what = f"n_fft {n_fft}, hop {hop}, center {center}, reflect {reflect}, n {n}, batch {batch}"
            out, mask, frames = energy_call(R.case_input(n)[:batch], n_fft, hop, center, reflect, x_off, device)
            check_written(out, mask, what)
            got = out[:batch * frames].reshape(batch, frames).cpu().numpy()
            worst = max(worst, R.assert_inside(got, want[:batch], bound[:batch], what))
            again, _, _ = energy_call(R.case_input(n)[:batch], n_fft, hop, center, reflect, x_off, device)
            assert same_bits(again, out), f"{what}: two calls differ"
            if batch > 1:                     # rows end to end: a window that leaves a row meets the next row's samples
                assert same_bits(energy_call(R.case_input(n)[:batch], n_fft, hop, center, reflect, x_off, device, pad=0)[0], out), f"{what}: rows end to end"
    print(f"stft_energy n_fft {n_fft}: worst error / bound {worst:.3f}")


def test_stft_energy_is_the_sum_of_the_spectrogram(device):
    """native.stft_energy against the parent's composition, the 'pol' magnitudes summed over the bins in float64"""
    for n_fft, hop in ((256, 64), (1024, 256), (2048, 512)):
        x = torch.from_numpy(R.case_input(20 * hop + 5).copy()).to(device)
        e = native.stft_energy(x, n_fft, hop, True, "reflect")
        s = native.stft(x, n_fft, hop, True, "reflect", "pol")[..., 0].double().sum(-1)
        assert e.shape == s.shape == (3, 21) and e.dtype == torch.float32
        assert float(((e.double() - s).abs() / s).max()) <= (4 + R.C_ENERGY * (n_fft // 2 + 1) ** 0.5) * R.U      # two roundings per magnitude on either side, and the sum


# ----------------------------------------------------------------------------------------------------------------- interpolation
@surround_rule(*FLOAT_SURROUNDS)
def interp_call(x_np, n_out, mode, align, x_off, y_off, device):
    batch, n = x_np.shape
    x, y = Strided.of(x_np, x_off, device), Strided((batch, n_out), y_off, device, float("nan"))
    native.check(native.lib().mmk_interp1d_f32(x.ptr, x.stride, batch, n, y.ptr, y.stride, n_out, native.INTERP_MODES[mode], align,
                                               native.stream_ptr(device)))
    return y


@pytest.mark.parametrize("n,n_out", R.INTERP_SIZES)
def test_interp1d_against_the_bound(device, n, n_out):
    x = R.case_input(n)
    worst = 0.0
    for mode, align in (("linear", 1), ("linear", 0), ("previous", 1)):
        want, bound = R.interp_ref(x.astype(np.float64), n_out, mode, align)
        for batch in (1, 3):
            for x_off, y_off in OFFSETS:
                what = f"{n} -> {n_out}, {mode}, align {align}, batch {batch}, offsets {x_off} / {y_off}"
                y = interp_call(x[:batch], n_out, mode, align, x_off, y_off, device)
                check_written(y.buf, y.mask(), what)
                worst = max(worst, R.assert_inside(y.view.cpu().numpy(), want[:batch], bound[:batch], what))
    print(f"interp1d {n} -> {n_out}: worst error / bound {worst:.3f}")


def test_interp1d_previous_at_exact_knots(device):
    """positions that are integers: 9 knots to 17 points puts every other point on a knot, 9 to 5 every point, and the last point is the
    last knot whatever the rounding of i * step"""
    x = R.case_input(9)
    for n_out, idx in ((17, np.arange(17) // 2), (5, np.arange(5) * 2), (9, np.arange(9))):
        y = interp_call(x, n_out, "previous", 1, 1, 3, device)
        assert np.array_equal(y.view.cpu().numpy(), x[:, idx]), n_out
        lin = interp_call(x, n_out, "linear", 1, 1, 3, device).view.cpu().numpy()
        on_knot = (np.arange(n_out) * 8) % (n_out - 1) == 0
        assert np.array_equal(lin[:, on_knot], x[:, idx][:, on_knot])
    for n, n_out in ((300, 4097), (7, 1000)):
        x = R.case_input(n)
        y = interp_call(x, n_out, "previous", 1, 0, 0, device).view.cpu().numpy()
        assert np.array_equal(y[:, -1], x[:, -1]) and np.array_equal(y[:, 0], x[:, 0])
        assert np.array_equal(y, x[:, np.floor(np.linspace(0, n - 1, n_out)).astype(np.int64)])


# -------------------------------------------------------------------------------------------------------------------- derivative
@surround_rule(*FLOAT_SURROUNDS)
def derivative_call(x_np, L, x_off, y_off, device, pad=PAD):
    batch, n = x_np.shape
    x, y = Strided.of(x_np, x_off, device, row_stride=n + pad), Strided((batch, n), y_off, device, float("nan"))
    native.check(native.lib().mmk_derivative_f32(x.ptr, x.stride, batch, n, L, y.ptr, y.stride, native.stream_ptr(device)))
    return y


@pytest.mark.parametrize("L,n", R.DERIV_CASES)
def test_derivative_against_the_bound(device, L, n):
    x = R.case_input(n, seed=L)
    want, bound = R.derivative_reference(L, n)
    worst = 0.0
    for batch in (1, 3):
        for x_off, y_off in OFFSETS:
            what = f"max_lag {L}, n {n}, batch {batch}, offsets {x_off} / {y_off}"
            y = derivative_call(x[:batch], L, x_off, y_off, device)
            check_written(y.buf, y.mask(), what)
            worst = max(worst, R.assert_inside(y.view.cpu().numpy(), want[:batch], bound[:batch], what))
            if batch > 1:                     # rows end to end: a lag that leaves a row meets the row before it
                packed = derivative_call(x[:batch], L, x_off, y_off, device, pad=0)
                assert same_bits(packed.view.contiguous(), y.view.contiguous()), f"{what}: rows end to end"
    print(f"derivative max_lag {L}, n {n}: worst error / bound {worst:.3f}")


# ------------------------------------------------------------------------------------------------------------------- functionals
def envelop_want(n_fft, x_np, interp, normalize):
    """by parts: the float64 energy restatement of the length-fixed rows, then the steps the fixture pins"""
    T = x_np.shape[-1]
    hop = n_fft // 4
    keep = MagSpec(n_fft, hop, center=True, pad_mode="reflect").stft.fixed_length(T)
    e, bound = R.energy_ref(torch.from_numpy(x_np[..., -keep:].astype(np.float64)), n_fft, hop, 1, 1)
    e, bound = e.numpy(), bound.numpy()
    if interp:
        lo, hi, w_hi, w_lo = R.interp_positions(e.shape[-1], T, 1)
        ib = R.interp_ref(e, T, "linear", 1)[1]
        e, bound = w_lo * e[..., lo] + w_hi * e[..., hi], w_lo * bound[..., lo] + w_hi * bound[..., hi] + ib
    if normalize:
        m = e.max(-1, keepdims=True)
        # the maximum carries its own bound into every quotient; the division rounds once more
        bound = bound / m + e / m * (bound.max(-1, keepdims=True) / m) + 2 * R.U * e / m
        e = e / m
    return e, bound


@pytest.mark.parametrize("interp", (True, False))
@pytest.mark.parametrize("normalize", (True, False))
def test_envelop(device, interp, normalize):
    x = G["env_x"]
    xb = np.stack([x, x[::-1].copy(), 0.25 * x])
    for n_fft in (256, 1024):
        f = Envelop(n_fft, n_fft // 4, normalize=normalize, interp_to_time_domain=interp)
        want, bound = envelop_want(n_fft, xb, interp, normalize)
        got1 = f(torch.from_numpy(x.copy()).to(device))
        gotb = f(torch.from_numpy(xb).to(device))
        assert got1.device.type == "cuda" and got1.dtype == torch.float32 and got1.shape == want.shape[1:] and gotb.shape == want.shape
        R.assert_inside(gotb.cpu().numpy(), want, bound, f"Envelop({n_fft}) on (B, T)")
        R.assert_inside(got1.cpu().numpy(), want[0], bound[0], f"Envelop({n_fft}) on (T,)")
        assert same_bits(got1, gotb[0])
        # ... and the reference's own steps after the transform (the fixture)
        key = f"env_{n_fft}_" + ("interp" if interp else "sum") + ("_normalized" if normalize else "")
        R.assert_inside(got1.cpu().numpy(), G[key].astype(np.float64), bound[0] + R.U * np.abs(G[key]), f"Envelop({n_fft}) against the reference's steps")


def test_envelop_of_a_silent_row_and_the_bank(device):
    x = torch.from_numpy(np.stack([G["env_x"], np.zeros_like(G["env_x"])])).to(device)
    e = Envelop(256, 64)(x)
    assert bool((e[1] == 0).all()) and float(e[0].max()) == 1.0 and float(e[0].min()) >= 0.0
    bank = EnvelopBank((256, 1024), (64, 256))
    got = bank(x[0])
    T = x.shape[-1]
    assert got.shape == (2 * T,)
    assert same_bits(got[:T], Envelop(256, 64)(x[0])) and same_bits(got[T:], Envelop(1024, 256)(x[0]))
    assert bank(x).shape == (2, 2 * T)


def test_derivative_functional(device):
    x = G["deriv_x"]
    xd = torch.from_numpy(x.copy()).to(device)
    for lag in (1, 3, 9, 33):
        want, bound = R.derivative_ref(x.astype(np.float64), lag), R.derivative_bound(x.astype(np.float64), lag)
        got = Derivative(lag)(xd)
        R.assert_inside(got.cpu().numpy(), want, bound, f"Derivative({lag})")
        assert same_bits(Derivative(lag)(xd[0]), got[0]) and same_bits(Derivative(lag)(xd.reshape(3, 1, -1)), got.reshape(3, 1, -1))
        # the kernel makes the reference's roundings in the reference's order
        assert np.array_equal(got.cpu().numpy(), G[f"deriv_torch_2d_{lag}"]), lag
    got = Derivative(3, normalize=True)(xd).cpu().numpy()
    want = G["deriv_np_normalized_3"].astype(np.float64)
    R.assert_inside(got, want, 4 * R.U * np.abs(want), "Derivative(3, normalize=True)")
    assert bool((Derivative(3, normalize=True)(torch.zeros(2, 50, device=device)) == 0).all())
    with pytest.raises(NotImplementedError):
        Derivative(native.DERIV_MAX_LAG + 1)(xd)
    with pytest.raises(ValueError):
        Derivative(9)(xd[:, :9])


def test_interpolate_functional(device):
    x = G["interp_x"]
    xd = torch.from_numpy(x.copy()).to(device)
    x64 = x.astype(np.float64)
    for key, kw in {"length100": dict(length=100), "length13": dict(length=13), "length37": dict(length=37), "factor3": dict(factor=3)}.items():
        n_out = kw.get("length", 3 * x.shape[-1])
        want, bound = R.interp_ref(x64, n_out, "linear", 0)
        got = Interpolate(**kw)(xd)
        assert got.shape == (3, n_out) and got.device.type == "cuda"
        R.assert_inside(got.cpu().numpy(), want, bound, f"Interpolate({kw})")
        R.assert_inside(got.cpu().numpy(), G[f"interp_torch_2d_{key}"].astype(np.float64), 2 * bound, f"Interpolate({kw}) against the reference")
        assert same_bits(Interpolate(**kw)(xd[0]), got[0])
        prev = Interpolate(mode="previous", **kw)(xd)
        assert np.array_equal(prev.cpu().numpy(), G[f"interp_np_previous_{key}"])
    assert Interpolate(length=1)(xd[:1]).shape == ()            # the reference's .squeeze()
    with pytest.raises(ValueError, match="No target length provided"):
        Interpolate()(xd)
    with pytest.raises(NotImplementedError, match="nearest"):
        Interpolate(mode="nearest", length=4)(xd)
    with pytest.raises(NotImplementedError, match="axis=0"):
        Interpolate(axis=0, length=4)(xd)
    with pytest.raises(ValueError):
        Interpolate(length=4)(xd[:, :1])
