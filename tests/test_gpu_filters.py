"""The first-order filter section and the row normalisation on the MI355X (csrc/filters.hip) against the float64 references and derived
bounds of tests/filter_refs.py: the entry points on strided, misaligned rows with lengths on every boundary of the kernel's tiling, the
four functionals on device tensors, and a pre-emphasised mu-law network through GenerateLoopV2 to a de-emphasised waveform."""
import math

import numpy as np
import pytest
import torch

import mimikit_amd as mmk
from mimikit_amd import native
from mimikit_amd.features.functionals import mulaw_table
from oracle.weights import load_recipe
from tests import filter_refs as R
from tests import helpers as H
from tests.f64_bounds import check_written
from tests.strided_inputs import FLOAT_SURROUNDS, Strided, surround_rule

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

OFFSETS = ((1, 3), (3, 0))                # element offsets of the first row of x and of y in their buffers


@surround_rule(*FLOAT_SURROUNDS)
def lfilter1_rows(x_np, coeffs, x_off, y_off, device):
    batch, n = x_np.shape
    x, y = Strided.of(x_np, x_off, device), Strided((batch, n), y_off, device, float("nan"))
    work = torch.empty((max(1, native.lib().mmk_lfilter1_workspace_floats(batch, n)),), dtype=torch.float32, device=device)
    native.check(native.lib().mmk_lfilter1_f32(x.ptr, x.stride, batch, n, *coeffs, y.ptr, y.stride, work.data_ptr(), native.stream_ptr(device)))
    return y


@surround_rule(*FLOAT_SURROUNDS)
def normalize_rows(x_np, p, x_off, y_off, device):
    batch, n = x_np.shape
    x, y = Strided.of(x_np, x_off, device), Strided((batch, n), y_off, device, float("nan"))
    work = torch.empty((native.lib().mmk_row_normalize_workspace_floats(batch, n),), dtype=torch.float32, device=device)
    native.check(native.lib().mmk_row_normalize_f32(x.ptr, x.stride, batch, n, native.NORM_ORDERS[p], R.EPS, y.ptr, y.stride, work.data_ptr(),
                                                    native.stream_ptr(device)))
    return y


def assert_inside(got, want, bound, what):
    bad = R.outside(got, want, bound)
    if bad.any():
        i = tuple(int(a[0]) for a in np.nonzero(bad))
        err = abs(float(got[i]) - want[i])
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.size} elements outside the derived bound; at {i}: got {float(got[i]):.9g}, "
                             f"want {want[i]:.9g}, error {err:.3e} > bound {bound[i]:.3e}")
    return float(np.max(np.abs(got.astype(np.float64) - want) / np.maximum(bound, 1e-300)))


def test_constants_are_the_header_s():
    assert (R.CHUNK, R.RUN, R.WG) == (4096, 16, 256)


@pytest.mark.parametrize("n", R.LENGTHS)
def test_lfilter1_against_the_bound(device, n):
    names, want, bound = R.case_reference(n)
    x = R.case_input(n)
    worst = 0.0
    for k, name in enumerate(names):
        for batch in R.BATCHES:
            for x_off, y_off in OFFSETS:
                what = f"{name}, batch {batch}, n {n}, offsets {x_off} / {y_off}"
                y = lfilter1_rows(x[:batch], R.FILTERS[name], x_off, y_off, device)
                check_written(y.buf, y.mask(), what)
                got = y.view.cpu().numpy()
                worst = max(worst, assert_inside(got, want[k, :batch], bound[k, :batch], what))
                again = lfilter1_rows(x[:batch], R.FILTERS[name], x_off, y_off, device)
                assert torch.equal(again.view.view(torch.int32), y.view.view(torch.int32)), f"{what}: two calls differ"
    print(f"n = {n}: worst error / bound {worst:.3f}")


def test_lfilter1_on_positive_input(device):
    """uniform(0, 1): nothing cancels, every chunk's carry-in is large"""
    name, n = R.POSITIVE_CASE
    _, want, bound = R.case_reference(n, True)
    x = R.case_input(n, True)
    for x_off, y_off in OFFSETS:
        y = lfilter1_rows(x, R.FILTERS[name], x_off, y_off, device)
        check_written(y.buf, y.mask(), name)
        print(f"positive input: worst error / bound {assert_inside(y.view.cpu().numpy(), want[0], bound[0], name):.3f}")


@pytest.mark.parametrize("p", [math.inf, 1, 2])
def test_row_normalize_against_the_bound(device, p):
    for n in R.LENGTHS:
        x = R.case_input(n)
        want = R.normalize_ref(x.astype(np.float64), p)
        bound = R.normalize_bound(want, p, n)
        for batch in R.BATCHES:
            for x_off, y_off in OFFSETS:
                what = f"p {p}, batch {batch}, n {n}, offsets {x_off} / {y_off}"
                y = normalize_rows(x[:batch], p, x_off, y_off, device)
                check_written(y.buf, y.mask(), what)
                assert_inside(y.view.cpu().numpy(), want[:batch], bound[:batch], what)
                again = normalize_rows(x[:batch], p, x_off, y_off, device)
                assert torch.equal(again.view.view(torch.int32), y.view.view(torch.int32)), f"{what}: two calls differ"
    # an all-zero row: 0 / eps
    z = R.case_input(R.CHUNK + 1).copy()
    z[1] = 0
    y = normalize_rows(z, p, 1, 3, device).view.cpu().numpy()
    assert np.array_equal(y[1], np.zeros(R.CHUNK + 1, dtype=np.float32)) and np.isfinite(y).all()


def test_functionals_on_device_tensors(device):
    n = 3 * R.CHUNK + 17
    x = R.case_input(n)
    x64 = x.astype(np.float64)
    xd = torch.from_numpy(x.copy()).to(device)
    for f, co in ((mmk.Emphasis(0.97), R.emphasis_coeffs(0.97)), (mmk.Deemphasis(0.97), R.deemphasis_coeffs(0.97)),
                  (mmk.Deemphasis(0.999), R.deemphasis_coeffs(0.999)), (mmk.RemoveDC(), R.REMOVE_DC)):
        want, bound = R.lfilter1_ref(x64, *co), R.lfilter1_bound(x64, *co)
        got = f(xd)
        assert got.shape == xd.shape and got.dtype == torch.float32 and got.device == xd.device
        assert_inside(got.cpu().numpy(), want, bound, repr(f))
        # one row, and rows under two leading dimensions: flattened over the last dimension and restored
        assert torch.equal(f(xd[1]), got[1]) and f(xd[1]).shape == (n,)
        x3 = xd[:, :2 * (n // 2)].reshape(3, 2, n // 2)
        got3 = f(x3)
        assert got3.shape == x3.shape
        assert_inside(got3.cpu().numpy().reshape(6, -1), R.lfilter1_ref(x64[:, :2 * (n // 2)].reshape(6, -1), *co),
                      R.lfilter1_bound(x64[:, :2 * (n // 2)].reshape(6, -1), *co), repr(f) + " 3-D")
    for p in (math.inf, 1, 2):
        want = R.normalize_ref(x64, p)
        assert_inside(mmk.Normalize(p)(xd).cpu().numpy(), want, R.normalize_bound(want, p, n), f"Normalize({p})")
        assert torch.equal(mmk.Normalize(p, dim=1)(xd), mmk.Normalize(p)(xd))
    # the default extractor chain of mulaw_io / magspec_io on a (B, T) device tensor: the second stage takes the first one's fp32 output
    mid = mmk.Normalize()(xd)
    got = mmk.Compose(mmk.Normalize(), mmk.RemoveDC())(xd)
    assert torch.equal(got, mmk.RemoveDC()(mid))
    mid64 = mid.cpu().numpy().astype(np.float64)
    assert_inside(got.cpu().numpy(), R.lfilter1_ref(mid64, *R.REMOVE_DC), R.lfilter1_bound(mid64, *R.REMOVE_DC), "Compose(Normalize, RemoveDC)")
    with pytest.raises(TypeError, match="float32"):
        mmk.Deemphasis(0.5)(xd.double())
    with pytest.raises(NotImplementedError, match="dim=0"):
        mmk.Normalize(dim=0)(xd)


@pytest.mark.parametrize("e", [0.5, 0.97])
def test_deemphasis_of_emphasis_is_the_gain(device, e):
    """Deemphasis(e)(Emphasis(e)(x)) = (1 - e) x.  With the fp32 coefficients both kernels receive, the pole of the second cancels the zero of
    the first exactly and the gain is b0 = fl(1 - e).  The second stage filters the first one's error along with the signal, so the first bound
    goes through the second filter's magnitudes (|b0|, |a1|: a gain of (1 - e) / (1 - e) = 1 on a constant), and the second stage adds its own."""
    n = 3 * R.CHUNK + 17
    x = R.case_input(n)
    x64 = x.astype(np.float64)
    em, de = R.emphasis_coeffs(e), R.deemphasis_coeffs(e)
    mid64 = R.lfilter1_ref(x64, *em)
    carried = R.lfilter1_ref(R.lfilter1_bound(x64, *em), abs(de[0]), 0.0, -abs(de[2]))
    bound = carried + R.lfilter1_bound(mid64, *de)
    got = mmk.Deemphasis(e)(mmk.Emphasis(e)(torch.from_numpy(x.copy()).to(device)))
    assert np.abs(R.lfilter1_ref(mid64, *de) - de[0] * x64).max() < 1e-13
    assert_inside(got.cpu().numpy(), de[0] * x64, bound, f"Deemphasis({e})(Emphasis({e}))")


def _run_loop(net, prompt, n_steps, inversed):
    loop = mmk.GenerateLoopV2(mmk.GenerateLoopV2.Config(display_waveform=False, yield_inversed_outputs=inversed), net, n_steps,
                              [[np.arange(prompt.size(0)), prompt]], logger=None)
    outs = list(loop.run())
    torch.set_grad_enabled(False)
    return outs[0][0]


def _wavenet(io_spec):
    """the network of helpers.wavenet_a on another IOSpec"""
    net = mmk.WaveNet.from_config(mmk.WaveNet.Config(io_spec=io_spec, blocks=(3, 2), dims_dilated=(16,), residuals_dim=16, skips_dim=16))
    load_recipe(net, seed=11, gain=2.0)
    return net.eval()


def test_pre_emphasised_network_through_the_loop(device):
    """targets with transform Compose(Emphasis(0.9), MuLawCompress(256)): the loop's tail expands the generated classes and de-emphasises
    them on the device; the classes themselves do not depend on the Emphasis stage when the prompt is given as classes"""
    e, steps = 0.9, 24
    prompt = H.T(H.golden("wavenet.npz")["a_prompt"])
    net = _wavenet(R.emphasis_io(e))
    assert net.config.io_spec.targets[0].inv == mmk.Compose(mmk.MuLawExpand(256), mmk.Deemphasis(e))
    idx = _run_loop(net, prompt, steps, inversed=False)
    wave = _run_loop(net, prompt, steps, inversed=True)
    assert idx.dtype == torch.int64 and wave.dtype == torch.float32 and wave.shape == idx.shape and wave.is_cuda
    plain = _run_loop(_wavenet(R.emphasis_io(None)), prompt, steps, inversed=False)
    assert torch.equal(idx, plain) and torch.equal(plain.cpu(), H.T(H.golden("wavenet.npz")["a_out"]))
    expanded = mulaw_table(256, 1.0)[idx.cpu()].numpy().astype(np.float64)
    co = R.deemphasis_coeffs(e)
    assert_inside(wave.cpu().numpy(), R.lfilter1_ref(expanded, *co), R.lfilter1_bound(expanded, *co), "the loop's de-emphasised waveform")
