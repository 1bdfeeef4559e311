"""The float64 references and bounds of tests/filter_refs.py held to scipy and to the plain fp32 recurrence, the defects the bound must
catch, and the numpy path / protocol of Emphasis, Deemphasis, RemoveDC and Normalize.  No GPU."""
import math

import numpy as np
import pytest
import torch
from scipy.signal import lfilter

import mimikit_amd as mmk
from mimikit_amd import native
from tests import filter_refs as R

MULTI_CHUNK = tuple(n for n in R.LENGTHS if n > R.CHUNK)


def _col(a):
    return a[:, None]


def test_reference_is_scipy_and_a_plain_loop():
    x = R.case_input(R.RUN + 1).astype(np.float64)
    for name, (b0, b1, a1) in R.FILTERS.items():
        want = lfilter([b0, b1], [1.0, a1], x, axis=-1)
        got = R.lfilter1_ref(x, b0, b1, a1)
        assert np.abs(got - want).max() <= 1e-14 * np.abs(want).max(), name
        for row in range(x.shape[0]):
            y_prev, x_prev = 0.0, 0.0
            for i in range(x.shape[1]):
                y_prev = b0 * x[row, i] + b1 * x_prev - a1 * y_prev
                x_prev = x[row, i]
                assert got[row, i] == pytest.approx(y_prev, rel=1e-14, abs=1e-300), (name, row, i)
    # coefficient arrays along a leading axis give the same rows as one filter at a time
    names, b0, b1, a1 = R.filter_arrays()
    allf = R.lfilter1_ref(x, _col(b0), _col(b1), _col(a1))
    for k, name in enumerate(names):
        assert np.array_equal(allf[k], R.lfilter1_ref(x, *R.FILTERS[name])), name
    S, S2 = R.lfilter1_sums(x, 1.0, 0.3, 0.9)
    g = np.abs(x) + 0.3 * np.abs(np.concatenate([np.zeros((3, 1)), x[:, :-1]], -1))
    assert np.allclose(S, lfilter([1.0], [1.0, -0.9], g), rtol=1e-13) and np.allclose(S2, lfilter([1.0], [1.0, -0.9], S), rtol=1e-13)


def _fp32_ratio(n, positive=False):
    """worst err / (u S2) per filter of the sequential fp32 recurrence over case_input(n), and its worst err / bound"""
    names, want, bound = R.case_reference(n, positive)
    _, b0, b1, a1 = R.filter_arrays(names)
    x = R.case_input(n, positive)
    got = R.lfilter1_ref(x, _col(b0.astype(np.float32)), _col(b1.astype(np.float32)), _col(a1.astype(np.float32)))
    assert got.dtype == np.float32
    err = np.abs(got.astype(np.float64) - want)
    _, S2 = R.lfilter1_sums(x.astype(np.float64), _col(b0), _col(b1), _col(a1))
    with np.errstate(invalid="ignore", divide="ignore"):
        ratio = np.where(S2 > 0, err / (R.U * S2), 0.0)
    assert not R.outside(got, want, bound).any(), f"the fp32 recurrence leaves the bound at length {n}"
    return ratio.reshape(len(names), -1).max(-1)


def test_sequential_fp32_recurrence_stays_inside_the_bound_and_sets_c_iir():
    worst = max([_fp32_ratio(n).max() for n in R.LENGTHS] + [_fp32_ratio(R.POSITIVE_CASE[1], True).max()])
    print(f"worst err / (u S2) of the fp32 recurrence: {worst:.3f}")
    assert R.C_IIR == math.ceil(2 * worst), (R.C_IIR, worst)


@pytest.mark.parametrize("n", MULTI_CHUNK)
def test_bound_catches_the_defects_of_a_chunked_scan(n):
    """a dropped carry-in, a missing b1 x[n-1] on a chunk's first sample and a carry applied as p^i leave the bound on every case they
    apply to (a carry exists where a1 != 0, the b1 term where b1 != 0).  The p^i defect moves the chunk's first sample by (1 - p) carry:
    it leaves the bound for |a1| <= 0.97; at 0.999 it is 1e-3 of a carry against 5 u S2 with S2 ~ 1e6 g, and stays inside - the same
    estimate as for any error of relative size 1 - |p|, which a filter this close to an integrator cannot tell from its own roundings."""
    names, want, bound = R.case_reference(n)
    _, b0, b1, a1 = R.filter_arrays(names)
    x64 = R.case_input(n).astype(np.float64)
    caught = {d: R.outside(R.lfilter1_ref(x64, _col(b0), _col(b1), _col(a1), defect=d, at=R.CHUNK), want, bound).reshape(len(names), 3, -1).any(-1)
              for d in ("carry", "b1", "power")}
    for k, name in enumerate(names):
        assert caught["carry"][k].all() == (a1[k] != 0), name
        assert caught["b1"][k].all() == (b1[k] != 0), name
        if a1[k] != 0 and abs(a1[k]) <= 0.971:
            assert caught["power"][k].all(), name
        if a1[k] == 0:
            assert not caught["power"][k].any(), name
    # the input of positive samples: every carry is large
    names, want, bound = R.case_reference(n, True) if n == R.POSITIVE_CASE[1] else (None, None, None)
    if names:
        xp = R.case_input(n, True).astype(np.float64)
        for d in ("carry", "power"):
            assert R.outside(R.lfilter1_ref(xp, *R.FILTERS[names[0]], defect=d, at=2 * R.CHUNK), want[0], bound[0]).any(-1).all(), d


@pytest.mark.parametrize("p", [math.inf, 1, 2])
def test_normalize_reference_and_its_defect(p):
    n = 3 * R.CHUNK + 17
    x64 = R.case_input(n).astype(np.float64)
    want = R.normalize_ref(x64, p)
    assert np.allclose(want, torch.nn.functional.normalize(torch.from_numpy(x64), p=p, dim=-1).numpy(), rtol=1e-14, atol=0)
    assert np.array_equal(R.normalize_ref(np.zeros((2, 5)), p), np.zeros((2, 5)))
    bound = R.normalize_bound(want, p, n)
    for row in range(3):
        j = int(np.abs(x64[row]).argmax()) // R.CHUNK if p == math.inf else 1        # (the maximum sits in one chunk only)
        assert R.outside(R.normalize_ref(x64[row], p, skip_chunk=j), want[row], bound[row]).any(), (p, row)
    if p == math.inf:      # one exact maximum and one division: torch's own fp32 result is inside (its sums take another order than the kernel's)
        got = torch.nn.functional.normalize(torch.from_numpy(R.case_input(n).copy()), p=p, dim=-1).numpy()
        assert not R.outside(got, want, bound).any()


# ----------------------------------------------------------------------------------------------------------- the functionals
@pytest.mark.parametrize("e", R.EMPHASES)
def test_numpy_path_against_scipy(e):
    x = R.case_input(R.CHUNK + 1)
    em, de = mmk.Emphasis(e), mmk.Deemphasis(e)
    assert np.array_equal(em(x), lfilter([1, -e], [1], x).astype(np.float32)) and em(x).dtype == np.float32
    assert np.array_equal(de(x), lfilter([1 - e], [1, -e], x).astype(np.float32)) and de(x).dtype == np.float32
    # the pair leaves the gain 1 - e behind, as the reference's
    x64 = x.astype(np.float64)
    assert np.allclose(de(em(x64)), (1 - e) * x64, rtol=0, atol=1e-12)
    # the float64 reference with the decimal coefficients is the numpy path
    assert np.allclose(R.lfilter1_ref(x64, 1.0, -e, 0.0), em(x64), rtol=0, atol=1e-13)
    assert np.allclose(R.lfilter1_ref(x64, 1 - e, 0.0, -e), de(x64), rtol=0, atol=1e-13)


def test_protocol_of_the_new_functionals():
    em, de = mmk.Emphasis(0.9), mmk.Deemphasis(0.9)
    assert em.inv == de and de.inv == em and mmk.Emphasis().emphasis == 0. and mmk.Deemphasis().emphasis == 0.
    for f in (em, de):
        assert f.unit is None and f.elem_type is None
    tr = mmk.Compose(em, mmk.MuLawCompress(256))
    assert tr.inv == mmk.Compose(mmk.MuLawExpand(256), de)
    assert tr.elem_type == mmk.Discrete(256) and tr.inv.elem_type == mmk.Continuous(-1., 1., 1)
    back = mmk.Config.deserialize(tr.serialize())
    assert back == tr and isinstance(back.functionals[0], mmk.Emphasis) and back.functionals[0].emphasis == 0.9
    assert "type: Emphasis" in tr.serialize() and "type: Deemphasis" in tr.inv.serialize()
    assert mmk.Config.deserialize(tr.inv.serialize()) == tr.inv
    ex = mmk.Config.deserialize("type: Compose\nfunctionals:\n- type: Normalize\n  p: .inf\n  dim: -1\n- type: RemoveDC\n- type: Deemphasis\n  emphasis: 0.97\n")
    assert ex == mmk.Compose(mmk.Normalize(), mmk.RemoveDC(), mmk.Deemphasis(0.97))
    # an IOSpec whose transform pre-emphasises: the target's inverse is what the loop's tail applies
    spec = R.emphasis_io(0.9)
    assert spec.targets[0].inv == tr.inv and spec.inputs[0].elem_type == mmk.Discrete(256) and spec.targets[0].elem_type == mmk.Discrete(256)


def test_argument_errors_come_before_the_device_is_asked_for():
    x64, xi = torch.zeros(2, 8, dtype=torch.float64), torch.zeros(2, 8, dtype=torch.int64)
    for f in (mmk.Emphasis(0.5), mmk.Deemphasis(0.5), mmk.RemoveDC(), mmk.Normalize()):
        for bad in (x64, xi, torch.zeros(8, dtype=torch.float16)):
            with pytest.raises(TypeError, match="float32"):
                f(bad)
        with pytest.raises(RuntimeError, match="HIP device|MI355X"):      # float32 on the host: no CPU path
            f(torch.zeros(2, 8))
    x = torch.zeros(2, 8)
    with pytest.raises(NotImplementedError, match="p=3"):
        mmk.Normalize(p=3)(x)
    with pytest.raises(NotImplementedError, match="dim=0"):
        mmk.Normalize(dim=0)(x)
    with pytest.raises(NotImplementedError, match="p=0.5"):
        native.row_normalize(x, 0.5)
    with pytest.raises(TypeError):
        native.lfilter1(x64, 1.0, 0.0, 0.5)
    assert mmk.Normalize(dim=1).dim == 1      # (the last dimension of a (B, T) tensor by its index: refused only on the host here)
    with pytest.raises(RuntimeError, match="HIP device|MI355X"):
        mmk.Normalize(dim=1)(x)


def test_entry_points_validate_without_a_gpu():
    lib = native.load_library()
    header = open(native.os.path.join(native.os.path.dirname(native._HERE), "include", "mmk.h")).read()
    for name, value in (("RUN", native.LFILTER1_RUN), ("WG", native.LFILTER1_WG), ("CHUNK", native.LFILTER1_CHUNK)):
        assert f"#define MMK_LFILTER1_{name} {value}" in header
    assert native.LFILTER1_CHUNK == native.LFILTER1_RUN * native.LFILTER1_WG
    assert lib.mmk_lfilter1_workspace_floats(3, 3 * R.CHUNK + 17) == 12 == lib.mmk_row_normalize_workspace_floats(3, 3 * R.CHUNK + 17)
    assert lib.mmk_lfilter1_workspace_floats(1, R.CHUNK) == 1 and lib.mmk_lfilter1_workspace_floats(0, 5) == 0
    assert lib.mmk_lfilter1_f32(None, 8, 1, 8, 1.0, 0.0, 0.5, None, 8, None, None) == -1 and b"lfilter1" in lib.mmk_last_error()
    assert lib.mmk_lfilter1_f32(16, 8, 2, 9, 1.0, 0.0, 0.5, 32, 8, None, None) == -1         # rows of y overlap
    assert lib.mmk_lfilter1_f32(16, 8, 1, 8, 1.0, 0.0, 0.5, 34, 8, None, None) == -1         # y not 4-byte aligned
    assert lib.mmk_lfilter1_f32(16, 8, 1, 8, 1.0, 0.0, -1.5, 32, 8, None, None) == -3 and b"a1" in lib.mmk_last_error()
    assert lib.mmk_lfilter1_f32(16, 2 * R.CHUNK, 1, 2 * R.CHUNK, 1.0, 0.0, 0.5, 1 << 20, 2 * R.CHUNK, None, None) == -4      # two chunks need the workspace
    assert lib.mmk_row_normalize_f32(16, 8, 1, 8, 3, 1e-12, 64, 8, 128, None) == -3 and b"p must be" in lib.mmk_last_error()
    assert lib.mmk_row_normalize_f32(16, 8, 1, 8, 2, 1e-12, 64, 8, None, None) == -4
