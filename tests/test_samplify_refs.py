"""CPU side of the Samplifyer tests: the restatement of tests/samplify_refs.py against tests/golden/samplify.npz, the spline's bound against
an independent float64 solve and against the near misses that must leave it, the C ABI's declarations (include/mmk_samplify.h against the
ctypes table against the library), the public classes' fields and every refusal that needs no device."""
import ctypes as C
import dataclasses
import os
import re

import numpy as np
import pytest
import scipy.interpolate as SI
import torch

import mimikit_amd as mmk
from mimikit_amd import native
from mimikit_amd.extract import samplify as SM
from mimikit_amd.features.functionals import Interpolate
from tests import samplify_refs as R

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
HEADER = os.path.join(ROOT, "include", "mmk_samplify.h")
G = R.golden()


# ------------------------------------------------------------------------------------------------------------------- the golden file
def test_golden_file_is_small_and_holds_every_fixture():
    assert os.path.getsize(R.GOLDEN_PATH) < 400 * 1024
    assert sorted(G.files) == sorted(f"{n}_{k}" for n in R.FIXTURES for k in R.GOLDEN_KEYS)
    for name in R.FIXTURES:
        n = G[f"{name}_cuts"].shape[0]
        assert all(G[f"{name}_{k}"].shape == (n,) for k in R.GOLDEN_KEYS if k not in ("y", "sensitivity"))
        assert G[f"{name}_y"].dtype == np.float32 and G[f"{name}_scores"].dtype == np.float32 and G[f"{name}_cuts"].dtype == np.int64
        assert 4 * int(G[f"{name}_robust"].sum()) >= 3 * n and 4 * int((G[f"{name}_robust"] & G[f"{name}_robust_f32"]).sum()) >= 3 * n
    assert (G["bursts_sides"] == 1).all() and G["bursts_cuts"].shape[0] >= 6 and float(G["bursts_sensitivity"]) == 0.05
    assert (G["dense_sides"] == 0).any() and (G["dense_sides"] == 1).any() and G["dense_cuts"].shape[0] >= 12 and float(G["dense_sensitivity"]) == 0.0


@pytest.mark.parametrize("name", tuple(R.FIXTURES))
def test_restatement_equals_the_golden_file(name):
    r = R.fixture(name)
    assert np.array_equal(r["y"].view(np.int32), G[f"{name}_y"].view(np.int32))
    for key in ("coarse_cuts", "coarse_peaks", "sides", "cuts", "windows", "robust"):
        assert np.array_equal(r[key], G[f"{name}_{key}"]), key
    assert np.array_equal(r["scores"].view(np.int32), G[f"{name}_scores"].view(np.int32))
    assert np.array_equal(r["windows"], np.minimum(r["coarse_peaks"] - r["coarse_cuts"], R.MAX_WINDOW))
    assert (r["scores"] > np.float32(r["sensitivity"])).all() and np.all(np.diff(r["coarse_cuts"]) >= 2)


def test_a_left_side_cut_is_its_coarse_cut_snapped():
    """the reference's dead branch (d = c; c = c - (d - c)): side 0 leaves c where it is with an empty range"""
    r = R.fixture("dense")
    z = R.zero_crossings(r["y"])
    left = np.nonzero(r["sides"] == 0)[0]
    assert left.size >= 1
    for k in left:
        assert r["cuts"][k] == R.snap(int(r["coarse_cuts"][k]), z)
        assert abs(int(r["cuts"][k]) - int(r["coarse_cuts"][k])) <= np.diff(np.nonzero(z)[0]).max()
    right = np.nonzero(r["sides"] == 1)[0]
    assert any(r["cuts"][k] != R.snap(int(r["coarse_cuts"][k]), z) for k in right)


def test_selection_edges_of_the_restatement():
    g = np.array([-1, 1, 1, -1, -1, 0, 1, -1, 1, 1], dtype=np.float32)         # an exact 0 between - and +: no attack at 6
    att, dec = R.attack_decay(g)
    assert att.tolist() == [1, 8] and dec.tolist() == [2, 9]                    # (the last attack has no peak before T - 1: T - 1)
    assert R.attack_decay(np.array([1, 2, 3], dtype=np.float32))[0].size == 0
    z = R.zero_crossings(np.array([1, 2, -0.0, 0.0, 3], dtype=np.float32))
    assert z.tolist() == [True, False, True, True, False]
    assert R.snap(4, z) == 3 and R.snap(1, z) == 2 and R.snap(1, R.zero_crossings(np.ones(5, dtype=np.float32))) == 0
    e = np.array([5, 1, 3, 9, 2, 2], dtype=np.float32)
    assert R.refine_step(0, 6, e, np.zeros(6, dtype=np.float32))[:2] == (1, 3)
    assert R.refine_step(2, 2, e, e)[:2] == (2, 2)
    lr = R.left_right(e, np.zeros(6, dtype=np.float32), np.array([0, 3]), np.array([2, 2]))
    assert lr[0].tolist() == [-np.inf, 5.0] and lr[1].tolist() == [3.0, 9.0]


# ------------------------------------------------------------------------------------------------------------------------ the spline
SPLINE_SIZES = ((3, 7), (4, 9), (5, 5), (6, 50), (7, 1), (40, 101), (300, 4097))


def test_knots_and_collocation_rows_are_scipys():
    for n in (3, 4, 5, 6, 7, 12):
        y = np.arange(n, dtype=np.float64) ** 2
        assert np.array_equal(SI.make_interp_spline(np.arange(n), y, k=2).t, R.knots(n))
    A = R.collocation(12)
    assert np.allclose(A[0, :3], (1, 0, 0)) and np.allclose(A[1, :3], (1 / 9, 28 / 45, 4 / 15)) and np.allclose(A[2, 1:4], (1 / 10, 31 / 40, 1 / 8))
    assert np.allclose(A[5, 4:7], (1 / 8, 3 / 4, 1 / 8)) and np.allclose(A[-2, -3:], (4 / 15, 28 / 45, 1 / 9)) and np.allclose(A[-1, -3:], (0, 0, 1))
    assert np.count_nonzero(np.triu(A, 2)) == 0 and np.count_nonzero(np.tril(A, -2)) == 0
    assert np.linalg.norm(np.linalg.inv(A), np.inf) < 4.1


@pytest.mark.parametrize("n,n_out", SPLINE_SIZES)
def test_an_independent_float64_solve_is_inside_the_bound(n, n_out):
    y = np.random.default_rng(n).uniform(-1, 1, (2, n)).astype(np.float32)
    want, bound = R.spline_ref(y, n_out)
    c = np.linalg.solve(R.collocation(n), y.astype(np.float64).T)
    got = SI.BSpline(R.knots(n), c, 2)(R.positions(n, n_out)).T.astype(np.float32)
    assert not ER_outside(got, want, bound).any()
    assert np.abs(got.astype(np.float64) - want).max() > 0 or n_out == 1      # (the rounding to float32 is what the bound is made of)


def ER_outside(got, want, bound):
    return ~(np.abs(np.asarray(got, dtype=np.float64) - want) <= bound)


@pytest.mark.parametrize("which", R.NEAR_MISSES)
def test_near_misses_fall_outside_the_bound(which):
    y = np.random.default_rng(5).uniform(-1, 1, 40).astype(np.float32)
    want, bound = R.spline_ref(y, 101)
    miss = R.near_miss(y, 101, which)
    bad = ER_outside(miss, want, bound)
    assert bad.mean() > 0.25, (which, bad.mean())
    assert np.abs(miss - want).max() > 1e4 * bound.max()


# ------------------------------------------------------------------------------------------------------------------- the public classes
def test_package_exports_fields_and_defaults():
    assert mmk.Samplifyer is SM.Samplifyer and mmk.Periods is SM.Periods and mmk.attack_decay is SM.attack_decay
    build = __import__("mimikit_amd.build", fromlist=["SOURCES"])
    assert "samplify.hip" in build.SOURCES and any(h.endswith("mmk_samplify.h") for h in build.HEADERS) and "spline2.h" in build.HEADERS
    s = mmk.Samplifyer(filter_level=1)
    assert [f.name for f in dataclasses.fields(s) if f.name != "type"] == ["filter_level", "sensitivity", "levels_def"]
    d = mmk.Samplifyer()
    assert (d.filter_level, d.sensitivity, d.levels_def) == (0, 0.0, [{}])
    assert [(lv.n_fft, lv.overlap, lv.grad_max_lag) for lv in d.levels] == list(SM.DEFAULT_LEVELS) and len(d.levels) == 6
    assert [(lv.n_fft, lv.overlap, lv.grad_max_lag) for lv in s.levels] == [(4096, 64, 33), (2048, 32, 17), (1024, 16, 9), (512, 8, 9), (256, 8, 9)]
    assert all(lv.window == "hann" and lv.interp_mode == "quadratic" for lv in s.levels)
    lv = s.levels[0]
    assert lv.hop_length == 64 and lv.env_ex == mmk.Envelop(4096, 64, True, "hann", False) and lv.dx == mmk.Derivative(33, True)
    for bad in (-1, 5):
        with pytest.raises(ValueError, match="filter_level must be between 0 and 4"):
            mmk.Samplifyer(filter_level=bad)
    c = mmk.Samplifyer(sensitivity=0.05, levels_def=[dict(n_fft=n, overlap=o, grad_max_lag=g) for n, o, g in R.LEVELS])
    assert [(lv.n_fft, lv.overlap, lv.grad_max_lag) for lv in c.levels] == list(R.LEVELS)
    assert isinstance(c.inv, mmk.Identity) and c.unit is None and c.elem_type is None
    for name in ("cuts", "coarse_cuts", "coarse_peaks", "scores", "sides", "windows", "mins_rank", "maxs_rank", "coarse_env", "coarse_grad", "fine_envs"):
        assert getattr(c, name) is None, name
    back = mmk.Config.deserialize(c.serialize())
    assert isinstance(back, mmk.Samplifyer) and back.sensitivity == 0.05 and [lv.n_fft for lv in back.levels] == [1024, 512, 256]
    for absent in ("plot_refined_cuts", "sr"):
        assert not hasattr(c, absent)
    assert not hasattr(SM, "samplify")
    p = mmk.Periods()
    assert p.att_i is None and p.dec_i is None and p.T == 0
    assert (native.SPLINE2_TILE, native.SPLINE2_HALO, native.PERIODS_TILE, native.SAMPLIFY_MAX_WINDOW) == (256, 32, 1024, R.MAX_WINDOW)
    assert native.INTERP_MODES == {"linear": 0, "previous": 1}
    for lv in R.LEVELS:          # the frames a level has are the transform's own count
        level = SM._EnvelopAndGrad(*lv)
        for t in (48000, 47999, 5000):
            keep = level.env_ex.fft.stft.fixed_length(t)
            assert keep == R.fixed_length(t, lv[0], lv[0] // lv[1])
            assert level.n_frames(t) == native.load_library().mmk_stft_n_frames(keep, lv[0], lv[0] // lv[1], 1)


def test_refusals_that_need_no_device():
    y = torch.zeros(48000)
    levels = lambda **kw: [dict(dict(n_fft=1024, overlap=16, grad_max_lag=9), **kw)]      # noqa: E731
    with pytest.raises(NotImplementedError, match=r"8192.*filter_level >= 1"):
        mmk.Samplifyer().fit(y)
    with pytest.raises(NotImplementedError, match="n_fft = 32"):
        mmk.Samplifyer(levels_def=levels(n_fft=32, overlap=2)).fit(y)
    with pytest.raises(NotImplementedError, match="n_fft = 1000"):
        mmk.Samplifyer(levels_def=levels(n_fft=1000)).fit(y)
    with pytest.raises(NotImplementedError, match="interp_mode='cubic'.*quadratic"):
        mmk.Samplifyer(levels_def=levels(interp_mode="cubic")).fit(y)
    with pytest.raises(NotImplementedError, match="window='hamming'.*hann"):
        mmk.Samplifyer(levels_def=levels(window="hamming")).fit(y)
    with pytest.raises(ValueError, match="no more than grad_max_lag = 33"):
        mmk.Samplifyer(levels_def=levels(grad_max_lag=33)).fit(y[:2048])          # 33 frames
    with pytest.raises(ValueError, match="at least 3 frames"):
        mmk.Samplifyer(levels_def=levels(n_fft=4096, overlap=2, grad_max_lag=1)).fit(y[:4095])      # 2 frames
    with pytest.raises(NotImplementedError, match=str(native.DERIV_MAX_LAG)):
        mmk.Samplifyer(levels_def=levels(grad_max_lag=native.DERIV_MAX_LAG + 1)).fit(y)
    with pytest.raises(ValueError, match="overlap = 1"):
        mmk.Samplifyer(levels_def=levels(overlap=1)).fit(y)
    with pytest.raises(ValueError, match="reflect padding"):
        mmk.Samplifyer(filter_level=4).fit(y[:256])
    with pytest.raises(NotImplementedError, match="levels"):
        mmk.Samplifyer(levels_def=levels() * 7).fit(y)
    ok = mmk.Samplifyer(filter_level=1)
    for call in (lambda: ok.fit(y), lambda: ok(y), lambda: ok.label(y), lambda: mmk.Periods().fit(y), lambda: mmk.attack_decay(y),
                 lambda: native.spline2_coef(y), lambda: native.spline2_eval(y.double(), 5), lambda: native.periods(y.double(), 9), lambda: native.periods(None, 9, row=y),
                 lambda: Interpolate(mode="quadratic", length=9)(y)):
        with pytest.raises(RuntimeError, match="HIP device|MI355X"):
            call()
    with pytest.raises(TypeError, match="float32"):
        ok.fit(y.double())
    with pytest.raises(ValueError, match=r"\(T,\)"):
        ok.fit(y[None])
    with pytest.raises(TypeError):
        ok.fit(y.numpy())
    with pytest.raises(NotImplementedError, match="device tensors only"):
        ok(y.numpy())
    with pytest.raises(TypeError, match="float64"):
        native.spline2_eval(y, 5)
    with pytest.raises(NotImplementedError, match="cubic"):
        Interpolate(mode="cubic", length=4)(y)


# ------------------------------------------------------------------------------------------------------------------------ the header
def header_prototypes():
    text = re.sub(r"/\*.*?\*/", " ", open(HEADER).read(), flags=re.S)
    return {m.group(2): (m.group(1), m.group(3)) for m in re.finditer(r"\b(int|size_t)\s+(mmk_[a-z0-9_]+)\s*\(([^;{}]*?)\)\s*;", text)}


def test_header_names_signatures_exports_and_macros():
    protos = header_prototypes()
    assert sorted(protos) == sorted(native.SAMPLIFY_SYMBOLS) and len(protos) == 7
    assert not set(native.SAMPLIFY_SYMBOLS) & (set(native.EXPORTED_SYMBOLS) | set(native.KMEANS_SYMBOLS) | set(native.NN_FILTER_SYMBOLS) | set(native.NMF_SYMBOLS))
    kinds = {"int64_t": C.c_int64, "int32_t": C.c_int32, "size_t": C.c_size_t, "float": C.c_float, "double": C.c_double,
             "mmk_stream_t": C.c_void_p, "int": C.c_int32}
    lib = native.load_library()
    for name, (res, args) in protos.items():
        want_res, want_args = native._SAMPLIFY_SIGNATURES[name]
        assert want_res is kinds[res], name
        got = [C.c_void_p if "*" in a else kinds[a.strip().replace("const ", "").split()[0]] for a in args.split(",")]
        assert got == list(want_args), (name, got, want_args)
        fn = getattr(lib, name)
        assert fn.restype is want_res and list(fn.argtypes) == list(want_args), name
    text = open(HEADER).read()
    for macro, value in (("SPLINE2_TILE", native.SPLINE2_TILE), ("SPLINE2_HALO", native.SPLINE2_HALO), ("SPLINE2_EVAL_TILE", native.SPLINE2_EVAL_TILE),
                         ("PERIODS_TILE", native.PERIODS_TILE), ("SAMPLIFY_MAX_LEVELS", native.SAMPLIFY_MAX_LEVELS),
                         ("SAMPLIFY_MAX_WINDOW", native.SAMPLIFY_MAX_WINDOW), ("SAMPLIFY_GROUP", native.SAMPLIFY_GROUP)):
        assert int(re.search(rf"#define MMK_{macro} (\d+)", text).group(1)) == value, macro
    main = open(os.path.join(ROOT, "include", "mmk.h")).read()
    assert int(re.search(r"#define MMK_ABI_VERSION (\d+)", main).group(1)) == native.ABI_VERSION == 6
    assert 0.1716 ** native.SPLINE2_HALO < 1e-23          # the header's claim about what lies beyond the halo


def test_entry_points_refuse_bad_arguments_before_any_launch():
    """(pointer arguments are never dereferenced by the checks: every call below returns before a launch)"""
    lib = native.load_library()
    err = lambda: lib.mmk_last_error().decode()      # noqa: E731
    assert lib.mmk_spline2_coef_f64(16, 8, 1, 2, 1024, 8, None) == -1 and "n >= 3" in err()
    assert lib.mmk_spline2_coef_f64(None, 8, 1, 8, 1024, 8, None) == -1
    assert lib.mmk_spline2_coef_f64(16, 8, 2, 8, 1024, 7, None) == -1            # rows of coef overlap
    assert lib.mmk_spline2_coef_f64(18, 8, 1, 8, 1024, 8, None) == -1            # y not 4-byte aligned
    assert lib.mmk_spline2_coef_f64(16, 8, 1, 8, 1028, 8, None) == -1            # coef not 8-byte aligned
    assert lib.mmk_spline2_coef_f64(16, 8, 65536, 8, 1024, 8, None) == -3
    assert lib.mmk_spline2_eval_f32(1024, 8, 1, 2, 16, 8, 8, None) == -1 and "n >= 3" in err()
    assert lib.mmk_spline2_eval_f32(1024, 8, 1, 8, 16, 8, 0, None) == -1 and "n_out" in err()
    assert lib.mmk_spline2_eval_f32(1028, 8, 1, 8, 16, 8, 8, None) == -1
    assert lib.mmk_spline2_eval_f32(1024, 8, 2, 8, 16, 7, 8, None) == -1         # rows of out overlap
    assert lib.mmk_periods_workspace_bytes(0) == 0 and lib.mmk_periods_workspace_bytes(1) == 16
    assert lib.mmk_periods_workspace_bytes(native.PERIODS_TILE + 1) == 32
    assert lib.mmk_periods_count_i64(1024, 2, None, 100, 2048, 4096, 16, None) == -1 and "n >= 3" in err()
    assert lib.mmk_periods_count_i64(1024, 8, 16, 100, 2048, 4096, 16, None) == -1 and "exactly one" in err()
    assert lib.mmk_periods_count_i64(None, 0, None, 100, 2048, 4096, 16, None) == -1 and "exactly one" in err()
    assert lib.mmk_periods_count_i64(None, 0, 18, 100, 2048, 4096, 16, None) == -1           # row not 4-byte aligned
    assert lib.mmk_periods_count_i64(1024, 8, None, 0, 2048, 4096, 16, None) == -1
    assert lib.mmk_periods_count_i64(1024, 8, None, 5000, 2048, 4096, 16, None) == -4 and "are needed" in err()
    assert lib.mmk_periods_count_i64(1024, 8, None, 100, None, 4096, 16, None) == -1
    assert lib.mmk_periods_fill_i64(1024, 8, None, 100, 4096, 8, 1, 1, 2048, 2048, 2048, None) == -4
    assert lib.mmk_periods_fill_i64(1024, 8, None, 100, 4096, 16, 51, 1, 2048, 2048, 2048, None) == -1 and "two samples apart" in err()
    assert lib.mmk_periods_fill_i64(None, 0, 16, 100, 4096, 16, 1, 1, None, 2048, 2048, None) == -1
    assert lib.mmk_periods_fill_i64(None, 0, 16, 100, 4096, 16, 0, 0, None, None, None, None) == 0
    assert lib.mmk_samplify_scores_f32(1024, 2, 100, 2048, 2048, 1, 0.0, 16, 16, 16, 16, None) == -1
    assert lib.mmk_samplify_scores_f32(1024, 8, 100, 2048, 2048, -1, 0.0, 16, 16, 16, 16, None) == -1
    assert lib.mmk_samplify_scores_f32(1024, 8, 100, None, 2048, 1, 0.0, 16, 16, 16, 16, None) == -1
    assert lib.mmk_samplify_scores_f32(1024, 8, 100, None, None, 0, 0.0, None, None, None, None, None) == 0
    ptrs, knots = (native.vp * 7)(*[1024] * 7), (native.i64 * 7)(*[8] * 7)
    assert lib.mmk_samplify_cuts_i64(16, 100, ptrs, ptrs, knots, 0, 2048, 2048, 1, 2048, None, 2048, None) == -1
    assert lib.mmk_samplify_cuts_i64(16, 100, ptrs, ptrs, knots, 7, 2048, 2048, 1, 2048, None, 2048, None) == -3 and "MMK_SAMPLIFY_MAX_LEVELS" in err()
    assert lib.mmk_samplify_cuts_i64(None, 100, ptrs, ptrs, knots, 2, 2048, 2048, 1, 2048, None, 2048, None) == -1
    knots[1] = 2
    assert lib.mmk_samplify_cuts_i64(16, 100, ptrs, ptrs, knots, 2, 2048, 2048, 1, 2048, None, 2048, None) == -1 and "n >= 3" in err()
    knots[1] = 8
    assert lib.mmk_samplify_cuts_i64(16, 100, ptrs, ptrs, knots, 2, 2048, None, 1, 2048, None, 2048, None) == -1
    assert lib.mmk_samplify_cuts_i64(16, 100, ptrs, ptrs, knots, 2, None, None, 0, None, None, None, None) == 0
