"""CPU side of the NMF kernels' tests: the float64 restatement of tests/nmf_refs.py against the reference's results in
tests/golden/nmf.npz (both starts, equal iteration counts), the spreads that the device tolerance is made of, near misses that must
leave that tolerance, the half-sweep bound against a replay in another order, the public class and the C ABI's declarations."""
import ctypes as C
import os
import re
import warnings

import numpy as np
import pytest
import torch

import mimikit_amd as mmk
from mimikit_amd import native
from mimikit_amd.features import functionals as F
from tests import nmf_refs as R

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
HEADER = os.path.join(ROOT, "include", "mmk_nmf.h")
G = R.golden()
AGREE = 1e-10
SMALL = tuple(n for n in R.NAMES if n not in ("runs", "k64"))


def rel(a, b):
    return np.abs(np.asarray(a, dtype=np.float64) - b).max() / np.abs(b).max()


# ------------------------------------------------------------------------------------------------------------------- the golden file
def test_golden_file_is_small_and_holds_every_fixture():
    assert os.path.getsize(R.GOLDEN_PATH) < 400 * 1024
    keys = ("w", "components", "n_iter", "transform", "seed_spread", "f32_diff", "f32_n_iter")
    assert sorted(G.files) == sorted(f"{n}_{k}" for n in R.NAMES for k in keys)
    for name in R.NAMES:
        f = R.FIXTURES[name]
        assert G[f"{name}_w"].shape == (f["n"], f["k"]) and G[f"{name}_components"].shape == (f["k"], f["d"])
        assert G[f"{name}_transform"].shape == (R.TRANSFORM_ROWS, f["k"])
        assert float(G[f"{name}_seed_spread"]) <= AGREE
    assert int(G["cap_n_iter"]) == 7 and int(G["k1_n_iter"]) == 6 and int(G["loose_n_iter"]) < 30
    assert all(int(G[f"{n}_n_iter"]) < R.FIXTURES[n]["max_iter"] for n in R.NAMES if n not in R.BY_COUNT)


@pytest.mark.parametrize("name", R.NAMES)
def test_restatement_equals_the_reference(name):
    r = R.fixture_case(name)                                   # (asserts the fixture's conditions)
    f = r["f"]
    want_w, want_h = G[f"{name}_w"].astype(np.float64), G[f"{name}_components"]
    tol_w = AGREE + (2.0 ** -24 if name == "runs" else 0.0)    # (the golden W of `runs` is stored as float32)
    assert r["n_iter"] == int(G[f"{name}_n_iter"])
    assert rel(r["w"], want_w) <= tol_w and rel(r["h"], want_h) <= AGREE
    assert rel(r["tw"], G[f"{name}_transform"]) <= AGREE
    if name != "runs":
        other = R.fit64(r["x"], f["k"], f["tol"], f["max_iter"], route="svd")
        assert other["n_iter"] == r["n_iter"] and rel(other["w"], want_w) <= AGREE and rel(other["h"], want_h) <= AGREE
        assert rel(other["start"]["w"], r["start"]["w"]) <= 1e-11 and rel(other["start"]["ht"], r["start"]["ht"]) <= 1e-11
        assert np.array_equal(np.abs(np.sign((other["start"]["vt"] * r["start"]["vt"]).sum(1))), np.ones(f["k"]))


def test_fixtures_cover_what_they_are_for():
    x, y = R.fixture_frames("silent")
    assert int((x.sum(1) == 0).sum()) == 10 and int((x.sum(0) == 0).sum()) == 3
    for name in R.NAMES:
        x, y = R.fixture_frames(name)
        assert x.dtype == np.float32 and y.shape == (R.TRANSFORM_ROWS, x.shape[1]) and x.min() >= 0 and y.min() >= 0
    assert R.FIXTURES["wide"]["n"] < R.FIXTURES["wide"]["d"] and R.FIXTURES["k64"]["k"] == native.NMF_MAX_COMPONENTS
    assert R.FIXTURES["runs"]["n"] > 4 * 256                   # more than one run of rows on the column side (csrc/nmf.hip: kNfMinRun)
    assert any((R.fixture_case(n)["w"] == 0).any() for n in SMALL)


# ------------------------------------------------------------------------------------------------------------------- the tolerance's inputs
@pytest.mark.parametrize("name", R.NAMES)
def test_a_thousand_spreads_stay_below_1e_6(name):
    r = R.fixture_case(name)
    sw, sh, stw = R.spread(name)
    tw, th, tt = R.fit_tolerance(name)
    print(f"NMF {name}: spread of W {sw:.2e}, of H {sh:.2e}, of the transform {stw:.2e}; largest entries {np.abs(r['w']).max():.3g}, "
          f"{np.abs(r['h']).max():.3g}, {np.abs(r['tw']).max():.3g}; tolerances {tw:.2e}, {th:.2e}, {tt:.2e}")
    assert R.SPREAD_FACTOR * sw <= 1e-6 * np.abs(r["w"]).max()
    assert R.SPREAD_FACTOR * sh <= 1e-6 * np.abs(r["h"]).max()
    assert R.SPREAD_FACTOR * stw <= 1e-6 * np.abs(r["tw"]).max()


def leaves(name, w=None, h=None, tw=None, n_iter=None):
    """does a variant leave what the device is held to on this fixture: the iteration count, or a tolerance"""
    r = R.fixture_case(name)
    tol_w, tol_h, tol_t = R.fit_tolerance(name)
    out = n_iter is not None and n_iter != r["n_iter"]
    if w is not None:
        out = out or not (np.abs(w.astype(np.float32).astype(np.float64) - r["w"]) <= tol_w).all()
    if h is not None:
        out = out or not (np.abs(h - r["h"]) <= tol_h).all()
    if tw is not None:
        out = out or not (np.abs(tw.astype(np.float32).astype(np.float64) - r["tw"]) <= tol_t).all()
    return out


def test_the_restatement_itself_stays_inside():
    for name in SMALL:
        r = R.fixture_case(name)
        assert not leaves(name, r["w"], r["h"], r["tw"], r["n_iter"])
        o = R.fit64(r["x"], r["f"]["k"], r["f"]["tol"], r["f"]["max_iter"], route="svd", order="reversed")
        assert not leaves(name, o["w"], o["h"], None, o["n_iter"]), name


@pytest.mark.parametrize("defect", ["eps_machine", "transform_from_sqrt", "ge_for_gt", "jacobi", "violation_unprojected", "fit_then_transform"])
def test_near_misses_leave_the_tolerance(defect):
    seen = []
    for name in SMALL:
        r = R.fixture_case(name)
        f = r["f"]
        kw = dict(k=f["k"], tol=f["tol"], max_iter=f["max_iter"])
        if defect == "eps_machine":
            o = R.fit64(r["x"], eps=np.finfo(np.float64).eps, **kw)
            out = leaves(name, o["w"], o["h"], None, o["n_iter"])
        elif defect == "transform_from_sqrt":
            tw, tn = R.transform64(r["y"], r["h"], f["tol"], f["max_iter"], w0="sqrt")
            out = leaves(name, tw=tw) or tn != r["tn"]
        elif defect == "ge_for_gt":
            # the strict comparison matters at a tie only, and a fixture with a tie is not pinned by sklearn: the defect is shown on the
            # rule itself, with a pair whose two products are equal
            s, u, vt = np.array([2.0, 1.0]), np.array([[0.6, 0.5], [0.8, -0.5], [0.0, 0.5], [0.0, -0.5]]), np.array([[0.6, 0.8], [0.5 ** 0.5, -0.5 ** 0.5]])
            x = np.abs((u * s) @ vt)
            a, b = R.nndsvda(x, s, u, vt), R.nndsvda(x, s, u, vt, ge=True)
            out = a["part"][1] == 0 and b["part"][1] == 1 and not np.allclose(a["w"], b["w"])
        elif defect == "jacobi":
            o = R.fit64(r["x"], jacobi=True, **kw)
            out = leaves(name, o["w"], o["h"], None, o["n_iter"])
        elif defect == "violation_unprojected":
            o = R.fit64(r["x"], project=False, **kw)
            out = leaves(name, o["w"], o["h"], None, o["n_iter"])
        else:
            tw, _ = R.transform64(r["x"], r["h"], f["tol"], f["max_iter"])
            out = leaves(name, w=tw)
        seen.append(out)
    assert any(seen), f"{defect} stays inside the tolerance on every fixture - the tolerance is too loose"
    print(f"NMF near miss {defect}: leaves the tolerance on {sum(seen)} of {len(seen)} fixtures")


# ------------------------------------------------------------------------------------------------------------------- the half-sweep's bound
@pytest.mark.parametrize("name", ["tiny", "odd", "k16"])
def test_half_sweeps_in_another_order_stay_inside_the_bound(name):
    x64, w, ht = R.sweep_inputs(name)
    assert (w == 0).any() or (ht == 0).any() or name == "tiny"
    for side in ("w", "h"):
        a0 = (w if side == "w" else ht).copy()
        xa, b, length = (x64, ht, x64.shape[1]) if side == "w" else (x64.T, w, x64.shape[0])
        want, got = a0.copy(), a0.copy()
        v_want = R.sweep64(xa @ b, b.T @ b, want)
        v_got = R.sweep64(R.product(xa, b, "longdouble"), R.product(b.T, b, "reversed"), got)
        da, dv = R.sweep_bound(xa, b, a0, length)
        assert (np.abs(got - want) <= da).all() and abs(v_got - v_want) <= dv
        assert da.max() <= 1e-9 * np.abs(want).max() and dv <= 1e-9 * v_want            # the bound is tight enough to see a wrong rule:
        jac = a0.copy()
        R.sweep64(xa @ b, b.T @ b, jac, jacobi=True)
        assert not (np.abs(jac - want) <= da).all()


# ------------------------------------------------------------------------------------------------------------------- the public class
def test_package_exports_and_yaml_round_trip():
    assert mmk.NMF is F.NMF and "NMF" in F.__all__
    build = __import__("mimikit_amd.build", fromlist=["SOURCES"])
    assert "nmf.hip" in build.SOURCES and any(h.endswith("mmk_nmf.h") for h in build.HEADERS)
    p = mmk.NMF()
    fields = [f.name for f in __import__("dataclasses").fields(p) if f.name != "type"]
    assert fields == ["n_components", "tol", "max_iter", "random_seed"]
    assert (p.n_components, p.tol, p.max_iter, p.random_seed) == (16, 1e-4, 200, 42)
    assert isinstance(p.inv, mmk.Identity) and p.unit is None and p.elem_type is None and p.components_ is None and p.n_iter_ is None
    q = mmk.NMF(n_components=5, tol=1e-3, max_iter=50, random_seed=7)
    back = mmk.Config.deserialize(q.serialize())
    assert isinstance(back, mmk.NMF) and back == q and "components_" not in q.serialize()
    chain = mmk.Config.deserialize("type: Compose\nfunctionals:\n- type: MagSpec\n- type: NMF\n  n_components: 8\n")
    assert isinstance(chain.functionals[1], mmk.NMF) and chain.functionals[1].n_components == 8
    for absent in ("solver", "beta_loss", "alpha_W", "alpha_H", "shuffle", "init", "reconstruction_err_"):
        assert not hasattr(p, absent), absent
    assert (native.NMF_MAX_D, native.NMF_MAX_COMPONENTS) == (native.PCA_MAX_D, native.PCA_MAX_COMPONENTS)


def test_refusals_that_need_no_device():
    x = torch.zeros(20, 6)
    with pytest.raises(RuntimeError, match="cpu"):
        mmk.NMF(n_components=3)(x)
    with pytest.raises(TypeError, match="float64"):
        mmk.NMF(n_components=3)(x.double())
    with pytest.raises(TypeError):
        mmk.NMF(n_components=3).torch_func(x.numpy())
    with pytest.raises(ValueError, match="n_components = 0"):
        mmk.NMF(n_components=0)(x)
    with pytest.raises(ValueError, match=r"n_components = 7 .*min\(N, D\) = 6"):
        mmk.NMF(n_components=7)(x)
    with pytest.raises(ValueError, match=r"n_components = 4 .*min\(N, D\) = 3"):
        mmk.NMF(n_components=4)(x[:3])
    with pytest.raises(ValueError, match="max_iter = 0"):
        mmk.NMF(n_components=2, max_iter=0)(x)
    with pytest.raises(ValueError, match="tol = -1"):
        mmk.NMF(n_components=2, tol=-1.0)(x)
    with pytest.raises(NotImplementedError, match="device tensors only"):
        mmk.NMF().np_func(np.zeros((20, 6), dtype=np.float32))
    with pytest.raises(NotImplementedError, match=f"D = {native.NMF_MAX_D + 1}.*NMF_MAX_D"):
        mmk.NMF(n_components=2)(torch.zeros(3, native.NMF_MAX_D + 1))
    with pytest.raises(NotImplementedError, match=f"n_components = {native.NMF_MAX_COMPONENTS + 1}.*NMF_MAX_COMPONENTS"):
        mmk.NMF(n_components=native.NMF_MAX_COMPONENTS + 1)(torch.zeros(100, 100))
    with pytest.raises(RuntimeError, match="before NMF.fit"):
        mmk.NMF().transform(x)
    with pytest.raises(RuntimeError, match="MI355X|cpu"):
        native.nmf_start(x, 2)
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        mmk.NMF(max_iter=7)._warn(7, "NMF")
        mmk.NMF(max_iter=7)._warn(6, "NMF")
        mmk.NMF(max_iter=7, tol=0.0)._warn(7, "NMF")
    assert len(caught) == 1 and "maximum number of iterations 7" in str(caught[0].message)


# ------------------------------------------------------------------------------------------------------------------- the header
def header_prototypes():
    text = re.sub(r"/\*.*?\*/", " ", open(HEADER).read(), flags=re.S)
    return {m.group(2): (m.group(1), m.group(3)) for m in re.finditer(r"\b(int|size_t)\s+(mmk_[a-z0-9_]+)\s*\(([^;{}]*?)\)\s*;", text)}


def test_header_names_signatures_exports_and_macros():
    protos = header_prototypes()
    assert sorted(protos) == sorted(native.NMF_SYMBOLS) and len(protos) == 7
    assert not set(native.NMF_SYMBOLS) & (set(native.EXPORTED_SYMBOLS) | set(native.KMEANS_SYMBOLS) | set(native.NN_FILTER_SYMBOLS))
    kinds = {"int64_t": C.c_int64, "int32_t": C.c_int32, "size_t": C.c_size_t, "float": C.c_float, "double": C.c_double,
             "mmk_stream_t": C.c_void_p, "int": C.c_int32}
    lib = native.load_library()
    for name, (res, args) in protos.items():
        want_res, want_args = native._NMF_SIGNATURES[name]
        assert want_res is kinds[res], name
        got = [C.c_void_p if "*" in a else kinds[a.strip().replace("const ", "").split()[0]] for a in args.split(",")]
        assert got == list(want_args), (name, got, want_args)
        fn = getattr(lib, name)
        assert fn.restype is want_res and list(fn.argtypes) == list(want_args), name
    text = open(HEADER).read()
    main = open(os.path.join(ROOT, "include", "mmk.h")).read()
    assert "#define MMK_NMF_MAX_D MMK_PCA_MAX_D" in text and "#define MMK_NMF_MAX_COMPONENTS MMK_PCA_MAX_COMPONENTS" in text
    assert float(re.search(r"#define MMK_NMF_EPS (\S+)", text).group(1)) == native.NMF_EPS == R.EPS_CUT == 1e-6
    assert int(re.search(r"#define MMK_NMF_POLL (\d+)", text).group(1)) == native.NMF_POLL == 8
    assert float(re.search(r"#define MMK_NMF_RANK_MARGIN (\S+)", text).group(1)) == native.NMF_RANK_MARGIN == R.RANK_MARGIN
    assert int(re.search(r"#define MMK_ABI_VERSION (\d+)", main).group(1)) == native.ABI_VERSION == 6
    paragraph = main[main.index("streams.  Every kernel"):main.index("no torch / C++ types")]
    assert "mmk_nmf_start_f64" in paragraph and "mmk_nmf_solve_f64" in paragraph


def test_entry_points_refuse_bad_sizes_before_any_launch():
    lib = native.load_library()
    buf = (C.c_double * 64)()
    p = C.addressof(buf)
    it = C.c_int32(0)
    assert lib.mmk_nmf_start_workspace_bytes(1, 8, 1) == 0 and lib.mmk_nmf_start_workspace_bytes(8, 8, 9) == 0
    assert lib.mmk_nmf_half_workspace_bytes(8, native.NMF_MAX_D + 1, 2) == 0 and lib.mmk_nmf_solve_workspace_bytes(100, 100, 65) == 0
    assert lib.mmk_nmf_half_workspace_bytes(8, 8, 2) > 0 and lib.mmk_nmf_solve_workspace_bytes(8, 8, 2) > lib.mmk_nmf_half_workspace_bytes(8, 8, 2)
    big = 1 << 40
    assert lib.mmk_nmf_w_half_f64(p, 8, 8, 8, 0, p, p, p, p, big, None) == -1 and "n_components = 0" in lib.mmk_last_error().decode()
    assert lib.mmk_nmf_start_f64(p, 8, 8, 8, 9, p, p, p, p, p, p, big, None) == -1 and "min(n, d) = 8" in lib.mmk_last_error().decode()
    assert lib.mmk_nmf_half_workspace_bytes(8, 8, 9) > 0                          # (a sweep of fewer rows than components is a transform)
    assert lib.mmk_nmf_h_half_f64(p, 8, 100, native.NMF_MAX_D + 1, 2, p, p, p, p, big, None) == -3 and "MMK_NMF_MAX_D" in lib.mmk_last_error().decode()
    assert lib.mmk_nmf_h_half_f64(p, 8, 100, 100, 65, p, p, p, p, big, None) == -3 and "MMK_NMF_MAX_COMPONENTS" in lib.mmk_last_error().decode()
    assert lib.mmk_nmf_w_half_f64(None, 8, 8, 8, 2, p, p, p, p, big, None) == -1
    assert lib.mmk_nmf_w_half_f64(p, -1, 8, 8, 2, p, p, p, p, big, None) == -1
    assert lib.mmk_nmf_w_half_f64(p + 2, 8, 8, 8, 2, p, p, p, p, big, None) == -1
    assert lib.mmk_nmf_w_half_f64(p, 8, 8, 8, 2, p + 4, p, p, p, big, None) == -1
    assert lib.mmk_nmf_w_half_f64(p, 8, 8, 8, 2, p, p, p, p, 8, None) == -4 and "are needed" in lib.mmk_last_error().decode()
    assert lib.mmk_nmf_solve_f64(p, 8, 8, 8, 2, p, p, 1, 1e-4, 0, 0, 0, C.byref(it), p, big, None) == -1 and "max_iter = 0" in lib.mmk_last_error().decode()
    assert lib.mmk_nmf_solve_f64(p, 8, 8, 8, 2, p, p, 1, -1.0, 5, 0, 0, C.byref(it), p, big, None) == -1
    assert lib.mmk_nmf_solve_f64(p, 8, 8, 8, 2, p, p, 1, 1e-4, 5, 0, 0, C.byref(it), p, 8, None) == -4
    part = (C.c_int32 * 8)()
    assert lib.mmk_nmf_start_f64(p, 8, 1, 8, 1, p, p, p, p, part, p, big, None) == -1 and "at least 2" in lib.mmk_last_error().decode()
    assert lib.mmk_nmf_start_f64(p, 8, 8, 8, 2, p, p, p, p, part, p, 8, None) == -4
