"""No GPU: the float64 restatement of tests/factor_analysis_refs.py against the recorded results of sklearn's exact method and of the
reference (tests/golden/factor_analysis.npz), the conditions under which the fixtures pin the EM loop, the public class and what it
refuses on the host, and the completeness of include/mmk_factor_analysis.h against native.FACTOR_ANALYSIS_SYMBOLS."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import mimikit_amd as mmk
from mimikit_amd import native
from mimikit_amd.features import functionals as F
from tests import factor_analysis_refs as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "mmk_factor_analysis.h")
G = R.golden()


# ------------------------------------------------------------------------------------------------------------------- the restatement
@pytest.mark.parametrize("name", R.NAMES)
def test_restatement_against_the_exact_method(name):
    r = R.fixture_case(name)
    assert r["n_iter"] == int(G[f"{name}_n_iter"])
    assert r["converged"] == (name != "cap3")
    errs = dict(components=R.rel_err(R.align(r["components"], G[f"{name}_components"]), G[f"{name}_components"]),
                noise_variance=R.rel_err(r["noise_variance"], G[f"{name}_noise_variance"]),
                scores=R.rel_err(R.align(r["scores"], G[f"{name}_scores"], by_rows=False), G[f"{name}_scores"]))
    ll_err = np.abs(r["loglike"] - G[f"{name}_loglike"]).max()
    ll_tol = R.REF_TOL * np.abs(G[f"{name}_loglike"]).max() + r["ll_rounding"]          # (factor_analysis_refs: ll's own rounding)
    print(f"fa64 {name}: n_iter {r['n_iter']}; against sklearn's lapack method " + ", ".join(f"{k} {v:.1e}" for k, v in errs.items())
          + f", loglike {ll_err:.2e} absolute (tolerance {ll_tol:.2e}, of which its own rounding {r['ll_rounding']:.2e})")
    assert max(errs.values()) <= R.REF_TOL, errs
    assert ll_err <= ll_tol
    assert r["ll_rounding"] <= (3.1e-3 if name == "two_rows" else 2e-8)
    a = R.transform_matrix64(r["components"], r["noise_variance"])
    assert R.rel_err((r["x"].astype(np.float64) - r["mean"]) @ a.T, r["scores"]) <= 1e-12


@pytest.mark.parametrize("name", R.NAMES)
def test_restatement_against_the_reference(name):
    """the reference's default (randomised) method takes the same number of EM steps; its deviation r_i from the restatement is the
    recorded one, and small: it is the reference's own approximation error, which the GPU test grants on top of 1e-6"""
    r = R.fixture_case(name)
    assert r["n_iter"] == int(G[f"{name}_ref_n_iter"])
    ref = G[f"{name}_ref_scores"]
    assert ref.shape == r["scores"].shape
    dev = np.abs(R.align(ref, r["scores"], by_rows=False) - r["scores"]).max()
    recorded = float(G[f"{name}_ref_deviation"])
    print(f"fa64 {name}: the reference's scores deviate by {dev / np.abs(r['scores']).max():.2e} of the largest score (recorded {recorded:.3e})")
    assert abs(dev - recorded) <= 1e-9 * np.abs(r["scores"]).max()
    assert recorded <= 1e-5 * np.abs(r["scores"]).max()


@pytest.mark.parametrize("name", R.NAMES)
def test_fixture_conditions(name):
    r = R.fixture_case(name)
    f = r["f"]
    assert r["gaps"].min() >= R.GAP_MIN, (name, r["gaps"].min())
    ll = r["loglike"]
    margin = np.abs(np.diff(ll) - f["tol"]).min() if len(ll) > 1 else np.inf
    print(f"fa64 {name}: smallest relative gap {r['gaps'].min():.2e}, smallest |ll_i - ll_(i-1) - tol| {margin:.2e}, largest |ll| {np.abs(ll).max():.3e}")
    assert margin >= R.STOP_MARGIN and margin >= 2 * r["ll_rounding"] and np.abs(ll).max() <= R.LL_MAX
    if f["const"]:
        assert r["noise_variance"][f["d"] // 2] == R.SMALL, "the constant column does not reach the floor of psi"
    assert (r["components"][np.arange(f["k"]), np.abs(r["components"]).argmax(1)] > 0).all()


def test_fixture_shapes_cover_the_kernels_paths():
    shapes = {(f["n"], f["d"], f["k"]) for f in R.FIXTURES.values()}
    assert any(d % 16 and d > 16 for _, d, _ in shapes) and any(d < k + 16 for _, d, k in shapes) and any(n < d for n, d, _ in shapes)
    assert any(n == 2 for n, _, _ in shapes) and any(d > 128 for _, d, _ in shapes)
    assert R.FIXTURES["cap3"]["max_iter"] == 3 < R.fixture_case("f24")["n_iter"]
    assert os.path.getsize(R.GOLDEN_PATH) < 1 << 20


# ------------------------------------------------------------------------------------------------------------------- the public class
def test_package_exports_and_yaml_round_trip():
    assert mmk.FactorAnalysis is F.FactorAnalysis and "FactorAnalysis" in F.__all__
    build = __import__("mimikit_amd.build", fromlist=["SOURCES"])
    assert "factor_analysis.hip" in build.SOURCES and any(h.endswith("mmk_factor_analysis.h") for h in build.HEADERS)
    assert "subspace_eig.h" in build.HEADERS
    p = mmk.FactorAnalysis()
    fields = [f.name for f in __import__("dataclasses").fields(p) if f.name != "type"]
    assert fields == ["n_components", "tol", "max_iter", "random_seed"]
    assert (p.n_components, p.tol, p.max_iter, p.random_seed) == (16, 1e-2, 1000, 42)
    assert isinstance(p.inv, mmk.Identity) and p.unit is None and p.elem_type is None
    assert all(getattr(p, a) is None for a in ("mean_", "components_", "noise_variance_", "loglike_", "n_iter_"))
    q = mmk.FactorAnalysis(n_components=5, tol=1e-3, max_iter=50, random_seed=7)
    back = mmk.Config.deserialize(q.serialize())
    assert isinstance(back, mmk.FactorAnalysis) and back == q and "components_" not in q.serialize()
    chain = mmk.Config.deserialize("type: Compose\nfunctionals:\n- type: MagSpec\n- type: FactorAnalysis\n  n_components: 8\n")
    assert isinstance(chain.functionals[1], mmk.FactorAnalysis) and chain.functionals[1].n_components == 8
    for absent in ("rotation", "noise_variance_init", "score", "get_covariance", "svd_method"):
        assert not hasattr(p, absent), absent
    assert "random_seed`` is kept" in F.FactorAnalysis.__doc__ and "Known limit" in F.FactorAnalysis.__doc__


def test_refusals_that_need_no_device():
    x = torch.zeros(20, 6)
    with pytest.raises(RuntimeError, match="cpu"):
        mmk.FactorAnalysis(n_components=3)(x)
    with pytest.raises(TypeError, match="float64"):
        mmk.FactorAnalysis(n_components=3)(x.double())
    with pytest.raises(TypeError):
        mmk.FactorAnalysis(n_components=3).torch_func(x.numpy())
    with pytest.raises(ValueError, match="n_components = 0"):
        mmk.FactorAnalysis(n_components=0)(x)
    with pytest.raises(ValueError, match=r"n_components = 7 .*min\(N, D\) = 6"):
        mmk.FactorAnalysis(n_components=7)(x)
    with pytest.raises(ValueError, match="N = 1 frames"):
        mmk.FactorAnalysis(n_components=1)(x[:1])
    with pytest.raises(ValueError, match="max_iter = 0"):
        mmk.FactorAnalysis(n_components=2, max_iter=0)(x)
    with pytest.raises(ValueError, match="tol = -1"):
        mmk.FactorAnalysis(n_components=2, tol=-1.0)(x)
    with pytest.raises(NotImplementedError, match="device tensors only"):
        mmk.FactorAnalysis().np_func(np.zeros((20, 6), dtype=np.float32))
    with pytest.raises(NotImplementedError, match=f"D = {native.PCA_MAX_D + 1}.*PCA_MAX_D"):
        mmk.FactorAnalysis(n_components=2)(torch.zeros(3, native.PCA_MAX_D + 1))
    with pytest.raises(NotImplementedError, match=f"n_components = {native.PCA_MAX_COMPONENTS + 1}.*PCA_MAX_COMPONENTS"):
        mmk.FactorAnalysis(n_components=native.PCA_MAX_COMPONENTS + 1)(torch.zeros(100, 100))
    with pytest.raises(RuntimeError, match="before FactorAnalysis.fit"):
        mmk.FactorAnalysis().transform(x)
    with pytest.raises(RuntimeError, match="MI355X|cpu"):
        native.fa_fit(torch.zeros(6, 6, dtype=torch.float64), 20, 2)
    with pytest.raises(TypeError):
        native.fa_fit(torch.zeros(6, 6), 20, 2)


# ------------------------------------------------------------------------------------------------------------------- the header
def header_prototypes():
    text = re.sub(r"/\*.*?\*/", " ", open(HEADER).read(), flags=re.S)
    return {m.group(2): (m.group(1), m.group(3)) for m in re.finditer(r"\b(int|size_t)\s+(mmk_[a-z0-9_]+)\s*\(([^;{}]*?)\)\s*;", text)}


def test_header_names_signatures_exports_and_macros():
    protos = header_prototypes()
    assert sorted(protos) == sorted(native.FACTOR_ANALYSIS_SYMBOLS) and len(protos) == 4
    others = (set(native.EXPORTED_SYMBOLS) | set(native.KMEANS_SYMBOLS) | set(native.NN_FILTER_SYMBOLS) | set(native.NMF_SYMBOLS)
              | set(native.SAMPLIFY_SYMBOLS) | set(native.SPEC_FILTER_SYMBOLS))
    assert not set(native.FACTOR_ANALYSIS_SYMBOLS) & others
    kinds = {"int64_t": C.c_int64, "int32_t": C.c_int32, "size_t": C.c_size_t, "float": C.c_float, "double": C.c_double,
             "mmk_stream_t": C.c_void_p, "int": C.c_int32}
    lib = native.load_library()
    for name, (res, args) in protos.items():
        want_res, want_args = native._FACTOR_ANALYSIS_SIGNATURES[name]
        assert want_res is kinds[res], name
        got = [C.c_void_p if "*" in a else kinds[a.strip().replace("const ", "").split()[0]] for a in args.split(",")]
        assert got == list(want_args), (name, got, want_args)
        fn = getattr(lib, name)
        assert fn.restype is want_res and list(fn.argtypes) == list(want_args), name
    text = open(HEADER).read()
    main = open(os.path.join(ROOT, "include", "mmk.h")).read()
    assert "#define MMK_FA_MAX_D MMK_PCA_MAX_D" in text and "#define MMK_FA_MAX_COMPONENTS MMK_PCA_MAX_COMPONENTS" in text
    assert float(re.search(r"#define MMK_FA_SMALL (\S+)", text).group(1)) == native.FA_SMALL == R.SMALL == 1e-12
    assert int(re.search(r"#define MMK_FA_POLL (\d+)", text).group(1)) == native.FA_POLL == 8
    assert (native.FA_MAX_D, native.FA_MAX_COMPONENTS) == (native.PCA_MAX_D, native.PCA_MAX_COMPONENTS)
    paragraph = main[main.index("streams.  Every kernel"):main.index("no torch / C++ types")]
    assert "mmk_fa_fit_f64" in paragraph and "mmk_fa_transform_matrix_f64" not in paragraph


def test_the_eigen_kernels_are_shared_not_copied():
    """the QR, H, Jacobi, rotation, residual and finish kernels are defined once, in csrc/subspace_eig.h"""
    csrc = os.path.join(ROOT, "mimikit_amd", "csrc")
    shared = open(os.path.join(csrc, "subspace_eig.h")).read()
    for kernel in ("pca_start_kernel", "pca_qr_kernel", "pca_h_kernel", "pca_jacobi_kernel", "pca_rotate_kernel", "pca_resid_kernel", "pca_finish_kernel"):
        assert len(re.findall(rf"void {kernel}\(", shared)) == 1, kernel
        for user in ("pca.hip", "factor_analysis.hip"):
            text = open(os.path.join(csrc, user)).read()
            assert '#include "subspace_eig.h"' in text and not re.search(rf"void {kernel}\(", text), (user, kernel)
