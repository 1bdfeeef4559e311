"""The factor analysis kernels on the MI355X (csrc/factor_analysis.hip, include/mmk_factor_analysis.h) against the float64 restatement and
the tolerances of tests/factor_analysis_refs.py and the recorded results of sklearn's exact method and of the reference in
tests/golden/factor_analysis.npz: both entry points through the C ABI with poisoned outputs and workspaces, every call made twice for the
same bits (neither takes rows: the frames enter through the covariance, so there is no stride to misalign - the operands sit 8-byte, not
16-byte, aligned in the middle of NaN buffers); the whole fit through mimikit_amd.FactorAnalysis with the EM step count held exactly; the
sign rule; running out of max_iter; other rows; the limits; a fit and a transform behind a busy side stream; a Compose pipeline.  Each
test prints its worst error over its tolerance."""
import ctypes as C
import math
import warnings

import numpy as np
import pytest
import torch

import mimikit_amd as mmk
from mimikit_amd import native
from tests import factor_analysis_refs as R
from tests import stream_cases as S
from tests.f64_bounds import check_written
from tests.test_gpu_pca import front_mask, poisoned, same_bits, to_dev

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

G = R.golden()


def surrounded(a, device):
    """a float64 array in the middle of a NaN buffer, 8-byte but not 16-byte aligned -> (buffer, view)"""
    a = np.ascontiguousarray(a, dtype=np.float64)
    buf = poisoned(a.size + 3, device, 5)
    view = buf[3:3 + a.size].view(a.shape)
    view.copy_(torch.from_numpy(a.copy()))
    return buf, view


def fit_call(c_np, n, k, tol, max_iter, device):
    """mmk_fa_fit_f64 through the C ABI -> (components, noise_variance, loglike, n_iter, converged, inner iterations)"""
    lib = native.lib()
    d = c_np.shape[0]
    b = min(d, k + 16)
    n_work = lib.mmk_fa_fit_workspace_bytes(d, k)
    assert n_work == (4 * d * b + 3 * b * b + b + 2 * d + k) * 8 + 64
    cbuf, c = surrounded(c_np, device)
    before = cbuf.clone()
    work = poisoned(n_work // 8, device)
    comps, noise, ll = poisoned(k * d + 1, device)[1:], poisoned(d + 1, device)[1:], poisoned(max_iter + 1, device)[1:]
    n_iter, conv, inner = C.c_int32(-7), C.c_int32(-7), (C.c_int32 * 3)(-7, -7, -7)
    native.check(lib.mmk_fa_fit_f64(c.data_ptr(), d, k, n, tol, max_iter, comps.data_ptr(), noise.data_ptr(), ll.data_ptr(), C.byref(n_iter),
                                    C.byref(conv), inner, work.data_ptr(), n_work, native.stream_ptr(device)))
    it = int(n_iter.value)
    check_written(comps, front_mask(comps, k * d), "components")
    check_written(noise, front_mask(noise, d), "noise_variance")
    check_written(ll, front_mask(ll, it), "loglike")
    assert bool(torch.isnan(work[n_work // 8:]).all()) and same_bits(torch.nan_to_num(cbuf), torch.nan_to_num(before)) and inner[2] == -7
    assert 1 <= it <= max_iter and conv.value in (0, 1) and inner[0] >= it and 1 <= inner[1] <= inner[0]
    return comps[:k * d].view(k, d), noise[:d], ll[:it], it, bool(conv.value), (inner[0], inner[1])


def matrix_call(w_np, psi_np, device):
    lib = native.lib()
    k, d = w_np.shape
    n_work = lib.mmk_fa_transform_matrix_workspace_bytes(d, k)
    assert n_work == k * k * 8
    wbuf, w = surrounded(w_np, device)
    pbuf, psi = surrounded(psi_np, device)
    before = (wbuf.clone(), pbuf.clone())
    work, a = poisoned(n_work // 8, device), poisoned(k * d + 1, device)[1:]
    native.check(lib.mmk_fa_transform_matrix_f64(w.data_ptr(), psi.data_ptr(), d, k, a.data_ptr(), work.data_ptr(), n_work, native.stream_ptr(device)))
    check_written(a, front_mask(a, k * d), "a")
    assert bool(torch.isnan(work[n_work // 8:]).all())
    assert same_bits(torch.nan_to_num(wbuf), torch.nan_to_num(before[0])) and same_bits(torch.nan_to_num(pbuf), torch.nan_to_num(before[1]))
    return a[:k * d].view(k, d)


def fit_errors(r, comps, noise, ll, name):
    """-> {array: error / tolerance} of a device fit against sklearn's exact method (the golden file), up to one sign per component"""
    want_c, want_p, want_l = G[f"{name}_components"], G[f"{name}_noise_variance"], G[f"{name}_loglike"]
    ll_tol = R.FIT_TOL * np.abs(want_l).max() + r["ll_rounding"]                  # (factor_analysis_refs: ll's own rounding)
    return dict(components_=R.rel_err(R.align(comps.cpu().numpy(), want_c), want_c) / R.FIT_TOL,
                noise_variance_=R.rel_err(noise.cpu().numpy(), want_p) / R.FIT_TOL,
                loglike_=float(np.abs(ll.cpu().numpy() - want_l).max() / ll_tol))


# ------------------------------------------------------------------------------------------------------------------ the C ABI
@pytest.mark.parametrize("name", R.NAMES)
def test_fit_entry_through_the_c_abi(device, name):
    r = R.fixture_case(name)
    f = r["f"]
    got = fit_call(r["cov"], f["n"], f["k"], f["tol"], f["max_iter"], device)
    again = fit_call(r["cov"], f["n"], f["k"], f["tol"], f["max_iter"], device)
    assert all(same_bits(a, b) for a, b in zip(got[:3], again[:3])) and got[3:] == again[3:], "two calls differ"
    wrapped = native.fa_fit(to_dev(r["cov"], device), f["n"], f["k"], f["tol"], f["max_iter"])
    assert all(same_bits(a, b) for a, b in zip(got[:3], wrapped[:3])) and got[3:] == wrapped[3:], "the wrapper differs from the call on the offset operands"
    comps, noise, ll, n_iter, conv, inner = got
    errs = fit_errors(r, comps, noise, ll, name)
    print(f"fa_fit {name}: n_iter {n_iter} (sklearn {int(G[f'{name}_n_iter'])}), {inner[0]} inner iterations ({inner[1]} in EM step 0); worst error / "
          f"tolerance " + ", ".join(f"{k} {v:.4f}" for k, v in errs.items()))
    assert n_iter == int(G[f"{name}_n_iter"]) == r["n_iter"] and conv == r["converged"]
    assert max(errs.values()) <= 1.0, errs
    assert same_bits(comps, torch.from_numpy(R.signed(comps.cpu().numpy())).to(device)), "a row's entry of largest magnitude is not positive"


@pytest.mark.parametrize("name", R.NAMES)
def test_transform_matrix_through_the_c_abi(device, name):
    """A = M^-1 Wpsi with M = I + Wpsi W^T.  The tolerance: a Cholesky solve of a k x k system leaves a relative error of the order of
    k 2^-53 cond(M) (Higham, Accuracy and Stability, 10.1); the explicit inverse and the products add terms of the same size; 64 of them."""
    r = R.fixture_case(name)
    w, psi = r["components"], r["noise_variance"]
    a = matrix_call(w, psi, device)
    assert same_bits(a, matrix_call(w, psi, device)), "two calls differ"
    assert same_bits(a, native.fa_transform_matrix(to_dev(w, device), to_dev(psi, device))), "the wrapper differs"
    want = R.transform_matrix64(w, psi)
    cond = np.linalg.cond(np.eye(len(w)) + (w / psi) @ w.T)
    tol = 64 * len(w) * 2.0 ** -53 * cond
    err = R.rel_err(a.cpu().numpy(), want)
    print(f"fa_transform_matrix {name}: cond(M) {cond:.2e}, worst error / tolerance {err / tol:.4f} (tolerance {tol:.2e} of the largest entry)")
    assert err <= tol


# ------------------------------------------------------------------------------------------------------------------ the whole fit
@pytest.mark.parametrize("name", R.NAMES)
def test_fit_and_transform_against_sklearn(device, name):
    r = R.fixture_case(name)
    f = r["f"]
    xd = to_dev(r["x"], device)
    fa = mmk.FactorAnalysis(n_components=f["k"], tol=f["tol"], max_iter=f["max_iter"])
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        z = fa(xd)
    assert len(caught) == (0 if r["converged"] else 1), [str(c.message) for c in caught]
    assert z.dtype == torch.float32 and z.shape == (f["n"], f["k"]) and z.device.type == "cuda"
    for attr, shape in (("mean_", (f["d"],)), ("components_", (f["k"], f["d"])), ("noise_variance_", (f["d"],)), ("loglike_", (fa.n_iter_,))):
        t = getattr(fa, attr)
        assert t.dtype == torch.float64 and tuple(t.shape) == shape and t.device.type == "cuda", attr
    assert type(fa.n_iter_) is int
    errs = fit_errors(r, fa.components_, fa.noise_variance_, fa.loglike_, name)
    exact = G[f"{name}_scores"]
    top = np.abs(exact).max()
    z64 = z.cpu().numpy().astype(np.float64)
    e32 = np.abs(R.align(z64, exact, by_rows=False) - exact.astype(np.float32).astype(np.float64)).max()
    ref = G[f"{name}_ref_scores"]
    eref = np.abs(R.align(z64, ref, by_rows=False) - ref).max()
    ref_tol = float(G[f"{name}_ref_deviation"]) + R.REF_SLACK * top
    print(f"FactorAnalysis {name}: n_iter {fa.n_iter_} (sklearn {int(G[f'{name}_n_iter'])}); worst error / tolerance "
          + ", ".join(f"{k} {v:.4f}" for k, v in errs.items()) + f", transform {e32 / (R.TRANSFORM_TOL * top):.3f}, against the reference "
          f"{eref / ref_tol:.3f} (r_i = {float(G[f'{name}_ref_deviation']) / top:.2e} of the largest score)")
    assert fa.n_iter_ == int(G[f"{name}_n_iter"])
    assert max(errs.values()) <= 1.0, errs
    assert e32 <= R.TRANSFORM_TOL * top
    assert eref <= ref_tol
    other = mmk.FactorAnalysis(n_components=f["k"], tol=f["tol"], max_iter=f["max_iter"])
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        z2 = other.fit_transform(xd)
    assert torch.equal(z2.view(torch.int32), z.view(torch.int32)) and same_bits(other.components_, fa.components_) and other.n_iter_ == fa.n_iter_
    assert torch.equal(other.transform(xd).view(torch.int32), z.view(torch.int32)), "torch_func is fit(x).transform(x)"


def test_sign_rule(device):
    """each component's entry of largest magnitude is positive, on every fixture - PCA's rule, not the sign sklearn's SVD happens to leave
    (the count of sklearn's components with the other sign is printed)"""
    flipped = total = 0
    for name in R.NAMES:
        r = R.fixture_case(name)
        f = r["f"]
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            fa = mmk.FactorAnalysis(n_components=f["k"], max_iter=f["max_iter"]).fit(to_dev(r["x"], device))
        comps = fa.components_.cpu().numpy()
        rows, at = np.arange(f["k"]), np.abs(comps).argmax(1)
        assert (comps[rows, at] > 0).all(), name
        assert np.array_equal(at, np.abs(r["components"]).argmax(1)), name
        flipped += int((G[f"{name}_components"][rows, at] < 0).sum())
        total += f["k"]
    print(f"sign rule: {flipped} of {total} components of sklearn's exact method have the other sign")


def test_running_out_of_max_iter(device):
    r, full = R.fixture_case("cap3"), R.fixture_case("f24")
    xd = to_dev(r["x"], device)
    fa = mmk.FactorAnalysis(n_components=4, max_iter=3)
    with pytest.warns(RuntimeWarning, match="maximum number of iterations 3"):
        fa.fit(xd)
    assert fa.n_iter_ == 3 and fa.loglike_.shape == (3,)
    psi = fa.noise_variance_.cpu().numpy()
    w = fa.components_.cpu().numpy()
    var = np.diag(r["cov"])
    post = np.maximum(var - (w ** 2).sum(0), R.SMALL)
    assert R.rel_err(psi, post) <= 1e-13, "noise_variance_ is not the psi updated after the last W"
    assert R.rel_err(psi, r["noise_variance"]) <= R.FIT_TOL
    pre = R.fa64(r["x"], 4, max_iter=2)["noise_variance"]                      # the psi the last W was computed with
    assert R.rel_err(psi, pre) > 1e-4
    assert R.rel_err(fa.loglike_.cpu().numpy(), full["loglike"][:3]) <= R.FIT_TOL
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        exact = mmk.FactorAnalysis(n_components=4, max_iter=full["n_iter"]).fit(xd)  # the tolerance stops the last allowed step: no warning
    assert exact.n_iter_ == full["n_iter"]


def test_transform_of_other_rows(device):
    r = R.fixture_case("odd33")
    fa = mmk.FactorAnalysis(n_components=5).fit(to_dev(r["x"], device))
    y = R.frames(12, 37, 33, 5, 2.0)
    want = R.transform64(y, r["mean"], r["components"], r["noise_variance"])
    top = np.abs(r["scores"]).max()
    got = fa.transform(to_dev(y, device))
    assert got.shape == (37, 5) and got.dtype == torch.float32
    err = np.abs(R.align(got.cpu().numpy(), want, by_rows=False) - want.astype(np.float32).astype(np.float64)).max()
    print(f"transform of 37 other rows: worst error / tolerance {err / (R.TRANSFORM_TOL * top):.3f}")
    assert err <= R.TRANSFORM_TOL * top
    one = fa.transform(to_dev(y[17:18], device))
    assert one.shape == (1, 5) and torch.equal(one.view(torch.int32), got[17:18].view(torch.int32))
    sliced = fa.transform(to_dev(np.concatenate([y, y]), device)[37:, :])
    assert torch.equal(sliced.view(torch.int32), got.view(torch.int32))
    with pytest.raises(ValueError, match="D = 33"):
        fa.transform(to_dev(y[:, :20], device))


# ------------------------------------------------------------------------------------------------------------------ limits
def test_what_raises_on_the_device(device):
    x = to_dev(R.fixture_case("f24")["x"], device)
    with pytest.raises(RuntimeError):
        mmk.FactorAnalysis(n_components=2)(x.cpu())
    with pytest.raises(TypeError, match="float32"):
        mmk.FactorAnalysis(n_components=2)(x.double())
    with pytest.raises(ValueError, match=r"n_components = 25 .*min\(N, D\) = 24"):
        mmk.FactorAnalysis(n_components=25)(x)
    with pytest.raises(ValueError, match=r"n_components = 4 .*min\(N, D\) = 3"):
        mmk.FactorAnalysis(n_components=4)(x[:3])
    with pytest.raises(ValueError, match="N = 1 frames"):
        mmk.FactorAnalysis(n_components=1)(x[:1])
    with pytest.raises(NotImplementedError, match=f"D = {native.PCA_MAX_D + 1}.*PCA_MAX_D"):
        mmk.FactorAnalysis(n_components=2)(torch.zeros((3, native.PCA_MAX_D + 1), device=device))
    with pytest.raises(NotImplementedError, match=f"n_components = {native.PCA_MAX_COMPONENTS + 1}.*PCA_MAX_COMPONENTS"):
        mmk.FactorAnalysis(n_components=native.PCA_MAX_COMPONENTS + 1)(torch.zeros((80, 80), device=device))
    with pytest.raises(RuntimeError, match="before FactorAnalysis.fit"):
        mmk.FactorAnalysis().transform(x)
    lib, c = native.lib(), torch.eye(24, dtype=torch.float64, device=device)
    out, it = torch.zeros(4 * 24 + 24 + 8, dtype=torch.float64, device=device), (C.c_int32 * 4)()
    work = torch.zeros(lib.mmk_fa_fit_workspace_bytes(24, 4) // 8, dtype=torch.float64, device=device)
    args = lambda cp=c.data_ptr(), d=24, k=4, n=300, tol=1e-2, mi=8, wb=work.numel() * 8: (
        cp, d, k, n, tol, mi, out.data_ptr(), out.data_ptr() + 8 * 96, out.data_ptr() + 8 * 120, it, C.byref(it, 4), C.byref(it, 8), work.data_ptr(), wb,
        native.stream_ptr(device))
    for bad, code, text in ((args(k=25), -1, "n_components = 25"), (args(n=1), -1, "n = 1 frames"), (args(mi=0), -1, "max_iter = 0"),
                            (args(tol=-1.0), -1, "tol = -1"), (args(cp=c.data_ptr() + 4), -1, "8-byte aligned"), (args(cp=None), -1, "null pointer"),
                            (args(wb=work.numel() * 8 - 8), None, "bytes"), (args(d=native.FA_MAX_D + 1), -3, "MMK_FA_MAX_D")):
        rc = lib.mmk_fa_fit_f64(*bad)
        assert rc < 0 and (code is None or rc == code) and text in lib.mmk_last_error().decode(), (rc, lib.mmk_last_error())
    assert lib.mmk_fa_fit_workspace_bytes(24, 25) == 0 and lib.mmk_fa_transform_matrix_workspace_bytes(24, 65) == 0
    rc = lib.mmk_fa_transform_matrix_f64(out.data_ptr(), out.data_ptr() + 4, 24, 4, out.data_ptr(), work.data_ptr(), 128, native.stream_ptr(device))
    assert rc == -1 and "8-byte aligned" in lib.mmk_last_error().decode()
    again = mmk.FactorAnalysis(n_components=4)(x)                                # (and the next call is a fresh one)
    assert torch.equal(again, mmk.FactorAnalysis(n_components=4)(x))


# ------------------------------------------------------------------------------------------------------------------ the stream contract
def _cov(seed):
    x = R.frames(1 if seed == 0 else 11, 300, 24, 4, 3.0).astype(np.float64)
    xc = x - x.mean(0)
    return xc.T @ xc / 300


def _stream_fit():
    d, k, steps = 24, 4, 3                                  # (max_iter = 3: every entry of loglike is written whatever the input)

    def call(L, a, s):
        it = (C.c_int32 * 4)()
        return L.mmk_fa_fit_f64(S.P(a["c"]), d, k, 300, 1e-2, steps, S.P(a["components"]), S.P(a["noise_variance"]), S.P(a["loglike"]), it,
                                C.byref(it, 4), C.byref(it, 8), S.P(a["ws"]), a["ws"].numel(), s)
    return S.Case("mmk_fa_fit_f64", lambda seed: dict(c=torch.from_numpy(_cov(seed))),
                  lambda L, i: dict(components=((k, d), torch.float64), noise_variance=((d,), torch.float64), loglike=((steps,), torch.float64)),
                  call, work=lambda L, i: dict(ws=L.mmk_fa_fit_workspace_bytes(d, k)))


def _stream_transform():
    m, d, k = 37, 33, 5

    def build(seed):
        r = R.fixture_case("odd33")
        y = R.frames(12 + seed % 2 + seed // 7919, m, d, k, 2.0)
        scale = 1.0 if seed == 0 else 0.75
        return dict(y=torch.from_numpy(y), mean=torch.from_numpy(r["mean"] * scale), ones=torch.ones(d, dtype=torch.float64),
                    w=torch.from_numpy(r["components"] * scale), psi=torch.from_numpy(r["noise_variance"].copy()))

    def call(L, a, s):
        rc = L.mmk_fa_transform_matrix_f64(S.P(a["w"]), S.P(a["psi"]), d, k, S.P(a["a"]), S.P(a["ws"]), a["ws"].numel(), s)
        return rc or L.mmk_pca_project_f32(S.P(a["y"]), d, m, d, S.P(a["mean"]), S.P(a["ones"]), S.P(a["a"]), k, S.P(a["out"]), k, s)
    return S.Case("mmk_fa_transform_matrix_f64", build, lambda L, i: dict(a=((k, d), torch.float64), out=((m, k), torch.float32)), call, tag="transform",
                  work=lambda L, i: dict(ws=L.mmk_fa_transform_matrix_workspace_bytes(d, k)))


STREAM_CASES = [_stream_fit(), _stream_transform()]


@pytest.mark.parametrize("case", STREAM_CASES, ids=[c.id for c in STREAM_CASES])
def test_fit_and_transform_behind_a_busy_side_stream(device, case):
    """tests/test_gpu_streams.py's method: the real input twice on the default stream (the same bits), the stale input once (other bits),
    then behind a delay and a late write of the input on a side stream: the default-stream bits.  (A launch that left its stream would
    have read the stale input.)  The transform matrix returns without waiting; the fit waits for its stream by design."""
    bound = S.Bound(case, device)
    want, again = bound.run_default("real"), bound.run_default("real")
    assert not S.differs(want, again), (case.id, "two default-stream calls disagree")
    bound.check_surround(case.id + " on the default stream")
    assert S.differs(want, bound.run_default("stale")), (case.id, "the stale input gives the real outputs")
    got, busy, host = S.late_input(bound, S.side_stream(device))
    print(f"[streams] {case.id}: host time of the call {host * 1e3:.3f} ms, busy on return: {busy}")
    assert not S.differs(want, got), (case.id, "behind a late input on a side stream the outputs differ from the default-stream run")
    bound.check_surround(case.id + " on the side stream")
    if case.entry == "mmk_fa_transform_matrix_f64":
        assert busy, "the transform matrix and the projection waited for their stream"


# ------------------------------------------------------------------------------------------------------------------ a pipeline
def test_compose_magspec_factor_analysis_stays_on_the_device(device):
    g = torch.Generator().manual_seed(5)
    t = torch.arange(16384, dtype=torch.float64)
    wave = sum((1.0 - 0.1 * j) * (1.0 + 0.8 * torch.sin(2 * math.pi * t / period + j)) * torch.sin(2 * math.pi * t * bin_ / 128.0)
               for j, (bin_, period) in enumerate(((6, 700.0), (16, 1100.0), (28, 1700.0), (44, 2300.0))))
    wave = (wave / 4 + 0.05 * torch.randn(16384, generator=g, dtype=torch.float64)).float().to(device)
    chain = mmk.Compose(mmk.MagSpec(n_fft=128, hop_length=32), mmk.FactorAnalysis(4))
    z = chain(wave)
    spec = mmk.MagSpec(n_fft=128, hop_length=32)(wave)
    assert z.device.type == "cuda" and z.dtype == torch.float32 and z.shape == (spec.shape[0], 4) and spec.shape[1] == 65
    assert bool(torch.isfinite(z).all())
    fa = mmk.FactorAnalysis(4)
    assert torch.equal(fa(spec).view(torch.int32), z.view(torch.int32)), "the chain differs from the two calls made separately"
    print(f"Compose(MagSpec(128, 32), FactorAnalysis(4)): {z.shape[0]} frames of 65 bins, {fa.n_iter_} EM steps, largest score {float(z.abs().max()):.3f}")
