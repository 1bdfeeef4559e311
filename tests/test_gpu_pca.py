"""The PCA kernels on the MI355X (csrc/pca.hip) against the float64 restatement and derived bounds of tests/pca_refs.py: every entry point
through the C ABI on strided, misaligned rows with poisoned outputs and workspace, every call made twice for the same bits, the
covariance's MFMA map on exact integers, and mimikit_amd.PCA on device tensors.  Each test prints its worst error / bound."""
import ctypes as C

import numpy as np
import pytest
import torch

import mimikit_amd as mmk
from mimikit_amd import native
from tests import pca_refs as R
from tests.f64_bounds import check_written
from tests.strided_inputs import FLOAT_SURROUNDS, Strided, surround_rule

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

NAMES = sorted(R.FIXTURES)
NAN = float("nan")


def same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.int64), b.contiguous().view(torch.int64))


def poisoned(n, device, extra=3):
    return torch.full((n + extra,), NAN, dtype=torch.float64, device=device)


def front_mask(buf, n):
    mask = torch.zeros(buf.shape, dtype=torch.bool)
    mask[:n] = True
    return mask


def to_dev(a, device):
    return torch.from_numpy(np.array(a)).to(device)        # (a copy: the fixtures are read-only)


@surround_rule(*FLOAT_SURROUNDS)
def colstats_call(x_np, device):
    lib = native.lib()
    x = Strided.of(x_np, 1, device)
    n, d = x_np.shape
    n_work = lib.mmk_pca_colstats_workspace_bytes(n, d)
    assert n_work == (min(-(-n // 256), 1024) + 1) * d * 8
    work, mean, scale = poisoned(n_work // 8, device), poisoned(d, device), poisoned(d, device)
    native.check(lib.mmk_pca_colstats_f64(x.ptr, x.stride, n, d, mean.data_ptr(), scale.data_ptr(), work.data_ptr(), n_work,
                                          native.stream_ptr(device)))
    check_written(mean, front_mask(mean, d), "mean")
    check_written(scale, front_mask(scale, d), "scale")
    assert bool(torch.isnan(work[n_work // 8:]).all()) and x.untouched(), "the workspace was written beyond its size, or the input was written"
    return mean[:d], scale[:d]


@surround_rule(*FLOAT_SURROUNDS)
def cov_call(x_np, mean, scale, device):
    lib = native.lib()
    x = Strided.of(x_np, 3, device)
    n, d = x_np.shape
    n_work = lib.mmk_pca_cov_workspace_bytes(n, d)
    assert 0 < n_work and n_work % (64 * 64 * 8) == 0
    work, c = poisoned(n_work // 8, device), poisoned(d * d, device, 5)
    native.check(lib.mmk_pca_cov_f64(x.ptr, x.stride, n, d, mean.data_ptr(), scale.data_ptr(), c.data_ptr(), work.data_ptr(), n_work,
                                     native.stream_ptr(device)))
    check_written(c, front_mask(c, d * d), f"covariance {n, d}")
    assert bool(torch.isnan(work[n_work // 8:]).all()) and x.untouched(), "the workspace was written beyond its size, or the input was written"
    return c[:d * d].reshape(d, d)


def eig_call(c, k, device, max_iter=0):
    lib = native.lib()
    d = c.shape[0]
    n_work = lib.mmk_pca_eig_workspace_bytes(d, k)
    b = R.block_width(d, k)
    assert n_work == (4 * d * b + 3 * b * b + b + d + k + 4) * 8
    work, comps, var = poisoned(n_work // 8, device), poisoned(k * d, device), poisoned(k, device)
    before, n_iter = c.clone(), C.c_int32(-7)
    native.check(lib.mmk_pca_eig_f64(c.data_ptr(), d, k, max_iter, comps.data_ptr(), var.data_ptr(), C.byref(n_iter), work.data_ptr(), n_work,
                                     native.stream_ptr(device)))
    check_written(comps, front_mask(comps, k * d), f"components {k, d}")
    check_written(var, front_mask(var, k), "variance")
    assert bool(torch.isnan(work[n_work // 8:]).all()) and torch.equal(c, before), "the workspace was written beyond its size, or C was written"
    return comps[:k * d].reshape(k, d), var[:k], int(n_iter.value)


@surround_rule(*FLOAT_SURROUNDS)
def project_call(y_np, mean, scale, comps, device):
    lib = native.lib()
    y = Strided.of(y_np, 2, device)
    m, d = y_np.shape
    k = comps.shape[0]
    stride = k + 3
    out = torch.full((1 + m * stride + 4,), NAN, dtype=torch.float32, device=device)
    native.check(lib.mmk_pca_project_f32(y.ptr, y.stride, m, d, mean.data_ptr(), scale.data_ptr(), comps.data_ptr(), k, out.data_ptr() + 4, stride,
                                         native.stream_ptr(device)))
    mask = torch.zeros(out.shape, dtype=torch.bool)
    mask[1:1 + m * stride].view(m, stride)[:, :k] = True
    check_written(out, mask, f"scores {m, k}")
    assert y.untouched()
    return out[1:1 + m * stride].view(m, stride)[:, :k]


FITTED = {}


def fitted(name, device):
    """the device's statistics, covariance and components of a fixture through the Python wrappers, once per session, with the a posteriori
    component test of tests/pca_refs.py made on them"""
    if name not in FITTED:
        x, p, e, allow, null, margins = R.fixture_case(name)
        xd = to_dev(x, device)
        mean, scale = native.pca_colstats(xd)
        c = native.pca_cov(xd, mean, scale)
        comps, var, n_iter = native.pca_eig(c, p["k"])
        r = R.check_components(p, comps.cpu().numpy(), f"{name}: device components", allow)
        FITTED[name] = dict(xd=xd, mean=mean, scale=scale, c=c, comps=comps, var=var, n_iter=n_iter, r=r)
    return FITTED[name]


# ------------------------------------------------------------------------------------------------------------------ column statistics
@pytest.mark.parametrize("name", NAMES)
def test_colstats_against_the_bound(device, name):
    x, p, e, allow, null, margins = R.fixture_case(name)
    mean, scale = colstats_call(x, device)
    again = colstats_call(x, device)
    assert same_bits(mean, again[0]) and same_bits(scale, again[1]), "two calls differ"
    wm, ws = native.pca_colstats(to_dev(x, device))
    assert same_bits(mean, wm) and same_bits(scale, ws), "the wrapper on contiguous rows differs from the strided call"
    mean_bound, scale_bound = R.stats_bounds(p)
    em, es = np.abs(mean.cpu().numpy() - p["mean"]), np.abs(scale.cpu().numpy() - p["scale"])
    print(f"pca_colstats {name}: worst error / bound {max((em / mean_bound).max(), (es / np.maximum(scale_bound, 1e-300)).max()):.3f}")
    assert (em <= mean_bound).all() and (es <= scale_bound).all()
    assert ((scale.cpu().numpy() == 1.0) == p["const"]).all(), "the constant-column rule"


@pytest.mark.parametrize("n,d", ((1, 1), (1, 3), (2, 1), (2, 3), (257, 33)))
def test_the_smallest_rows(device, n, d):
    """one row, one column, a row shorter than any vector load, one row more than a block of 256: the three strided entry points under the
    surround rule, the statistics inside the float64 bound, covariance and scores the bits of the wrappers on contiguous rows"""
    x = np.random.default_rng(100 * n + d).standard_normal((n, d)).astype(np.float32)
    p = R.pca64(x, 1) if n > 1 else None
    mean, scale = colstats_call(x, device)
    xd = to_dev(x, device)
    wm, ws = native.pca_colstats(xd)
    assert same_bits(mean, wm) and same_bits(scale, ws), "the wrapper on contiguous rows differs from the strided call"
    if n == 1:                                              # a single row: its own mean exactly, every column constant
        assert np.array_equal(mean.cpu().numpy(), x[0].astype(np.float64)) and bool((scale == 1.0).all())
    else:
        mean_bound, scale_bound = R.stats_bounds(p)
        em, es = np.abs(mean.cpu().numpy() - p["mean"]), np.abs(scale.cpu().numpy() - p["scale"])
        assert (em <= mean_bound).all() and (es <= scale_bound).all()
        c = cov_call(x, mean, scale, device)
        assert same_bits(c, native.pca_cov(xd, mean, scale)) and torch.equal(c, c.t())
    comps = torch.eye(d, dtype=torch.float64, device=device)[:min(d, 2)].contiguous()
    got = project_call(x, mean, scale, comps, device)
    want = native.pca_project(xd, mean, scale, comps)
    assert torch.equal(got.contiguous().view(torch.int32), want.view(torch.int32)), "the wrapper on contiguous rows differs from the strided call"
    print(f"pca entry points on {n} x {d}: worst error / bound 0.000 (bits of the wrappers)")


# ------------------------------------------------------------------------------------------------------------------ covariance
def test_covariance_layout_on_exact_integers(device):
    """every product and sum is exact in fp64, so any wrong row or column of the f64 MFMA map shows as a wrong integer"""
    x, want = R.layout_case()
    d = x.shape[1]
    zeros, ones = torch.zeros((d,), dtype=torch.float64, device=device), torch.ones((d,), dtype=torch.float64, device=device)
    c = cov_call(x, zeros, ones, device)
    wrong = int((c.cpu().numpy() != want).sum())
    print(f"pca_cov layout 48 x 35: {wrong} of {d * d} entries differ from numpy's exact result (worst error / bound {float(wrong):.3f})")
    assert wrong == 0
    assert torch.equal(c, c.t())


@pytest.mark.parametrize("name", NAMES)
def test_covariance_against_the_bound(device, name):
    x, p, e, allow, null, margins = R.fixture_case(name)
    f = fitted(name, device)
    c = cov_call(x, f["mean"], f["scale"], device)
    again = cov_call(x, f["mean"], f["scale"], device)
    assert same_bits(c, again) and same_bits(c, f["c"]), "two calls differ"
    assert torch.equal(c, c.t()), "C is not mirrored exactly"
    err = np.abs(c.cpu().numpy() - p["c"])
    floor = e + 1e-300
    print(f"pca_cov {name}: worst error / bound {(err / floor).max():.3f}")
    assert (err <= floor).all()


# ------------------------------------------------------------------------------------------------------------------ eigenpairs
@pytest.mark.parametrize("name", NAMES)
def test_components_a_posteriori(device, name):
    x, p, e, allow, null, margins = R.fixture_case(name)
    f = fitted(name, device)
    comps, var, n_iter = eig_call(f["c"], p["k"], device)
    again = eig_call(f["c"], p["k"], device)
    assert same_bits(comps, again[0]) and same_bits(var, again[1]) and n_iter == again[2], "two calls differ"
    assert same_bits(comps, f["comps"]) and same_bits(var, f["var"]) and n_iter == f["n_iter"]
    r = R.check_components(p, comps.cpu().numpy(), name, allow)
    assert np.array_equal(r["null"], null)
    got = var.cpu().numpy()
    assert (got >= 0).all() and (np.abs(got - p["evals"][:p["k"]]) <= r["resid"] + allow).all(), "explained variance"
    at = np.abs(comps.cpu().numpy()).argmax(1)
    assert (comps.cpu().numpy()[np.arange(p["k"]), at] > 0).all(), "a component's entry of largest magnitude is not positive"
    sketch = R.subspace64(p["c"], p["k"])[2]
    print(f"pca_eig {name}: {n_iter} iterations (the numpy sketch: {sketch}), worst error / bound {r['worst']:.3f}, largest residual "
          f"{r['resid'].max():.3e} of {allow:.3e} allowed")
    assert 1 <= n_iter <= 4 * sketch + 8


def test_iteration_cap_raises_with_the_residual(device):
    f = fitted("iid", device)
    with pytest.raises(RuntimeError, match=r"3 iterations .* residual of \d\.\d+e-\d+"):
        native.pca_eig(f["c"], 8, max_iter=3)
    comps, var, n_iter = native.pca_eig(f["c"], 8)                       # (and the next call is a fresh one)
    assert same_bits(comps, f["comps"]) and n_iter == f["n_iter"] > 50   # the loop and the stop rule really ran


# ------------------------------------------------------------------------------------------------------------------ projection and PCA
@pytest.mark.parametrize("name", NAMES)
def test_scores_against_the_bound(device, name):
    x, p, e, allow, null, margins = R.fixture_case(name)
    f = fitted(name, device)
    got = project_call(x, f["mean"], f["scale"], f["comps"], device)
    again = project_call(x, f["mean"], f["scale"], f["comps"], device)
    assert torch.equal(got.contiguous().view(torch.int32), again.contiguous().view(torch.int32)), "two calls differ"
    bound = R.score_bound(p, f["r"]["vec_bound"], null, allow)
    err = np.abs(got.cpu().numpy().astype(np.float64) - R.score_target(p, null))
    print(f"pca_project {name}: worst error / bound {(err / bound).max():.3f}; null columns {int(null.sum())}, their largest |score| "
          f"{np.abs(got.cpu().numpy()[:, null]).max() if null.any() else 0:.2e}")
    assert (err <= bound).all()
    k = p["k"]
    pca = mmk.PCA(n_components=k)
    whole = pca(f["xd"])
    assert whole.dtype == torch.float32 and whole.shape == (p["n"], k) and whole.device.type == "cuda"
    assert torch.equal(whole.view(torch.int32), got.contiguous().view(torch.int32)), "PCA()(x) differs from the entry points' scores"
    other = mmk.PCA(n_components=k).fit(f["xd"])
    assert torch.equal(other.transform(f["xd"]).view(torch.int32), whole.view(torch.int32)), "fit(x).transform(x) differs from PCA()(x)"
    for t, shape in ((other.mean_, (p["d"],)), (other.scale_, (p["d"],)), (other.components_, (k, p["d"])), (other.explained_variance_, (k,))):
        assert t.dtype == torch.float64 and t.device.type == "cuda" and tuple(t.shape) == shape
    assert type(other.n_iter_) is int and other.n_iter_ == f["n_iter"]


def test_transform_of_frames_that_were_not_fitted(device):
    x = R.fixture_frames("full")
    fit_rows, new_rows, k = x[:220], x[220:], 8
    p = R.pca64(fit_rows, k)
    allow = R.resid_allow(p)
    null = R.null_columns(p, allow)
    assert not null.any() and (R.gaps(p["evals"][:k], p["evals"]) >= R.MARGIN * allow).all()
    pca = mmk.PCA(n_components=k).fit(to_dev(fit_rows, device))
    r = R.check_components(p, pca.components_.cpu().numpy(), "full[:220]", allow)
    got = pca.transform(to_dev(new_rows, device))
    z = (new_rows.astype(np.float64) - p["mean"]) / p["scale"]
    want = z @ p["comps"].T
    bound = R.score_bound(p, r["vec_bound"], null, allow, z=z, scores=want)
    err = np.abs(got.cpu().numpy().astype(np.float64) - want)
    print(f"PCA.transform of {new_rows.shape[0]} new frames: worst error / bound {(err / bound).max():.3f}")
    assert got.shape == (new_rows.shape[0], k) and (err <= bound).all()
    sliced = pca.transform(to_dev(x, device)[220:, :])                    # a view with an offset, not a copy
    assert torch.equal(sliced.view(torch.int32), got.view(torch.int32))
    with pytest.raises(ValueError, match="D = 130"):
        pca.transform(to_dev(new_rows[:, :100], device))


def test_pca_in_front_of_qcluster(device):
    x = to_dev(R.fixture_frames("tall"), device)
    low = mmk.PCA(n_components=8)(x)
    q = mmk.QCluster().fit(low)
    assert q.labels_.shape == (600,) and q.labels_.dtype == torch.int64 and 1 <= q.K_ <= 600
    assert int(q.labels_.max()) == q.K_ - 1


def test_limits_raise_by_name(device):
    with pytest.raises(NotImplementedError, match=f"D = {native.PCA_MAX_D + 1}.*PCA_MAX_D"):
        mmk.PCA(n_components=2)(torch.zeros((3, native.PCA_MAX_D + 1), device=device))
    with pytest.raises(NotImplementedError, match=f"n_components = {native.PCA_MAX_COMPONENTS + 1}.*PCA_MAX_COMPONENTS"):
        mmk.PCA(n_components=native.PCA_MAX_COMPONENTS + 1)(torch.zeros((80, 80), device=device))
    with pytest.raises(NotImplementedError, match="PCA_MAX_COMPONENTS"):
        native.pca_eig(torch.eye(80, dtype=torch.float64, device=device), native.PCA_MAX_COMPONENTS + 1)
    with pytest.raises(TypeError):
        mmk.PCA(n_components=2)(torch.zeros((8, 4), dtype=torch.float64, device=device))
    with pytest.raises(RuntimeError):
        mmk.PCA(n_components=2)(torch.zeros((8, 4)))
    widest = mmk.PCA(n_components=native.PCA_MAX_COMPONENTS)              # the widest block (80 columns) runs
    x = torch.from_numpy(np.random.default_rng(5).standard_normal((200, 90)).astype(np.float32)).to(device)
    s = widest(x)
    gram = (s.double().t() @ s.double()).cpu().numpy() / 199
    off = np.abs(gram - np.diag(np.diag(gram))).max()
    assert s.shape == (200, 64) and off <= 1e-5 * np.diag(gram).max(), f"the scores of 64 components are not uncorrelated: {off:.3e}"
    assert np.allclose(np.diag(gram), widest.explained_variance_.cpu().numpy(), rtol=1e-5)
