"""The NMF kernels on the MI355X (csrc/nmf.hip, include/mmk_nmf.h) against the float64 restatement, the derived bounds and the measured
tolerance of tests/nmf_refs.py and the reference's results in tests/golden/nmf.npz: every entry point through the C ABI on strided,
misaligned rows with poisoned outputs and workspaces, every call made twice for the same bits; one half-sweep against the half-sweep
bound; the start against its a-posteriori bound; the whole fit and transform through mimikit_amd.NMF with the iteration count held
exactly; the convergence flag; the limits; and a fit and a transform behind a busy side stream.  Each test prints its worst error / bound."""
import ctypes as C
import warnings

import numpy as np
import pytest
import torch

import mimikit_amd as mmk
from mimikit_amd import native
from tests import nmf_refs as R
from tests import stream_cases as S
from tests.f64_bounds import check_written
from tests.strided_inputs import FLOAT_SURROUNDS, Strided, surround_rule
from tests.test_gpu_pca import front_mask, poisoned, same_bits, to_dev

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

G = R.golden()
NAN = float("nan")


def surrounded(a, device):
    """a float64 array in the middle of a NaN buffer -> (buffer, view)"""
    a = np.ascontiguousarray(a)
    buf = poisoned(a.size + 3, device, 5)
    view = buf[3:3 + a.size].view(a.shape)
    view.copy_(torch.from_numpy(a.copy()))
    return buf, view


def mid_mask(buf, n):
    mask = torch.zeros(buf.shape, dtype=torch.bool)
    mask[3:3 + n] = True
    return mask


@surround_rule(*FLOAT_SURROUNDS)
def start_call(x_np, k, device):
    lib = native.lib()
    x = Strided.of(x_np, 1, device)
    n, d = x_np.shape
    n_work = lib.mmk_nmf_start_workspace_bytes(n, d, k)
    assert n_work > lib.mmk_pca_cov_workspace_bytes(n, d) + lib.mmk_pca_eig_workspace_bytes(d, k) + d * d * 8
    work = poisoned(n_work // 8, device)
    w, ht, s, v = poisoned(n * k, device), poisoned(d * k, device), poisoned(k, device), poisoned(k * d, device)
    part = torch.full((k + 2,), -7, dtype=torch.int32, device=device)
    native.check(lib.mmk_nmf_start_f64(x.ptr, x.stride, n, d, k, w.data_ptr(), ht.data_ptr(), s.data_ptr(), v.data_ptr(), part.data_ptr(),
                                       work.data_ptr(), n_work, native.stream_ptr(device)))
    for buf, count, what in ((w, n * k, "w"), (ht, d * k, "ht"), (s, k, "s"), (v, k * d, "v")):
        check_written(buf, front_mask(buf, count), f"start {what}")
    assert bool(torch.isnan(work[n_work // 8:]).all()) and x.untouched() and bool((part[k:] == -7).all())
    return w[:n * k].view(n, k), ht[:d * k].view(d, k), s[:k], v[:k * d].view(k, d), part[:k]


@surround_rule(*FLOAT_SURROUNDS)
def half_call(which, x_np, w_np, ht_np, device):
    """one half-sweep through the C ABI -> (the updated factor, the violation); the other factor must stay untouched"""
    lib = native.lib()
    x = Strided.of(x_np, 2, device)
    n, d = x_np.shape
    k = w_np.shape[1]
    n_work = lib.mmk_nmf_half_workspace_bytes(n, d, k)
    assert n_work > 0
    work = poisoned(n_work // 8, device)
    wbuf, w = surrounded(w_np, device)
    hbuf, ht = surrounded(ht_np, device)
    viol = poisoned(1, device)
    fn = lib.mmk_nmf_w_half_f64 if which == "w" else lib.mmk_nmf_h_half_f64
    a, b = (ht, w) if which == "w" else (w, ht)
    native.check(fn(x.ptr, x.stride, n, d, k, a.data_ptr(), b.data_ptr(), viol.data_ptr(), work.data_ptr(), n_work, native.stream_ptr(device)))
    check_written(wbuf, mid_mask(wbuf, n * k), "w")
    check_written(hbuf, mid_mask(hbuf, d * k), "ht")
    check_written(viol, front_mask(viol, 1), "violation")
    assert bool(torch.isnan(work[n_work // 8:]).all()) and x.untouched()
    fixed, fixed_np = (ht, ht_np) if which == "w" else (w, w_np)
    assert np.array_equal(fixed.cpu().numpy(), fixed_np), "the factor that is held fixed was written"
    return (w if which == "w" else ht).clone(), viol[:1].clone()


@surround_rule(*FLOAT_SURROUNDS)
def solve_call(x_np, w_np, ht_np, device, update_h=True, tol=1e-4, max_iter=200, poll=0):
    lib = native.lib()
    x = Strided.of(x_np, 3, device)
    n, d = x_np.shape
    k = w_np.shape[1]
    n_work = lib.mmk_nmf_solve_workspace_bytes(n, d, k)
    work = poisoned(n_work // 8, device)
    wbuf, w = surrounded(w_np, device)
    hbuf, ht = surrounded(ht_np, device)
    n_iter = C.c_int32(-7)
    native.check(lib.mmk_nmf_solve_f64(x.ptr, x.stride, n, d, k, w.data_ptr(), ht.data_ptr(), 1 if update_h else 0, tol, max_iter, poll, 1,
                                       C.byref(n_iter), work.data_ptr(), n_work, native.stream_ptr(device)))
    check_written(wbuf, mid_mask(wbuf, n * k), "w")
    check_written(hbuf, mid_mask(hbuf, d * k), "ht")
    assert bool(torch.isnan(work[n_work // 8:]).all()) and x.untouched()
    return w.clone(), ht.clone(), int(n_iter.value)


# ------------------------------------------------------------------------------------------------------------------ the start
@pytest.mark.parametrize("name", R.NAMES)
def test_start_against_the_a_posteriori_bound(device, name):
    r = R.fixture_case(name)
    k = r["f"]["k"]
    w, ht, s, v, part = start_call(r["x"], k, device)
    again = start_call(r["x"], k, device)
    assert all(same_bits(a, b) for a, b in zip((w, ht, s, v), again[:4])) and torch.equal(part, again[4]), "two calls differ"
    ww, wh, ws, wv, wp = native.nmf_start(to_dev(r["x"], device), k)
    assert same_bits(w, ww) and same_bits(ht, wh) and torch.equal(part, wp), "the wrapper on contiguous rows differs from the strided call"
    b = R.start_bound(r["x"], k, v.cpu().numpy())
    st = b["start"]
    ew, eh = np.abs(w.cpu().numpy() - st["w"]), np.abs(ht.cpu().numpy() - st["ht"])
    print(f"nmf_start {name}: worst error / bound {max((ew / b['dw']).max(), (eh / b['dht']).max()):.3f}; parts {part.cpu().numpy().tolist()}")
    assert np.array_equal(part.cpu().numpy(), b["part"]), "another part was chosen"
    assert (ew <= b["dw"]).all() and (eh <= b["dht"]).all()
    assert (np.abs(s.cpu().numpy() - st["s"]) <= 1e-9 * st["s"][0]).all()


# ------------------------------------------------------------------------------------------------------------------ one half-sweep
@pytest.mark.parametrize("name", R.NAMES)
def test_half_sweeps_against_the_bound(device, name):
    x64, w0, ht0 = R.sweep_inputs(name)
    x = R.fixture_case(name)["x"]
    n, d = x.shape
    worst = []
    w1, v1 = half_call("w", x, w0, ht0, device)
    again = half_call("w", x, w0, ht0, device)
    assert same_bits(w1, again[0]) and same_bits(v1, again[1]), "two calls differ"
    want = w0.copy()
    v_want = R.w_half64(x64, want, ht0)
    da, dv = R.sweep_bound(x64, ht0, w0, d)
    ew, ev = np.abs(w1.cpu().numpy() - want), abs(float(v1) - v_want)
    worst += [(ew / np.maximum(da, 1e-300)).max(), ev / dv]
    assert (ew <= da).all() and ev <= dv, f"W half: worst error / bound {worst}"
    h1, v2 = half_call("h", x, want, ht0, device)
    again = half_call("h", x, want, ht0, device)
    assert same_bits(h1, again[0]) and same_bits(v2, again[1]), "two calls differ"
    hwant = ht0.copy()
    v_want = R.h_half64(x64, want, hwant)
    da, dv = R.sweep_bound(x64.T, want, ht0, n)
    eh, ev = np.abs(h1.cpu().numpy() - hwant), abs(float(v2) - v_want)
    worst += [(eh / np.maximum(da, 1e-300)).max(), ev / dv]
    print(f"nmf half-sweeps {name}: worst error / bound W {worst[0]:.3f}, its violation {worst[1]:.3f}, H {worst[2]:.3f}, its violation {worst[3]:.3f}")
    assert (eh <= da).all() and ev <= dv
    xd, wd, hd = to_dev(x, device), to_dev(w0, device), to_dev(ht0, device)
    vw = native.nmf_w_half(xd, wd, hd)
    assert same_bits(wd, w1) and same_bits(vw, v1) and np.array_equal(hd.cpu().numpy(), ht0), "the wrapper on contiguous rows differs"
    wd, hd = to_dev(want, device), to_dev(ht0, device)
    vh = native.nmf_h_half(xd, wd, hd)
    assert same_bits(hd, h1) and same_bits(vh, v2) and np.array_equal(wd.cpu().numpy(), want), "the wrapper on contiguous rows differs"


# ------------------------------------------------------------------------------------------------------------------ the whole fit
@pytest.mark.parametrize("name", R.NAMES)
def test_fit_and_transform_against_the_reference(device, name):
    r = R.fixture_case(name)
    f = r["f"]
    tol_w, tol_h, tol_t = R.fit_tolerance(name)
    xd, yd = to_dev(r["x"], device), to_dev(r["y"], device)
    nmf = mmk.NMF(n_components=f["k"], tol=f["tol"], max_iter=f["max_iter"])
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        w = nmf(xd)
        tw = nmf.transform(yd)
    want_warnings = (2 if r["tn"] == f["max_iter"] else 1) if (r["n_iter"] == f["max_iter"] and f["tol"] > 0) else 0
    assert len(caught) == want_warnings, [str(c.message) for c in caught]
    assert w.dtype == torch.float32 and w.shape == (f["n"], f["k"]) and w.device.type == "cuda"
    assert nmf.components_.dtype == torch.float64 and nmf.components_.shape == (f["k"], f["d"]) and type(nmf.n_iter_) is int
    ew = np.abs(w.cpu().numpy().astype(np.float64) - G[f"{name}_w"].astype(np.float64))
    eh = np.abs(nmf.components_.cpu().numpy() - G[f"{name}_components"])
    et = np.abs(tw.cpu().numpy().astype(np.float64) - G[f"{name}_transform"])
    if name == "runs":
        tol_w += R.half_ulp32(np.abs(r["w"]).max())                               # (its golden W is stored as float32: one more rounding)
    print(f"NMF {name}: n_iter {nmf.n_iter_} (reference {int(G[f'{name}_n_iter'])}); worst error / tolerance W {ew.max() / tol_w:.3f}, "
          f"components_ {eh.max() / tol_h:.4f}, transform {et.max() / tol_t:.3f}; tolerances {tol_w:.2e}, {tol_h:.2e}, {tol_t:.2e}; "
          f"components_ (float64 on both sides) are {eh.max() / R.spread(name)[1]:.1f} spreads from the reference")
    assert nmf.n_iter_ == int(G[f"{name}_n_iter"])
    assert (ew <= tol_w).all() and (eh <= tol_h).all() and (et <= tol_t).all()
    other = mmk.NMF(n_components=f["k"], tol=f["tol"], max_iter=f["max_iter"]).fit(xd)
    assert same_bits(other.components_, nmf.components_) and other.n_iter_ == nmf.n_iter_
    if name == "odd":
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            again = other.transform(xd)
        assert not torch.equal(again, w), "fit(x).transform(x) is fit_transform(x): transform does not solve again from zeros"
        sliced = other.transform(to_dev(np.concatenate([r["y"], r["y"]]), device)[R.TRANSFORM_ROWS:, :])
        assert torch.equal(sliced.view(torch.int32), tw.view(torch.int32))


# ------------------------------------------------------------------------------------------------------------------ the convergence flag
def test_the_flag_freezes_the_result_whenever_the_host_looks(device):
    r = R.fixture_case("loose")
    f, st = r["f"], r["start"]
    stop = r["n_iter"]
    assert stop % 8 != 0 and stop % 3 != 0 and 8 < stop < 24
    w, ht, n_iter = solve_call(r["x"], st["w"], st["ht"], device, tol=f["tol"], max_iter=200)
    assert n_iter == stop == int(G["loose_n_iter"])
    for max_iter, poll in ((stop, 0), (200, 3), (200, stop), (200, 1), (stop + 1, 200)):
        w2, ht2, n2 = solve_call(r["x"], st["w"], st["ht"], device, tol=f["tol"], max_iter=max_iter, poll=poll)
        assert n2 == stop and same_bits(w, w2) and same_bits(ht, ht2), (max_iter, poll)
    w3, ht3, n3 = solve_call(r["x"], st["w"], st["ht"], device, tol=f["tol"], max_iter=stop - 1)
    assert n3 == stop - 1 and not same_bits(w, w3), "a run stopped one iteration early has the converged bits"
    tw, _, tn = solve_call(r["y"], np.zeros((R.TRANSFORM_ROWS, f["k"])), np.ascontiguousarray(r["h"].T), device, update_h=False, tol=f["tol"])
    assert tn == r["tn"] and np.abs(tw.cpu().numpy() - r["tw"]).max() <= R.fit_tolerance("loose")[2]


# ------------------------------------------------------------------------------------------------------------------ limits
def test_what_raises_on_the_device(device):
    x = to_dev(R.fixture_case("tiny")["x"], device)
    bad = x.clone()
    bad[17, 5] = -1e-3
    with pytest.raises(ValueError, match="negative values"):
        mmk.NMF(n_components=3)(bad)
    fitted = mmk.NMF(n_components=3).fit(x)
    with pytest.raises(ValueError, match="negative values"):
        fitted.transform(bad)
    with pytest.raises(ValueError, match="D = 33"):
        fitted.transform(x[:, :20])
    col = to_dev(np.random.default_rng(3).uniform(0.1, 1, (60, 1)).astype(np.float32), device)
    with pytest.raises(ValueError, match="exceeds the numerical rank.*arbitrary"):
        mmk.NMF(n_components=4)(torch.cat([col, col * 2, col * 3, col * 0.5], 1).contiguous())      # rank 1 up to the rounding of col * 3
    with pytest.raises(ValueError, match="exceeds the numerical rank"):
        mmk.NMF(n_components=2)(torch.zeros((30, 12), device=device))
    with pytest.raises(NotImplementedError, match=f"D = {native.NMF_MAX_D + 1}.*NMF_MAX_D"):
        mmk.NMF(n_components=2)(torch.zeros((3, native.NMF_MAX_D + 1), device=device))
    with pytest.raises(NotImplementedError, match=f"n_components = {native.NMF_MAX_COMPONENTS + 1}.*NMF_MAX_COMPONENTS"):
        mmk.NMF(n_components=native.NMF_MAX_COMPONENTS + 1)(torch.zeros((80, 80), device=device))
    with pytest.raises(TypeError):
        mmk.NMF(n_components=2)(torch.zeros((8, 4), dtype=torch.float64, device=device))
    with pytest.raises(RuntimeError):
        mmk.NMF(n_components=2)(torch.zeros((8, 4)))
    with pytest.raises(ValueError, match="contiguous"):
        native.nmf_w_half(x, torch.zeros((3, 96), dtype=torch.float64, device=device).t(), torch.zeros((33, 3), dtype=torch.float64, device=device))
    again = mmk.NMF(n_components=3)(x)                                           # (and the next call is a fresh one)
    assert torch.equal(again, mmk.NMF(n_components=3)(x))


# ------------------------------------------------------------------------------------------------------------------ the stream contract
def _tiny(seed):
    x = R.fixture_frames("tiny")[0]
    return x.copy() if seed == 0 else np.ascontiguousarray(x[::-1] * np.float32(0.5))


def _stream_fit():
    f = R.FIXTURES["tiny"]
    n, d, k = f["n"], f["d"], f["k"]

    def call(L, a, s):
        it = C.c_int32(0)
        rc = L.mmk_nmf_start_f64(S.P(a["x"]), d, n, d, k, S.P(a["w"]), S.P(a["ht"]), S.P(a["s"]), S.P(a["v"]), S.P(a["part"]), S.P(a["start"]),
                                 a["start"].numel(), s)
        return rc or L.mmk_nmf_solve_f64(S.P(a["x"]), d, n, d, k, S.P(a["w"]), S.P(a["ht"]), 1, f["tol"], f["max_iter"], 0, 1, C.byref(it), S.P(a["solve"]),
                                         a["solve"].numel(), s)

    return S.Case("mmk_nmf_solve_f64", lambda seed: dict(x=torch.from_numpy(_tiny(seed))),
                  lambda L, i: dict(w=((n, k), torch.float64), ht=((d, k), torch.float64), s=((k,), torch.float64), v=((k, d), torch.float64),
                                    part=((k,), torch.int32)),
                  call, tag="fit", work=lambda L, i: dict(start=L.mmk_nmf_start_workspace_bytes(n, d, k), solve=L.mmk_nmf_solve_workspace_bytes(n, d, k)))


def _stream_transform():
    f = R.FIXTURES["tiny"]
    m, d, k = R.TRANSFORM_ROWS, f["d"], f["k"]

    def build(seed):
        y = R.fixture_frames("tiny")[1]
        ht = np.ascontiguousarray(G["tiny_components"].T)
        return dict(y=torch.from_numpy(y.copy() if seed == 0 else np.ascontiguousarray(y[::-1] * np.float32(0.5))),
                    ht=torch.from_numpy(ht.copy() if seed == 0 else ht * 0.75), w0=torch.zeros((m, k), dtype=torch.float64))

    def call(L, a, s):
        it = C.c_int32(0)
        with torch.cuda.stream(torch.cuda.ExternalStream(s) if s else torch.cuda.default_stream()):
            a["w"].copy_(a["w0"], non_blocking=True)                              # sklearn's transform starts from zeros - on the call's stream
        return L.mmk_nmf_solve_f64(S.P(a["y"]), d, m, d, k, S.P(a["w"]), S.P(a["ht"]), 0, f["tol"], f["max_iter"], 0, 1, C.byref(it), S.P(a["solve"]),
                                   a["solve"].numel(), s)

    return S.Case("mmk_nmf_solve_f64", build, lambda L, i: dict(w=((m, k), torch.float64)), call, tag="transform",
                  work=lambda L, i: dict(solve=L.mmk_nmf_solve_workspace_bytes(m, d, k)))


STREAM_CASES = [_stream_fit(), _stream_transform()]


@pytest.mark.parametrize("case", STREAM_CASES, ids=[c.id for c in STREAM_CASES])
def test_fit_and_transform_behind_a_busy_side_stream(device, case):
    """tests/test_gpu_streams.py's method for entry points that may wait for their stream: the real input twice on the default stream (the
    same bits), the stale input once (other bits), then behind a delay and a late write of the input on a side stream: the
    default-stream bits.  (A launch that left its stream would have read the stale input.)"""
    bound = S.Bound(case, device)
    want, again = bound.run_default("real"), bound.run_default("real")
    assert not S.differs(want, again), (case.id, "two default-stream calls disagree")
    bound.check_surround(case.id + " on the default stream")
    assert S.differs(want, bound.run_default("stale")), (case.id, "the stale input gives the real outputs")
    got, busy, host = S.late_input(bound, S.side_stream(device))
    print(f"[streams] {case.id}: host time of the call {host * 1e3:.3f} ms, busy on return: {busy} (the call waits for its stream)")
    assert not S.differs(want, got), (case.id, "behind a late input on a side stream the outputs differ from the default-stream run")
    bound.check_surround(case.id + " on the side stream")
