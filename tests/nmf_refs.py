"""float64 restatement, seeded fixtures and bounds of the NMF kernels (include/mmk_nmf.h) and of mimikit_amd.NMF, shared by
tests/test_nmf_refs.py (CPU), tests/test_gpu_nmf.py and tests/golden/make_golden_nmf.py.  numpy only; v = 2^-53.

The reference (mimikit/features/functionals.py:1141-1170) is sklearn.decomposition.NMF with its defaults: init=None -> "nndsvda" (for
n_components <= min(N, D)), solver "cd", Frobenius loss, no regularisation, no shuffle.  The restatement:

    start64      _initialize_nmf from a top-k SVD - numpy.linalg.svd of X, or the Gram route the device takes (exact eigenpairs of X^T X,
                 S = sqrt(lambda), u = X v / S).  NNDSVD does not see the sign of a singular pair, so the two agree to rounding.
    sweep64      one half-sweep of _update_cdnmf_fast, all rows at once (the rows are independent, the columns sequential)
    fit64        _fit_coordinate_descent: W half, H half, violation / violation_init <= tol
    transform64  the same with H fixed and W started at zeros (sklearn's start for the cd solver)

Conditions under which sklearn itself can be pinned, asserted by `fixture_case` for every fixture:
    - the relative margin |m_p - m_n| / max(m_p, m_n) of the part choice is at least 1e-6 for every j >= 1;
    - no start entry lies within a factor 1 +- 1e-6 of the 1e-6 cut;
    - the violation ratio at the stopping iteration and at the one before are each at least 0.5 % away from tol (fixtures that stop by
      count - tol = 0 or the cap - are exempt).
Frames without a spectral gap (iid noise, spectra of white noise) give nothing to pin: sklearn's own results at two seeds differ by order 1.

Half-sweep bound (`sweep_bound`), derived, one-sided, then doubled because the restatement's own products round too.  With P = X B (a sum
of L terms per entry) and G = B^T B:
    eP = (L + 2) v |X| |B|,   eG = (L + 2) v |B|^T |B|                              (any order of the sum)
    column t:  dg = eP[:,t] + sum_r (eG[t,r] (|a_r| + da_r) + |G[t,r]| da_r) + (k + 2) v (|P[:,t]| + sum_r |G[t,r]| |a_r|)
               da_t = dg / h_lo + |g| eG[t,t] / (h h_lo) + 3 v (|a_t| + |g| / h),   h = G[t,t], h_lo = h - eG[t,t]
    (da_r = 0 for the columns r >= t not yet updated: both sides got the same bits; max(., 0) and min(0, .) are 1-Lipschitz; a column of
    B of exact zeros has h = 0 on both sides and leaves a_t as it is.)
    violation: sum of dg + (rows k + 2) v sum |pg|.

Start bound (`start_bound`), a posteriori from the device's vectors as pca_refs.check_components does: r_j = G v_j - rho_j v_j against the
restatement's G, Davis-Kahan sin <= |r_j| / gap_j, |v_j - v_ref| <= sqrt(2) |r_j| / gap_j + 8 (D + k) v =: ev_j; the rest is first-order
propagation through u = X v / S, the part norms (1-Lipschitz), lbd = sqrt(S m) and the product, each with its roundings.

Whole fit.  200 nonlinear iterations have no derived bound; the tolerance is measured against the reference, never against the code under
test: `spread` is the largest difference between float64 restatements whose products are summed in BLAS order, in reversed order and in
longdouble; the tolerance of an array (W, components_, the transform's W) is the fp32 half ulp of its largest entry plus 1000 of its
spreads (the device's blocked order differs from all three and the loop amplified a perturbation up to 10-fold; the half ulp also
carries what the device's eigen step, stopped at a residual of 1e-12 |G|_inf, leaves in the start); tests/test_nmf_refs.py asserts that 1000 spreads stay below 1e-6 of the largest
entry, so the tolerance cannot hide a wrong rule.
"""
import functools
import os

import numpy as np

V = 2.0 ** -53
EPS_CUT = 1e-6           # include/mmk_nmf.h: MMK_NMF_EPS
PCA_TOL = 1e-12          # include/mmk.h: MMK_PCA_TOL
RANK_MARGIN = 64.0       # include/mmk_nmf.h: MMK_NMF_RANK_MARGIN
SPREAD_FACTOR = 1000.0

# name -> dict(seed, n, d, k, tol, max_iter, rank (templates), noise)
FIXTURES = {
    "tiny": dict(seed=210, n=96, d=33, k=3, tol=1e-4, max_iter=200, rank=3, noise=1e-3),
    "k1": dict(seed=201, n=50, d=33, k=1, tol=0.0, max_iter=6, rank=2, noise=1e-3),
    "wide": dict(seed=202, n=70, d=129, k=5, tol=1e-4, max_iter=200, rank=5, noise=1e-3),
    "loose": dict(seed=201, n=257, d=65, k=6, tol=1e-2, max_iter=200, rank=6, noise=1e-3),
    "cap": dict(seed=201, n=200, d=65, k=6, tol=1e-4, max_iter=7, rank=6, noise=1e-3),
    "odd": dict(seed=203, n=131, d=67, k=7, tol=1e-3, max_iter=200, rank=7, noise=1e-3),
    "k16": dict(seed=203, n=150, d=80, k=16, tol=1e-4, max_iter=200, rank=16, noise=1e-4),
    "k64": dict(seed=202, n=200, d=96, k=64, tol=1e-3, max_iter=200, rank=64, noise=1e-4),
    "silent": dict(seed=201, n=120, d=40, k=4, tol=1e-4, max_iter=200, rank=4, noise=1e-3),
    "runs": dict(seed=209, n=1500, d=257, k=12, tol=1e-4, max_iter=200, rank=12, noise=1e-3),
}
NAMES = tuple(FIXTURES)
BY_COUNT = ("k1", "cap")           # stop by count: exempt from the ratio condition
TRANSFORM_ROWS = 40
GOLDEN_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "nmf.npz")


def _templates(rng, rank, d):
    """spectral templates: a partial of its own per template and a weaker second one half the bins away"""
    bins = np.arange(d)
    t = np.zeros((rank, d))
    for r in range(rank):
        c = (r + 0.5) * d / rank
        t[r] = (np.exp(-0.5 * ((bins - c) / (0.25 * d / rank + 0.5)) ** 2)
                + 0.3 * np.exp(-0.5 * ((bins - (c + d / 2) % d) / (0.15 * d / rank + 0.5)) ** 2))
    return t


def _activations(rng, n, rank):
    """smooth and non-negative: three notes (Gaussian bumps in time) per template"""
    time = np.arange(n)[:, None]
    a = np.zeros((n, rank))
    for _ in range(3):
        a += rng.uniform(0.3, 1.0, rank) * np.exp(-0.5 * ((time - rng.uniform(0, n, rank)) / (0.3 * n / rank)) ** 2)
    return a


@functools.lru_cache(maxsize=None)
def fixture_frames(name):
    """(x (n, d), y (40, d)) float32, read-only: templates times activations times falling gains, plus small non-negative noise.  The
    seeds are the first from 201 on at which the conditions of the module text hold, the fixture stops by tol where it is meant to, and
    sklearn's own results at three seeds agree to 1e-10 (make_golden_nmf.py asserts it; k16 needed the smaller noise for that)"""
    f = FIXTURES[name]
    rng = np.random.default_rng(f["seed"])
    n, d, rank = f["n"], f["d"], f["rank"]
    if name == "k64":                                            # rank 64 on 96 bins: sparse random templates and activations
        temp = rng.uniform(0, 1, (rank, d)) * (rng.uniform(0, 1, (rank, d)) < 0.25)
        gains = np.ones(rank)
        act = rng.uniform(0, 1, (n + TRANSFORM_ROWS, rank)) * (rng.uniform(0, 1, (n + TRANSFORM_ROWS, rank)) < 0.3)
    else:
        temp = _templates(rng, rank, d)
        gains = 1.3 ** -np.arange(rank)
        act = _activations(rng, n + TRANSFORM_ROWS, rank)
        act = act[rng.permutation(n + TRANSFORM_ROWS)]          # (so that the unseen batch is drawn from the same notes)
    body = (act * gains) @ temp
    body = body + f["noise"] * np.abs(rng.standard_normal(body.shape)) * body.max()
    if name == "silent":
        rows = rng.choice(n, 16, replace=False)
        body[rows[:10]] = 0.0
        body[rows[10:]] *= 1e-7                                   # six nearly silent frames: start entries between machine epsilon and the cut
        body[:, rng.choice(d, 3, replace=False)] = 0.0
    x = body.astype(np.float32)
    x, y = x[:n].copy(), x[n:].copy()
    x.setflags(write=False)
    y.setflags(write=False)
    return x, y


# ------------------------------------------------------------------------------------------------------------------ the start
def topk_svd(x64, k, route):
    """(S (k,), U (n, k), Vt (k, d)).  route 'svd': numpy.linalg.svd;  'gram': exact eigenpairs of X^T X, S = sqrt(lambda), u = X v / S"""
    if route == "svd":
        u, s, vt = np.linalg.svd(x64, full_matrices=False)
        return s[:k].copy(), u[:, :k].copy(), vt[:k].copy()
    g = x64.T @ x64
    lam, vec = np.linalg.eigh(0.5 * (g + g.T))
    lam, vec = lam[::-1][:k], vec[:, ::-1][:, :k]
    s = np.sqrt(np.maximum(lam, 0.0))
    return s, (x64 @ vec) / s, vec.T.copy()


def nndsvda(x64, s, u, vt, eps=EPS_CUT, ge=False):
    """sklearn's _initialize_nmf(init='nndsvda') from a top-k SVD -> dict(w (n, k), ht (d, k), part (k,), margin (k,), raw_w, raw_ht).
    Defects: eps (the cut, e.g. machine epsilon), ge (>= for > in the choice of part)"""
    k = s.shape[0]
    w, h = np.zeros_like(u), np.zeros_like(vt)
    w[:, 0] = np.sqrt(s[0]) * np.abs(u[:, 0])
    h[0] = np.sqrt(s[0]) * np.abs(vt[0])
    part, margin = np.full(k, 2, dtype=np.int32), np.full(k, np.inf)
    for j in range(1, k):
        x, y = u[:, j], vt[j]
        x_p, y_p = np.maximum(x, 0), np.maximum(y, 0)
        x_n, y_n = np.abs(np.minimum(x, 0)), np.abs(np.minimum(y, 0))
        x_p_nrm, y_p_nrm = np.sqrt(x_p @ x_p), np.sqrt(y_p @ y_p)
        x_n_nrm, y_n_nrm = np.sqrt(x_n @ x_n), np.sqrt(y_n @ y_n)
        m_p, m_n = x_p_nrm * y_p_nrm, x_n_nrm * y_n_nrm
        pos = m_p >= m_n if ge else m_p > m_n
        if pos:
            uu, vv, sigma = x_p / x_p_nrm, y_p / y_p_nrm, m_p
        else:
            uu, vv, sigma = x_n / x_n_nrm, y_n / y_n_nrm, m_n
        lbd = np.sqrt(s[j] * sigma)
        w[:, j], h[j] = lbd * uu, lbd * vv
        part[j], margin[j] = int(pos), abs(m_p - m_n) / max(m_p, m_n)
    raw_w, raw_ht = w.copy(), h.T.copy()
    w[w < eps] = 0
    h[h < eps] = 0
    avg = x64.mean()
    w[w == 0] = avg
    h[h == 0] = avg
    return dict(w=w, ht=np.ascontiguousarray(h.T), part=part, margin=margin, raw_w=raw_w, raw_ht=raw_ht, avg=avg)


def start64(x, k, route="gram", eps=EPS_CUT, ge=False):
    x64 = np.asarray(x, dtype=np.float64)
    s, u, vt = topk_svd(x64, k, route)
    out = nndsvda(x64, s, u, vt, eps, ge)
    out.update(s=s, u=u, vt=vt)
    return out


# ------------------------------------------------------------------------------------------------------------------ the loop
def product(a, b, order="blas"):
    """a @ b with the sum over the inner index in BLAS order, in reversed order, or in longdouble"""
    if order == "blas":
        return a @ b
    if order == "reversed":
        return np.ascontiguousarray(a[:, ::-1]) @ np.ascontiguousarray(b[::-1])
    return (a.astype(np.longdouble) @ b.astype(np.longdouble)).astype(np.float64)


def sweep64(p, g, a, jacobi=False, project=True):
    """one half-sweep on all rows: p = X B (rows, k), g = B^T B (k, k), a (rows, k) updated IN PLACE; returns the violation.
    Defects: jacobi (every column updated from the old a), project=False (the violation without the a == 0 projection)"""
    k = a.shape[1]
    old = a.copy() if jacobi else a
    viol = 0.0
    for t in range(k):
        grad = -p[:, t] + old @ g[t]
        pg = np.where(a[:, t] == 0, np.minimum(0.0, grad), grad) if project else grad
        viol += np.abs(pg).sum()
        if g[t, t] != 0:
            a[:, t] = np.maximum(a[:, t] - grad / g[t, t], 0.0)
    return viol


def w_half64(x64, w, ht, order="blas", **kw):
    return sweep64(product(x64, ht, order), product(ht.T, ht, order), w, **kw)


def h_half64(x64, w, ht, order="blas", **kw):
    return sweep64(product(x64.T, w, order), product(w.T, w, order), ht, **kw)


def solve64(x64, w, ht, tol, max_iter, update_h=True, order="blas", **kw):
    """_fit_coordinate_descent, (w, ht) IN PLACE -> (n_iter, the violation ratios of every iteration)"""
    ratios, first, n_iter = [], 0.0, max_iter
    for it in range(1, max_iter + 1):
        viol = w_half64(x64, w, ht, order, **kw)
        if update_h:
            viol += h_half64(x64, w, ht, order, **kw)
        if it == 1:
            first = viol
        if first == 0:
            ratios.append(0.0)
            n_iter = it
            break
        ratios.append(viol / first)
        if viol / first <= tol:
            n_iter = it
            break
    return n_iter, ratios


def fit64(x, k, tol, max_iter, route="gram", order="blas", eps=EPS_CUT, ge=False, **kw):
    """-> dict(w (n, k), h (k, d), n_iter, ratios, start)"""
    x64 = np.asarray(x, dtype=np.float64)
    st = start64(x64, k, route, eps, ge)
    w, ht = st["w"].copy(), st["ht"].copy()
    n_iter, ratios = solve64(x64, w, ht, tol, max_iter, True, order, **kw)
    return dict(w=w, h=np.ascontiguousarray(ht.T), n_iter=n_iter, ratios=ratios, start=st)


def transform64(y, h, tol, max_iter, w0="zeros", order="blas"):
    """sklearn's transform: H fixed, W from zeros (defect 'sqrt': from sqrt(mean / k), the start of the mu solver) -> (w, n_iter)"""
    y64 = np.asarray(y, dtype=np.float64)
    k = h.shape[0]
    w = np.zeros((y64.shape[0], k)) if w0 == "zeros" else np.full((y64.shape[0], k), np.sqrt(y64.mean() / k))
    n_iter, _ = solve64(y64, w, np.ascontiguousarray(h.T), tol, max_iter, False, order)
    return w, n_iter


# ------------------------------------------------------------------------------------------------------------------ fixtures with their conditions
@functools.lru_cache(maxsize=None)
def fixture_case(name):
    """the restatement's fit and transform of a fixture, with the conditions of the module text asserted"""
    f = FIXTURES[name]
    x, y = fixture_frames(name)
    assert x.min() >= 0 and x.shape == (f["n"], f["d"])
    r = fit64(x, f["k"], f["tol"], f["max_iter"])
    st = r["start"]
    assert (st["margin"][1:] >= 1e-6).all(), f"{name}: a part choice has a margin of {st['margin'][1:].min():.2e}"
    for raw in (st["raw_w"], st["raw_ht"]):
        near = np.abs(raw / EPS_CUT - 1.0) <= 1e-6
        assert not near.any(), f"{name}: {int(near.sum())} start entries lie at the 1e-6 cut"
    if name not in BY_COUNT:
        assert r["n_iter"] < f["max_iter"], f"{name}: stopped by the cap"
        last = r["ratios"][-2:]
        assert all(abs(q / f["tol"] - 1.0) >= 5e-3 for q in last), f"{name}: a violation ratio {last} is within 0.5 % of tol {f['tol']}"
    else:
        assert r["n_iter"] == f["max_iter"], f"{name}: did not stop by count"
    lam = np.linalg.eigvalsh(x.astype(np.float64).T @ x.astype(np.float64))[::-1]
    thr = RANK_MARGIN * ((f["n"] + 2) * V + PCA_TOL * np.sqrt(f["d"])) * lam[0]
    assert lam[f["k"] - 1] > 100 * thr, f"{name}: eigenvalue {f['k'] - 1} is {lam[f['k'] - 1]:.2e}, the rank test's threshold {thr:.2e}"
    tw, tn = transform64(y, r["h"], f["tol"], f["max_iter"])
    r.update(x=x, y=y, tw=tw, tn=tn, f=f)
    return r


@functools.lru_cache(maxsize=None)
def spread(name):
    """(spread of W, spread of H, spread of the transform's W): the largest difference of the restatement under re-ordered sums"""
    r = fixture_case(name)
    f = r["f"]
    sw = sh = stw = 0.0
    for order in ("reversed", "longdouble"):
        o = fit64(r["x"], f["k"], f["tol"], f["max_iter"], order=order)
        assert o["n_iter"] == r["n_iter"], f"{name}: the {order} sums stop at {o['n_iter']}, BLAS order at {r['n_iter']}"
        sw, sh = max(sw, np.abs(o["w"] - r["w"]).max()), max(sh, np.abs(o["h"] - r["h"]).max())
        tw, tn = transform64(r["y"], r["h"], f["tol"], f["max_iter"], order=order)
        assert tn == r["tn"]
        stw = max(stw, np.abs(tw - r["tw"]).max())
    return sw, sh, stw


def half_ulp32(top):
    return float(np.spacing(np.float32(top))) / 2


def fit_tolerance(name):
    """(tolerance of W, of components_, of the transform's W): per array, the fp32 half ulp of its largest entry plus 1000 spreads"""
    r = fixture_case(name)
    return tuple(half_ulp32(np.abs(r[key]).max()) + SPREAD_FACTOR * s for key, s in zip(("w", "h", "tw"), spread(name)))


def golden():
    return np.load(GOLDEN_PATH)


# ------------------------------------------------------------------------------------------------------------------ the half-sweep's bound
def sweep_bound(xa, b, a_old, length):
    """bound of (a_new, violation) of one half-sweep of a_old (rows, k) against B (length, k), xa = |X| or |X^T| (rows, length)"""
    k = a_old.shape[1]
    p, g = xa @ b, b.T @ b                                     # (x >= 0: |X| = X)
    ep, eg = (length + 2) * V * (xa @ np.abs(b)), (length + 2) * V * (np.abs(b).T @ np.abs(b))
    a, da = a_old.copy(), np.zeros_like(a_old)
    dviol, sum_pg = 0.0, 0.0
    for t in range(k):
        grad = -p[:, t] + a @ g[t]
        dg = ep[:, t] + (np.abs(a) + da) @ eg[t] + da @ np.abs(g[t]) + (k + 2) * V * (np.abs(p[:, t]) + np.abs(a) @ np.abs(g[t]))
        pg = np.where(a[:, t] == 0, np.minimum(0.0, grad), grad)
        dviol += dg.sum()
        sum_pg += np.abs(pg).sum()
        h = g[t, t]
        if not b[:, t].any():                                    # a column of exact zeros: h = 0 on both sides, nothing is updated
            continue
        assert h > 2 * eg[t, t], "a nearly zero column of B: the h != 0 test is not covered by the bound"
        h_lo = h - eg[t, t]
        da[:, t] = dg / h_lo + np.abs(grad) * eg[t, t] / (h * h_lo) + 3 * V * (np.abs(a[:, t]) + np.abs(grad) / h)
        a[:, t] = np.maximum(a[:, t] - grad / h, 0.0)
    return 2 * da, 2 * (dviol + (a.size + 2) * V * sum_pg)


def sweep_inputs(name, iters=2):
    """(x, w, ht) float64 after `iters` iterations of the restatement: factors with exact zeros in them, the given state of a half-sweep"""
    r = fixture_case(name)
    x64 = r["x"].astype(np.float64)
    w, ht = r["start"]["w"].copy(), r["start"]["ht"].copy()
    solve64(x64, w, ht, 0.0, iters)
    return x64, w, ht


# ------------------------------------------------------------------------------------------------------------------ the start's bound
def start_bound(x, k, v_dev):
    """a posteriori, from the device's right singular vectors v_dev (k, d) -> dict(dw (n, k), dht (d, k), part (k,) expected, worst gap ratio).
    The restatement's own start carries errors of the same kind from numpy's eigh (its residual is at rounding level, included by
    doubling the rounding terms)."""
    x64 = np.asarray(x, dtype=np.float64)
    n, d = x64.shape
    g = x64.T @ x64
    lam_all = np.linalg.eigvalsh(0.5 * (g + g.T))[::-1]
    st = start64(x64, k, "gram")
    s, u, vt = st["s"], st["u"], st["vt"]
    sign = np.where((v_dev * vt).sum(1) < 0, -1.0, 1.0)
    va = v_dev * sign[:, None]
    rows = np.sqrt((x64 * x64).sum(1))
    dw, dht = np.zeros((n, k)), np.zeros((d, k))
    part = st["part"].copy()
    round_g = 2 * (n + 2) * V * lam_all[0]
    for j in range(k):
        rho = va[j] @ g @ va[j]
        res = np.sqrt(((g @ va[j] - rho * va[j]) ** 2).sum()) + round_g
        others = np.delete(lam_all, j)
        gap = np.abs(others - rho).min()
        assert gap > 100 * res, f"column {j}: gap {gap:.3e} against a residual of {res:.3e}"
        ev = np.sqrt(2) * res / gap + 8 * (d + k) * V
        ds = (res + round_g) / s[j]                                            # |s_dev^2 - lambda| <= res (+ the Ritz value's rounding)
        du = (rows * ev + 2 * (d + 2) * V * (x64 @ np.abs(va[j]))) / s[j] + np.abs(u[:, j]) * (ds / s[j] + 4 * V)
        dv = np.full(d, ev)
        if j == 0:
            dw[:, 0] = ds / np.sqrt(s[0]) * np.abs(u[:, 0]) + np.sqrt(s[0]) * du + 4 * V * st["raw_w"][:, 0]
            dht[:, 0] = ds / np.sqrt(s[0]) * np.abs(vt[0]) + np.sqrt(s[0]) * dv + 4 * V * st["raw_ht"][:, 0]
            continue
        pos = bool(st["part"][j])
        up, vp = (np.maximum(u[:, j], 0), np.maximum(vt[j], 0)) if pos else (np.abs(np.minimum(u[:, j], 0)), np.abs(np.minimum(vt[j], 0)))
        xn, yn = np.sqrt(up @ up), np.sqrt(vp @ vp)
        dxn, dyn = np.sqrt(du @ du) + 2 * (n + 2) * V * xn, np.sqrt(dv @ dv) + 2 * (d + 2) * V * yn
        m = xn * yn
        dm = xn * dyn + yn * dxn + dxn * dyn + 2 * V * m
        lbd = np.sqrt(s[j] * m)
        dl = (ds * m + s[j] * dm + ds * dm) / lbd + 2 * V * lbd
        dw[:, j] = dl * up / xn + (lbd + dl) * (du / xn + up * dxn / (xn * (xn - dxn))) + 6 * V * st["raw_w"][:, j]
        dht[:, j] = dl * vp / yn + (lbd + dl) * (dv / yn + vp * dyn / (yn * (yn - dyn))) + 6 * V * st["raw_ht"][:, j]
        part[j] = int(pos) if sign[j] > 0 else 1 - int(pos)                    # a negated pair swaps the names of its parts
    davg = 2 * (n * d + 2) * V * st["avg"]
    for raw, bound in ((st["raw_w"], dw), (st["raw_ht"], dht)):
        near = np.abs(raw - EPS_CUT) <= bound                                  # may fall on either side of the cut: raw or the mean
        bound[raw < EPS_CUT] = davg
        bound[near] = np.maximum(bound[near], st["avg"] + raw[near]) + davg
    return dict(dw=dw, dht=dht, part=part, start=st)
