"""float64 restatement, seeded fixtures and derived bounds of the PCA kernels (include/mmk.h: mmk_pca_colstats_f64, mmk_pca_cov_f64,
mmk_pca_eig_f64, mmk_pca_project_f32) and of mimikit_amd.PCA, shared by tests/test_pca_refs.py (CPU), tests/test_gpu_pca.py and
tests/golden/make_golden_pca.py.  numpy only; u = 2^-24 (fp32), v = 2^-53 (fp64).  Every bound is derived from the roundings the computation
makes, none is fitted to what the GPU returns.

The reference (mimikit/features/functionals.py:1114-1138) is sklearn's StandardScaler followed by sklearn's PCA; `pca64` restates it with
numpy's `eigh` on the full covariance:
    mu, var (ddof 0); scale = 1 where var <= N eps var + (N mu eps)^2 (sklearn's _is_constant_feature), sqrt(var) elsewhere
    z = (x - mu) / scale, re-centred by its own column mean m (sklearn's PCA.mean_); mean = mu + m scale is what the device stores
    C = z^T z / (N - 1); components = its leading eigenvectors, falling, each with its entry of largest magnitude positive
    (svd_flip(u_based_decision=False), sklearn >= 1.5); scores = z components^T

Statistics (N rows, any order of the fp64 sums: gamma_N <= N v sum|terms|).
    The device's mu_d = fl(sum x) / N is off by delta <= (N + 1) v mean|x|, and the mean of (x - mu_d) / scale IS (mu - mu_d) / scale, so the
    fold cancels delta: what is left is the rounding of that second mean, (N + 3) v mean|x - mu|, and the fma's v |mu|.  The restatement's own
    folded mean carries the same:                 mean_bound  = 2 ((N + 3) v mean|x - mu| + v |mu|)
    sum (x - mu_d)^2 = N var + N delta^2 (the cross term sums to 0), N + 3 roundings per unit of the sum, the division and the square root:
                                                  scale_bound = scale ((N + 6) v + (delta / scale)^2);   0 for a constant column (both sides 1)
Covariance.  z_d = (x - mean_d) / scale_d with two roundings differs from z by at most
    dz_ij = mean_bound_j / scale_j + |z_ij| (scale_bound_j / scale_j + 2 v)                                     (first order)
and the sum over N rows of products (rounded or fused), in whatever order the matrix unit adds them, and the division add (N + 3) v:
    cov_bound = (|z|^T dz + dz^T |z| + dz^T dz + (N + 3) v |z|^T |z|) / (N - 1),       |C_d - C|_2 <= |cov_bound|_F
Components, a posteriori (`check_components`).  The device stops when ITS residual |Y_k - theta_k Q_k|_2 <= TOL |C_d|_inf.  The residual of
the same vector against the restatement's C differs by (C - C_d) v and by the roundings of Z = C_d Q' (a sum of d terms per entry:
(d + 1) v |C|_inf per column, since | |C| |q| |_2 <= |C|_inf), of Y = Z W and Q = Q' W (sums of b terms against |Z|_F, |theta Q'|_F <=
sqrt(b) |C|_inf each) and of forming the residual (2 v |C|_inf):
    resid_allow = (TOL (|C|_inf + |cov_bound|_inf) + |cov_bound|_F + (d + 2 (b + 1) sqrt(b) + 5) v |C|_inf) (1 + 1e-9)
(the last factor: the vectors' length is 1 to about (d + b) v).  With r_k = C v_k - rho_k v_k for the Rayleigh quotient rho_k of the device's
vector (the theta that minimises |r|), Davis-Kahan gives sin(angle) <= |r_k|_2 / gap_k, gap_k = the distance from rho_k to the rest of the
restatement's spectrum, and two unit vectors with a positive inner product differ by 2 sin(angle / 2) <= sqrt(2) sin(angle):
    vec_bound_k = sqrt(2) |r_k|_2 / gap_k + NORM_SLACK,     NORM_SLACK = 8 (d + b) v for the length
`fixture_case` asserts for every fixture that each gap relied on is at least 1000 resid_allow and that the largest entry of each component
beats the second by 1000 times the a-priori vector bound sqrt(2) resid_allow / gap (so the sign cannot flip): choose another seed otherwise.
Null components.  Where the gap fails that test AND lambda_k <= 1000 resid_allow the component lies in what the solver sees as C's null
space (`deficient`, columns 6 to 8): no method that works from C can place the vector, and sklearn's own is arbitrary there.  Only the
size of the scores is bounded: sum_i s_ik^2 = (N - 1) v^T C v, the k-th Ritz value is at most lambda_k (Cauchy interlacing), so
    |s_ik| <= sqrt((N - 1) (max(lambda_k, 0) + 2 resid_allow)) + the projection terms below.
Scores.  One fp64 fma chain of d terms over z_d v_d, rounded to fp32 once:
    score_bound_ik = |z_i|_2 vec_bound_k + sum_j dz_ij a_jk + (d + 2) v sum_j |z_ij| a_jk + ulp32(|s_ik| + those) / 2,   a = |v| + vec_bound
"""
import functools

import numpy as np

U = 2.0 ** -24
V = 2.0 ** -53
EPS = 2.0 ** -52
TOL = 1e-12            # include/mmk.h: MMK_PCA_TOL
EXTRA = 16             # csrc/pca.hip: kPcExtra
MARGIN = 1000.0

# name -> (seed, N, D, rank of the latent (0: none), noise, n_components)
FIXTURES = {
    "tall": (101, 600, 40, 12, 0.1, 8),
    "wide": (102, 96, 200, 24, 0.1, 16),
    "full": (103, 300, 130, 20, 0.1, 16),
    "deficient": (104, 200, 40, 5, 0.0, 8),
    "iid": (105, 5000, 64, 0, 1.0, 8),
    "square": (106, 64, 12, 6, 0.1, 12),
    "big": (107, 6000, 513, 40, 0.1, 16),
}
GOLDEN = ("tall", "wide", "full", "deficient", "square")       # tests/golden/pca.npz (iid's scores alone would be 312 KiB)
DEFECTS = ("ddof1", "f32_mean_no_recentre", "u_sign", "stop_1e-6", "const_tiny_scale", "f32_accumulate")


def block_width(d, k):
    return min(d, k + EXTRA)


@functools.lru_cache(maxsize=None)
def fixture_frames(name):
    """low-rank latent times a mixing matrix, plus noise, times a per-column gain plus an offset, float32, read-only"""
    seed, n, d, rank, noise, _ = FIXTURES[name]
    rng = np.random.default_rng(seed)
    body = np.zeros((n, d))
    if rank:
        latent = rng.standard_normal((n, rank)) * 1.3 ** -np.arange(rank)
        body = latent @ rng.standard_normal((rank, d)) / np.sqrt(rank)
    if noise:
        body = body + noise * rng.standard_normal((n, d))
    gain, offset = np.exp(rng.uniform(-2, 2, d)), rng.uniform(-3, 3, d)
    x = (body * gain + offset).astype(np.float32)
    if name == "deficient":
        x[:, -3:] = 1.25
    x.setflags(write=False)
    return x


def sign_by_largest_entry(vecs):
    """(k, d) -> the same rows, each with its entry of largest magnitude (the first of equals) positive"""
    at = np.abs(vecs).argmax(1)
    return vecs * np.where(vecs[np.arange(vecs.shape[0]), at] < 0, -1.0, 1.0)[:, None]


def pca64(x, k, defect=None):
    """the restatement -> dict.  Defects: 'ddof1' (sample standard deviation), 'f32_mean_no_recentre' (the scaler's mean rounded to fp32,
    as a float32 StandardScaler leaves it, and no re-centring to repair it; 'f32_mean' alone is the same WITH re-centring), 'u_sign' (the
    sign by the largest score, sklearn < 1.5), 'const_tiny_scale' (a constant column divided by its sqrt(var))"""
    x64 = np.asarray(x, dtype=np.float64)
    n, d = x64.shape
    mu = x64.mean(0)
    if defect in ("f32_mean", "f32_mean_no_recentre"):
        mu = mu.astype(np.float32).astype(np.float64)
    var = ((x64 - mu) ** 2).mean(0) if defect in ("f32_mean", "f32_mean_no_recentre") else x64.var(0)
    const = var <= n * EPS * var + (n * mu * EPS) ** 2
    with np.errstate(invalid="ignore", divide="ignore"):
        scale = np.sqrt(var * (n / (n - 1.0) if defect == "ddof1" else 1.0))
        if defect != "const_tiny_scale":
            scale = np.where(const, 1.0, scale)
        z = (x64 - mu) / scale
    m = np.zeros(d) if defect == "f32_mean_no_recentre" else z.mean(0)
    z = z - m
    c = z.T @ z / (n - 1)
    c = 0.5 * (c + c.T)
    if not np.isfinite(c).all():
        nan = np.full((n, k), np.nan)
        return dict(n=n, d=d, k=k, x64=x64, mu=mu, scale=scale, const=const, mean=mu + m * scale, z=z, c=c, scores=nan)
    evals, evecs = np.linalg.eigh(c)
    evals, evecs = evals[::-1].copy(), evecs[:, ::-1].T.copy()
    comps = sign_by_largest_entry(evecs[:k])
    scores = z @ comps.T
    if defect == "u_sign":
        flip = np.where(scores[np.abs(scores).argmax(0), np.arange(k)] < 0, -1.0, 1.0)
        comps, scores = comps * flip[:, None], scores * flip
    return dict(n=n, d=d, k=k, x64=x64, mu=mu, var=var, scale=scale, const=const, mean=mu + m * scale, z=z, c=c, evals=evals, comps=comps,
                scores=scores)


# ---------------------------------------------------------------------------------------------------------------- bounds
def stats_bounds(p):
    n, x64, mu, scale = p["n"], p["x64"], p["mu"], p["scale"]
    mean_bound = 2 * ((n + 3) * V * np.abs(x64 - mu).mean(0) + V * np.abs(mu))
    delta = (n + 1) * V * np.abs(x64).mean(0)
    scale_bound = np.where(p["const"], 0.0, scale * ((n + 6) * V + (delta / scale) ** 2))
    return mean_bound, scale_bound


def z_bound(p):
    mean_bound, scale_bound = stats_bounds(p)
    return mean_bound / p["scale"] + np.abs(p["z"]) * (scale_bound / p["scale"] + 2 * V)


def cov_bound(p):
    n, a, dz = p["n"], np.abs(p["z"]), z_bound(p)
    cross = a.T @ dz
    return (cross + cross.T + dz.T @ dz + (n + 3) * V * (a.T @ a)) / (n - 1)


def resid_allow(p, e=None):
    e = cov_bound(p) if e is None else e
    d, b = p["d"], block_width(p["d"], p["k"])
    cinf = np.abs(p["c"]).sum(1).max()
    return (TOL * (cinf + e.sum(1).max()) + np.sqrt((e ** 2).sum()) + (d + 2 * (b + 1) * np.sqrt(b) + 5) * V * cinf) * (1 + 1e-9)


def norm_slack(p):
    return 8 * (p["d"] + block_width(p["d"], p["k"])) * V


def gaps(theta, evals):
    """theta (k,) at the places 0 .. k - 1 of the falling spectrum evals -> the distance of each to every OTHER eigenvalue"""
    dist = np.abs(theta[:, None] - evals[None, :])
    dist[np.arange(theta.shape[0]), np.arange(theta.shape[0])] = np.inf
    return dist.min(1)


def null_columns(p, allow):
    """the regime rule: a component whose gap is not MARGIN allowances wide and whose eigenvalue is at most MARGIN allowances"""
    k = p["k"]
    return (gaps(p["evals"][:k], p["evals"]) < MARGIN * allow) & (p["evals"][:k] <= MARGIN * allow)


def check_components(p, comps, what, allow=None):
    """the a posteriori test of (k, d) vectors against the restatement p -> dict(null, resid, allow, vec_err, vec_bound, worst): asserts
    |r_k| <= resid_allow for every k and |v_k - v_k_ref| <= vec_bound_k outside the null regime"""
    comps = np.asarray(comps, dtype=np.float64)
    k = p["k"]
    allow = resid_allow(p) if allow is None else allow
    null = null_columns(p, allow)
    cv = comps @ p["c"]
    rho = (cv * comps).sum(1) / (comps * comps).sum(1)
    resid = np.sqrt(((cv - rho[:, None] * comps) ** 2).sum(1))
    assert np.isfinite(resid).all() and (resid <= allow).all(), \
        f"{what}: residual {resid.max():.3e} of component {int(resid.argmax())} above the allowance {allow:.3e}"
    length = np.sqrt((comps * comps).sum(1))
    assert (np.abs(length - 1) <= norm_slack(p)).all(), f"{what}: a component's length is off by {np.abs(length - 1).max():.3e}"
    gap = gaps(rho, p["evals"])
    vec_bound = np.sqrt(2) * resid / gap + norm_slack(p)
    vec_err = np.sqrt(((comps - p["comps"]) ** 2).sum(1))
    bad = ~null & ~(vec_err <= vec_bound)
    assert not bad.any(), f"{what}: component {int(np.nonzero(bad)[0][0])} is {vec_err[bad][0]:.3e} from the restatement's, bound {vec_bound[bad][0]:.3e}"
    worst = max((resid / allow).max(), (vec_err[~null] / vec_bound[~null]).max() if (~null).any() else 0.0)
    return dict(null=null, resid=resid, allow=allow, vec_err=vec_err, vec_bound=np.where(null, np.inf, vec_bound), worst=float(worst))


def score_bound(p, vec_bound, null, allow, z=None, scores=None):
    """(rows, k) bound on |device score - restatement score|; in a null column on |device score| itself (compare those against 0).
    z, scores: other rows than the fitted ones (transform of new frames), standardised with the restatement's statistics"""
    z = p["z"] if z is None else z
    scores = p["scores"] if scores is None else scores
    mean_bound, scale_bound = stats_bounds(p)
    dz = mean_bound / p["scale"] + np.abs(z) * (scale_bound / p["scale"] + 2 * V)
    d, n, k = p["d"], p["n"], p["k"]
    znorm = np.sqrt((z * z).sum(1))[:, None]
    vb = np.where(null, 0.0, vec_bound)
    a = np.abs(p["comps"]).T + vb[None, :]                                    # (d, k)
    regular = znorm * vb[None, :] + dz @ a + (d + 2) * V * (np.abs(z) @ a)
    size = np.sqrt((n - 1) * (np.maximum(p["evals"][:k], 0) + 2 * allow))[None, :] + np.sqrt((dz * dz).sum(1))[:, None] + (d + 2) * V * znorm
    wide = np.where(null[None, :], size, regular)
    mag = np.where(null[None, :], 0.0, np.abs(scores)) + wide
    return wide + 0.5 * np.spacing(mag.astype(np.float32)).astype(np.float64)


def score_target(p, null, scores=None):
    """what a device score is compared with: the restatement's, 0 in a null column"""
    scores = p["scores"] if scores is None else scores
    return np.where(null[None, :], 0.0, scores)


# ---------------------------------------------------------------------------------------------------------------- the iteration, in numpy
def start_block(d, b):
    """csrc/pca.hip: pca_start_kernel, bit for bit"""
    h = (np.arange(d * b, dtype=np.uint64) * 0x9E3779B9 + 0x7F4A7C15) & 0xFFFFFFFF
    h ^= h >> 16
    h = (h * 0x85EBCA6B) & 0xFFFFFFFF
    h ^= h >> 13
    h = (h * 0xC2B2AE35) & 0xFFFFFFFF
    h ^= h >> 16
    return ((h >> 8).astype(np.float64) / 8388608.0 - 1.0).reshape(d, b)


def subspace64(c, k, tol=TOL, max_iter=4000):
    """the device's block subspace iteration in float64 numpy (LAPACK's Householder QR and eigh in place of the kernels' own) ->
    (components (k, d) with the sign rule, theta (k,), iterations)"""
    d = c.shape[0]
    b = block_width(d, k)
    cinf = np.abs(c).sum(1).max()
    y = start_block(d, b)
    for it in range(1, max_iter + 1):
        qp = np.linalg.qr(y)[0]
        z = c @ qp
        h = qp.T @ z
        theta, w = np.linalg.eigh(0.5 * (h + h.T))
        theta, w = theta[::-1], w[:, ::-1]
        q, y = qp @ w, z @ w
        if np.sqrt(((y[:, :k] - theta[:k] * q[:, :k]) ** 2).sum(0)).max() <= tol * cinf:
            return sign_by_largest_entry(q[:, :k].T), theta[:k].copy(), it
    raise RuntimeError(f"subspace64: no convergence in {max_iter} iterations")


def project_chain(z, comps, dtype=np.float64):
    """csrc/pca.hip: pca_project_kernel's accumulation - one chain over rising column per (row, component) in `dtype`, rounded to fp32"""
    z, comps = z.astype(dtype), comps.astype(dtype)
    acc = np.zeros((z.shape[0], comps.shape[0]), dtype=dtype)
    for j in range(z.shape[1]):
        acc = acc + z[:, j:j + 1] * comps[None, :, j]
    return acc.astype(np.float32)


# ---------------------------------------------------------------------------------------------------------------- cases
@functools.lru_cache(maxsize=None)
def fixture_case(name):
    """-> (x, p, cov bound e, allow, null, margins): the restatement of a fixture, computed once and shared, with the margins the bounds rely
    on asserted: every relied-on gap >= MARGIN allow, every component's largest entry ahead of the second by MARGIN a-priori vector bounds"""
    x = fixture_frames(name)
    k = FIXTURES[name][5]
    p = pca64(x, k)
    e = cov_bound(p)
    allow = resid_allow(p, e)
    null = null_columns(p, allow)
    gap = gaps(p["evals"][:k], p["evals"])
    assert (gap[~null] >= MARGIN * allow).all(), f"{name}: gap {gap[~null].min():.3e} < {MARGIN} allowances of {allow:.3e}: another seed"
    apriori = np.sqrt(2) * allow / gap + norm_slack(p)
    top2 = np.sort(np.abs(p["comps"]), axis=1)[:, -2:]
    lead = top2[:, 1] - top2[:, 0]
    assert (lead[~null] >= MARGIN * apriori[~null]).all(), f"{name}: a component's two largest entries are {lead[~null].min():.3e} apart: another seed"
    margins = dict(gap=float((gap[~null] / allow).min()), lead=float((lead[~null] / apriori[~null]).min()), null=int(null.sum()))
    for v in p.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    e.setflags(write=False)
    return x, p, e, allow, null, margins


def layout_case():
    """48 x 35 integers in [-8, 8]: with mean 0 and scale 1 every product and sum of the covariance is exact in fp64"""
    x = np.random.default_rng(4835).integers(-8, 9, (48, 35)).astype(np.float32)
    x64 = x.astype(np.float64)
    return x, (x64.T @ x64) / 47.0
