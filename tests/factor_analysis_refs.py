"""float64 restatement, seeded fixtures and bounds of the factor analysis kernels (include/mmk_factor_analysis.h) and of
mimikit_amd.FactorAnalysis, shared by tests/test_factor_analysis_refs.py (CPU), tests/test_gpu_factor_analysis.py and
tests/golden/make_golden_factor_analysis.py.  numpy only.

The reference (mimikit/features/functionals.py:1173-1203) is sklearn.decomposition.FactorAnalysis with its defaults (the randomised SVD).
The restatement, `fa64`, is sklearn 1.7's _factor_analysis.py in Gram form: per EM step sklearn takes the k leading singular values s and
right vectors of Xc / (sqrt(psi) sqrt(N)); s^2 and the vectors are the k leading eigenpairs of G = C / sp_r / sp_c with C = Xc^T Xc / N and
sp = sqrt(psi) + 1e-12, and the unexplained variance is trace G - sum s^2.  The frames enter through C alone.

Conditions under which the EM loop can be pinned, asserted by tests/test_factor_analysis_refs.py at every EM step of every fixture:
    - the relative gap (theta_k - theta_{k+1}) / theta_1 is at least GAP_MIN = 1e-2 (the device's eigen step stops at a residual of
      1e-12 |G|_inf; over that gap a vector is off by 1e-10 at most; with a margin of 10: FIT_TOL = 1e-9 of an array's largest magnitude);
    - |ll_i - ll_{i-1} - tol| is at least STOP_MARGIN = 1e-4 while |ll| <= LL_MAX = 2.4e5 (2.394e5 at EM step 0 of `tiles129`, 2.303e5 at its stop), so a relative rounding of 1e-12 in ll cannot
      flip the stop test and n_iter_ is held exactly.
    - ll's own rounding.  ll holds the difference trace G - sum theta, and where the frames are fitted exactly (two frames: psi falls to
      its floor of 1e-12 and G grows to 1e12) that difference cancels: float64 cannot hold it closer than a few ulps of trace G, in
      sklearn's arithmetic as in anyone's (sklearn's exact method and the restatement differ by 2.4e-4 = one ulp of trace G = 1.7e12 on
      `two_rows`, 2.4e-6 of the largest |ll|).  `ll_rounding` = LL_ULPS = 8 ulps of the largest trace G times N / 2 is therefore granted
      to loglike_ on top of the relative tolerance.  It is computed from the restatement alone; it is 3e-3 on `two_rows` and below
      2e-8 - a ten-thousandth of the relative term - on every other fixture, and twice it stays below the stop margin everywhere.
Where n_components exceeds the number of factors in the frames G has no gap after theta_k (the noise eigenvalues sit near 1) and sklearn's
own two methods disagree (15 % of the scores on 300 x 24 frames with 4 factors and k = 6): no fixture is of that kind.

Transform: TRANSFORM_TOL = 4 * 2^-24 of the largest score against the float32-rounded scores of the exact method - one half ulp of the
rounding on either side, and two more for FIT_TOL carried through the k x k solve.  Against the reference's own (randomised) scores the
tolerance is that method's measured deviation from the exact one, r_i (the golden file's `<name>_ref_deviation`, measured on the
restatement, never on the code under test) plus 1e-6 of the largest score.
"""
import functools
import os

import numpy as np

SMALL = 1e-12            # include/mmk_factor_analysis.h: MMK_FA_SMALL
GAP_MIN = 1e-2
STOP_MARGIN = 1e-4
LL_MAX = 2.4e5
FIT_TOL = 1e-9
REF_TOL = 1e-11          # restatement against sklearn's exact method
TRANSFORM_TOL = 4 * 2.0 ** -24
REF_SLACK = 1e-6
LL_ULPS = 8.0

# name -> dict(seed, n, d, k (= the factors in the frames), snr, tol, max_iter, const (column d // 2 is the constant 1.25))
FIXTURES = {
    "f24": dict(seed=1, n=300, d=24, k=4, snr=3.0),
    "odd33": dict(seed=2, n=257, d=33, k=5, snr=2.0),
    "f40": dict(seed=3, n=500, d=40, k=6, snr=2.0),
    "tiles129": dict(seed=4, n=1000, d=129, k=16, snr=2.0),
    "const": dict(seed=5, n=300, d=24, k=4, snr=3.0, const=True),
    "two_rows": dict(seed=7, n=2, d=5, k=1, snr=1.0),
    "wide70": dict(seed=8, n=40, d=70, k=3, snr=3.0),
    "cap3": dict(seed=1, n=300, d=24, k=4, snr=3.0, max_iter=3),
}
for _f in FIXTURES.values():
    _f.setdefault("tol", 1e-2)
    _f.setdefault("max_iter", 1000)
    _f.setdefault("const", False)
NAMES = tuple(FIXTURES)
GOLDEN_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "factor_analysis.npz")


def frames(seed, n, d, kt, snr, const=False):
    """kt factors with falling loadings, a noise variance of its own per column, a column offset; float32"""
    rng = np.random.RandomState(seed)
    load = rng.randn(kt, d) * snr * (np.arange(kt, 0, -1)[:, None] / kt + .5)
    x = (rng.randn(n, kt) @ load + rng.randn(n, d) * (.5 + rng.rand(d)) + 3 * rng.rand(d)).astype(np.float32)
    if const:
        x[:, d // 2] = 1.25
    return x


@functools.lru_cache(maxsize=None)
def fixture_frames(name):
    f = FIXTURES[name]
    x = frames(f["seed"], f["n"], f["d"], f["k"], f["snr"], f["const"])
    x.setflags(write=False)
    return x


def fa64(x, k, tol=1e-2, max_iter=1000):
    """the restatement -> dict(mean, components (k, d), noise_variance, loglike, n_iter, converged, gaps (per EM step), cov, ll_rounding
    (module text))"""
    x = np.asarray(x, dtype=np.float64)
    n, d = x.shape
    mean = x.mean(0)
    xc = x - mean
    c = xc.T @ xc / n
    var = np.diag(c).copy()
    psi, old, lls, gaps = np.ones(d), -np.inf, [], []
    converged, trace_max = False, 0.0
    for _ in range(max_iter):
        sp = np.sqrt(psi) + SMALL
        g = c / sp[:, None] / sp[None, :]
        lam, vec = np.linalg.eigh(g)
        lam, vec = lam[::-1], vec[:, ::-1]
        gaps.append((lam[k - 1] - (lam[k] if k < d else 0.0)) / lam[0])
        theta = lam[:k]
        w = np.sqrt(np.maximum(theta - 1.0, 0.0))[:, None] * vec[:, :k].T * sp
        ll = -n / 2.0 * (d * np.log(2.0 * np.pi) + k + np.log(theta).sum() + (np.trace(g) - theta.sum()) + np.log(psi).sum())
        lls.append(ll)
        trace_max = max(trace_max, float(np.trace(g)))
        if ll - old < tol:
            converged = True
            break
        old = ll
        psi = np.maximum(var - (w ** 2).sum(0), SMALL)
    return dict(mean=mean, components=signed(w), noise_variance=psi, loglike=np.array(lls), n_iter=len(lls), converged=converged,
                gaps=np.array(gaps), cov=c, ll_rounding=LL_ULPS * 2.0 ** -52 * trace_max * n / 2.0)


def transform64(y, mean, components, noise_variance):
    """sklearn's FactorAnalysis.transform"""
    wpsi = components / noise_variance
    cov_z = np.linalg.inv(np.eye(len(components)) + wpsi @ components.T)
    return ((np.asarray(y, dtype=np.float64) - mean) @ wpsi.T) @ cov_z


def transform_matrix64(components, noise_variance):
    """A (k, d) = (I + Wpsi W^T)^-1 Wpsi: transform64(y) = (y - mean) A^T"""
    wpsi = components / noise_variance
    return np.linalg.solve(np.eye(len(components)) + wpsi @ components.T, wpsi)


def signed(components):
    """each row's entry of largest magnitude (the first of equals) positive"""
    components = np.array(components, dtype=np.float64)
    at = np.abs(components).argmax(1)
    s = np.where(components[np.arange(len(components)), at] < 0, -1.0, 1.0)
    return components * s[:, None]


def align(got, want, by_rows=True):
    """`got` with one sign per component (row of components, column of scores) chosen to match `want`"""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    s = np.sign((got * want).sum(1 if by_rows else 0))
    s[s == 0] = 1.0
    return got * (s[:, None] if by_rows else s[None, :])


def rel_err(got, want):
    """the largest deviation over the largest magnitude of `want`"""
    want = np.asarray(want, dtype=np.float64)
    return float(np.abs(np.asarray(got, dtype=np.float64) - want).max() / np.abs(want).max())


@functools.lru_cache(maxsize=None)
def fixture_case(name):
    f = FIXTURES[name]
    x = fixture_frames(name)
    r = fa64(x, f["k"], f["tol"], f["max_iter"])
    r["scores"] = transform64(x, r["mean"], r["components"], r["noise_variance"])
    r["x"], r["f"] = x, f
    return r


@functools.lru_cache(maxsize=None)
def golden():
    with np.load(GOLDEN_PATH) as z:
        return {k: z[k] for k in z.files}
