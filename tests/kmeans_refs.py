"""float64 restatements, cases and derived bounds of the k-means kernels (include/mmk_kmeans.h: mmk_kmeans_assign_f32,
mmk_kmeans_label_sums_f64, mmk_kmeans_pp_step_f64) and of mimikit_amd.extract.clusters.KMeans / lloyd, shared by tests/test_kmeans_refs.py
(CPU), tests/test_gpu_kmeans.py and tests/golden/make_golden_kmeans.py.  numpy only, in the style of tests/qcluster_refs.py: u = 2^-24,
v = 2^-53, every bound is derived from the roundings the computation makes, none is fitted to what the GPU returns.

The algorithm (sklearn.cluster.KMeans, init "k-means++", algorithm "lloyd", tol 1e-4, unit weights), restated by `fit64`:
    mu = fl32(the float64 column mean of x), x' = fl32(x - mu) - everything below is about x';  tol = 1e-4 mean_c var_c(x)
    draws: rs = RandomState(seed) for all runs; per run rs.choice(N, p=full(N, 1 / N)), then K - 1 times rs.uniform(size=2 + int(log K))
    seeding (`seeding64`): closest = |x' - x'_first|^2, pot = sum closest; per further centre cand = clip(searchsorted(cumsum closest,
        u pot, "left"), N - 1), m_t = min(closest, |x' - x'_cand_t|^2), the first t with the smallest sum m_t wins
    Lloyd (`lloyd64`): label = the first arg-max of <x'_r, c_j> - |c_j|^2 / 2; centres = fl32(float64 mean of the members); the n_e
        frames farthest from their own old centre (descending |x'_r - c_old[label_r]|^2, ties to the lower index) go to the n_e empty
        clusters in rising cluster number and leave their old clusters' sums and counts; stop when the labels repeat ("strict"), else
        when sum |c_new - c_old|^2 <= tol, and then, as when max_iter runs out, assign once more; inertia directly in float64
    the run kept: the first, then a later one with a strictly smaller inertia that is not the same clustering up to renaming

Bounds.  With K the number of bins here written D:
  key       key[r, j] = <x'_r, c_j> + s_j, s_j = fl32(-|c_j|^2 / 2 in float64).  The dot product is a chain of D fused multiply-adds:
            e1 = g(D) <|x'_r|, |c_j|>, g(n) = n u / (1 - n u).  The shift is D fused multiply-adds and six butterfly adds of non-negative
            terms in float64, an exact product with -0.5 and ONE rounding: e2 = (u + (D + 7) v) |c_j|^2 / 2.  The sum rounds once more:
                key_bound[r, j] = (e1 + e2) (1 + u) + u |key64[r, j]|                       (qcluster_refs' euclidean bound)
            End to end the device's centres are not the restatement's: both are fl32(S / n_j) of float64 sums S taken in different orders,
            |S_dev - S_ref| <= 2 g64(n_j + SLABS) sum_r |x'_rc|, g64(n) = n v / (1 - n v), and the rounding can then fall to the other side:
                cerr[j, c] = u |c_jc| + 2 g64(n_j + SLABS) (sum_{r in j} |x'_rc|) / n_j (1 + u)
            which moves a key by at most  <|x'_r|, cerr_j> + <|c_j|, cerr_j> + |cerr_j|^2 / 2  (`centre_term`), added to the bound.
  labels    fp32 keys order two centres as float64 does wherever their float64 keys differ by more than the sum of their bounds.  A row
            is SAFE where key64[best] - key64[j] > 2 max(bound[best], bound[j]) for every other j: there the device must give float64's
            label.  Elsewhere its chosen key must lie within bound[chosen] + bound[best] of the best.
  sums      n_j terms added in float64 in some order, then at most SLABS partials: |S - S64| <= g64(n_j + SLABS) sum_{r in j} |x'_rc|.
  centres   one rounding of S / n_j:  u |c64| + sum_bound / n_j (1 + u).
  row_d2    the differences are exact; D products rounded once each and D + 6 adds of non-negative terms: g64(2 D + 8) d2.
  inertia, pots   a sum of n such non-negative terms in a fixed tree of at most n + SLABS adds: g64(2 D + 8 + n + SLABS) of the sum.
"""
import functools
import math

import numpy as np

from mimikit_amd import native
from tests import neighbors_refs as NR

U = NR.U
V = NR.V
SLABS = native.KMEANS_MAX_SLABS
MAX_K = native.KMEANS_MAX_K
MAX_TRIALS = native.KMEANS_PP_MAX_TRIALS
LEFT_CAP = 0.01                       # at most this share of a case's rows may be left to the second label rule

# the kernels' size grid: one past a workgroup's rows, one past a chunk of bins, one past a 32-column product and the largest instance
NS = (1, 129, 257)
DS = (1, 33, 129)
KS = (1, 2, 16, 33, 256)
DEFECTS = ("ties_high", "norm_not_halved", "offset_one_operand", "searchsorted_right", "fresh_generator", "no_same_clustering")


def gamma(n):
    return NR.gamma(n)


def gamma64(n):
    return n * V / (1 - n * V)


def rng_of(seed):
    return np.random.Generator(np.random.PCG64(seed))


# ---------------------------------------------------------------------------------------------------------------- kernel cases
@functools.lru_cache(maxsize=None)
def kernel_case(n, d, k, with_offset=True):
    """(x (n, d) f32, offset (d,) f32 or None, centres (k, d) f32 in the coordinates of x') of the size grid"""
    rng = rng_of(1000003 * n + 1009 * d + k + (0 if with_offset else 7))
    offset = (3.0 + rng.standard_normal(d)).astype(np.float32) if with_offset else None
    x = rng.standard_normal((n, d)).astype(np.float32)
    if with_offset:
        x = (x + offset).astype(np.float32)
    centres = rng.standard_normal((k, d)).astype(np.float32)
    take = rng.permutation(min(n, k))[:min(n, k) // 2]                 # half of the centres (where there are rows for it) sit near a row
    centres[take] = (centred(x, offset)[take] + 0.05 * rng.standard_normal((take.shape[0], d))).astype(np.float32)
    for a in (x, centres):
        a.setflags(write=False)
    return x, offset, centres


def centred(x, offset):
    """x' = fl32(x - offset), as float32"""
    return x if offset is None else (x - offset[None, :]).astype(np.float32)


# ---------------------------------------------------------------------------------------------------------------- keys, labels
def key64(xp, centres, halved=True):
    xp, c = np.asarray(xp, dtype=np.float64), np.asarray(centres, dtype=np.float64)
    return xp @ c.T - (0.5 if halved else 1.0) * (c * c).sum(-1)[None, :]


def key_bound(xp, centres):
    xp, c = np.asarray(xp, dtype=np.float64), np.asarray(centres, dtype=np.float64)
    d = xp.shape[-1]
    e1 = gamma(d) * (np.abs(xp) @ np.abs(c).T)
    e2 = (U + (d + 7) * V) * 0.5 * (c * c).sum(-1)[None, :]
    return (e1 + e2) * (1 + U) + U * np.abs(key64(xp, c))


def centre_term(xp, centres, cerr):
    """what an error of cerr (k, d) in the centres moves a key by, at most (module docstring)"""
    xp, c = np.asarray(xp, dtype=np.float64), np.asarray(centres, dtype=np.float64)
    return np.abs(xp) @ cerr.T + ((np.abs(c) * cerr).sum(-1) + 0.5 * (cerr * cerr).sum(-1))[None, :]


def first_argmax(key, high=False):
    """the first (high: the last) column with the row's largest key"""
    if high:
        return key.shape[1] - 1 - np.argmax(key[:, ::-1], axis=1)
    return np.argmax(key, axis=1)


def safe_rows(key, bound):
    """(labels64, safe): safe[r] where key64[best] - key64[j] > 2 max(bound[best], bound[j]) for every other j"""
    best = first_argmax(key)
    rows = np.arange(key.shape[0])
    gap = key[rows, best][:, None] - key
    need = 2 * np.maximum(bound[rows, best][:, None], bound)
    ok = gap > need
    ok[rows, best] = True
    return best, ok.all(1)


def gap_ratio(key, bound):
    """the smallest (key64[best] - key64[j]) / (2 max(bound[best], bound[j])) over the rows and the other centres j (inf for one centre)"""
    if key.shape[1] < 2:
        return math.inf
    best = first_argmax(key)
    rows = np.arange(key.shape[0])
    ratio = (key[rows, best][:, None] - key) / (2 * np.maximum(bound[rows, best][:, None], bound))
    ratio[rows, best] = np.inf
    return float(ratio.min())


def label_rule_violations(labels, got_key, key, bound):
    """rows whose device label / key break the label rule (module docstring); -> (bad rows, rows left to the second rule)"""
    labels = np.asarray(labels)
    rows = np.arange(key.shape[0])
    valid = (labels >= 0) & (labels < key.shape[1])
    at = np.where(valid, labels, 0)
    best, safe = safe_rows(key, bound)
    near = key[rows, best] - key[rows, at] <= bound[rows, at] + bound[rows, best]
    bad = ~valid | np.where(safe, labels != best, ~near)
    if got_key is not None:
        bad |= ~(np.abs(np.asarray(got_key, dtype=np.float64) - key[rows, at]) <= bound[rows, at])
    return bad, ~safe


# ---------------------------------------------------------------------------------------------------------------- sums, distances
def label_sums64(xp, labels, k):
    """(sums (k, d) f64, counts (k,), abs sums (k, d)): rows with a label outside [0, k) are left out"""
    xp = np.asarray(xp, dtype=np.float64)
    labels = np.asarray(labels)
    keep = (labels >= 0) & (labels < k)
    sums, asum = np.zeros((k, xp.shape[1])), np.zeros((k, xp.shape[1]))
    np.add.at(sums, labels[keep], xp[keep])
    np.add.at(asum, labels[keep], np.abs(xp[keep]))
    return sums, np.bincount(labels[keep], minlength=k).astype(np.int64), asum


def sums_bound(counts, asum):
    return gamma64(counts + SLABS)[:, None] * asum


def row_d2_64(xp, labels, centres):
    xp, c = np.asarray(xp, dtype=np.float64), np.asarray(centres, dtype=np.float64)
    labels = np.asarray(labels)
    keep = (labels >= 0) & (labels < c.shape[0])
    d2 = ((xp - c[np.where(keep, labels, 0)]) ** 2).sum(-1)
    return np.where(keep, d2, 0.0)


def d2_bound(d2, d):
    return gamma64(2 * d + 8) * d2


def total_bound(total, n, d):
    return gamma64(2 * d + 8 + n + SLABS) * total


def pp_step64(xp, cand, closest):
    """one seeding step -> (closest after, pot, the winning candidate's position, the pots)"""
    xp = np.asarray(xp, dtype=np.float64)
    cand = np.clip(np.asarray(cand), 0, xp.shape[0] - 1)
    m = np.minimum(closest[None, :], ((xp[None, :, :] - xp[cand][:, None, :]) ** 2).sum(-1))
    pots = m.sum(-1)
    t = int(np.argmin(pots))
    return m[t], float(pots[t]), t, pots


# ---------------------------------------------------------------------------------------------------------------- the estimator
def draws(seed, n, k, n_init, fresh=False):
    """[(first, uniforms (k - 1, T))] per run from ONE RandomState (fresh: the defect - every run starts a generator of its own)"""
    rs = np.random.RandomState(seed)
    trials = 2 + int(math.log(k))
    out = []
    for _ in range(n_init):
        if fresh:
            rs = np.random.RandomState(seed)
        first = int(rs.choice(n, p=np.full(n, 1 / n)))
        out.append((first, np.array([rs.uniform(size=trials) for _ in range(k - 1)]).reshape(k - 1, trials)))
    return out


def seeding64(xp, first, uniforms, side="left", other=None):
    """-> (rows (k,), margin): margin = the smallest distance of a draw u pot from a boundary of the scan, over pot.  other: the defect
    'offset ignored on one operand' - the candidate rows are taken from `other` (the uncentred corpus) instead of x'"""
    xp = np.asarray(xp, dtype=np.float64)
    src = xp if other is None else np.asarray(other, dtype=np.float64)
    n = xp.shape[0]
    closest = ((xp - src[first]) ** 2).sum(-1)
    pot = closest.sum()
    rows, margin = [first], math.inf
    for u in uniforms:
        cum = np.cumsum(closest)
        vals = u * pot
        cand = np.clip(np.searchsorted(cum, vals, side=side), None, n - 1)
        if pot > 0:
            margin = min(margin, float(np.abs(cum[None, :] - vals[:, None]).min() / pot))
        m = np.minimum(closest[None, :], ((xp[None, :, :] - src[cand][:, None, :]) ** 2).sum(-1))
        pots = m.sum(-1)
        t = int(np.argmin(pots))
        others = pots[cand != cand[t]]
        if others.size and pot > 0:
            margin = min(margin, float((others.min() - pots[t]) / pot))
        closest, pot = m[t], pots[t]
        rows.append(int(cand[t]))
    return np.array(rows, dtype=np.int64), margin


def lloyd64(xp, init, max_iter, tol, defect=None, raw=None):
    """one run on x' (n, d) float32 from init (k, d) float32 -> dict(labels, inertia, centres (float32, centred), n_iter, ratio = the
    smallest gap ratio over the iterations, end-to-end bound (with the centres' own rounding), shift_margin = the smallest
    |shift - tol| / tol over the iterations that test it).  raw: the uncentred corpus, for the defect 'offset ignored on one operand'"""
    xp32 = np.asarray(xp, dtype=np.float32)
    x64 = xp32.astype(np.float64)
    q64 = x64 if defect != "offset_one_operand" else np.asarray(raw, dtype=np.float64)
    n, k = x64.shape[0], init.shape[0]
    centres = np.asarray(init, dtype=np.float32)
    cerr = U * np.abs(centres.astype(np.float64))
    labels_old = np.full(n, -1)
    ratio, shift_margin, strict, n_iter = math.inf, math.inf, False, 0

    def assign(c, cerr):
        key = key64(q64, c, halved=defect != "norm_not_halved")
        bound = key_bound(q64, c) + centre_term(q64, c, cerr)
        return first_argmax(key, high=defect == "ties_high"), gap_ratio(key, bound)

    for i in range(max_iter):
        labels, r = assign(centres, cerr)
        ratio = min(ratio, r)
        sums, counts, asum = label_sums64(x64, labels, k)
        empty = np.nonzero(counts == 0)[0]
        if empty.size:
            d2 = row_d2_64(x64, labels, centres)
            far = np.argsort(-d2, kind="stable")[:empty.size]
            for j, r_far in zip(empty, far):
                sums[labels[r_far]] -= x64[r_far]
                asum[labels[r_far]] += np.abs(x64[r_far])
                counts[labels[r_far]] -= 1
                sums[j], asum[j], counts[j] = x64[r_far], np.abs(x64[r_far]), 1
        div = np.maximum(counts, 1)[:, None]
        new = (sums / div).astype(np.float32)
        cerr = U * np.abs(new.astype(np.float64)) + 2 * gamma64(counts + SLABS)[:, None] * asum / div * (1 + U)
        old, centres, n_iter = centres, new, i + 1
        if np.array_equal(labels, labels_old):
            strict = True
            break
        shift = float(((new.astype(np.float64) - old.astype(np.float64)) ** 2).sum())
        if tol > 0:
            shift_margin = min(shift_margin, abs(shift - tol) / tol)
        if shift <= tol:
            break
        labels_old = labels
    if not strict:
        labels, r = assign(centres, cerr)
        ratio = min(ratio, r)
    inertia = float(row_d2_64(x64, labels, centres).sum())
    return dict(labels=labels.astype(np.int64), inertia=inertia, centres=centres, n_iter=n_iter, ratio=ratio, shift_margin=shift_margin, cerr=cerr)


def same_clustering(a, b, k):
    """every label of a is paired with one single label of b (sklearn's _is_same_clustering)"""
    return np.unique(a.astype(np.int64) * k + b).size == np.unique(a).size


def centre_stats(x):
    """(mu float32, tol): the float64 column mean rounded once; 1e-4 x the mean population variance"""
    x64 = np.asarray(x, dtype=np.float64)
    return x64.mean(0).astype(np.float32), 1e-4 * float(x64.var(0).mean())


def fit64(x, k, n_init=2, max_iter=100, seed=42, defect=None):
    """KMeans(k, n_init, max_iter, random_state=seed).fit(x) restated -> dict(labels, centres (input coordinates, float32), centres_c (centred),
    inertia, n_iter, seed_rows (n_init, k), winner, ratio, margin, shift_margin, cerr)"""
    x = np.asarray(x, dtype=np.float32)
    mu, tol = centre_stats(x)
    xp = (x - mu[None, :]).astype(np.float32)
    best, seed_rows, ratio, margin, shift_margin = None, [], math.inf, math.inf, math.inf
    for run, (first, uniforms) in enumerate(draws(seed, x.shape[0], k, n_init, fresh=defect == "fresh_generator")):
        rows, m = seeding64(xp, first, uniforms, side="right" if defect == "searchsorted_right" else "left",
                            other=x if defect == "offset_one_operand" else None)
        seed_rows.append(rows)
        res = lloyd64(xp, xp[rows], max_iter, tol, defect, raw=x)
        ratio, margin, shift_margin = min(ratio, res["ratio"]), min(margin, m), min(shift_margin, res["shift_margin"])
        if best is None or (res["inertia"] < best["inertia"] and (defect == "no_same_clustering" or not same_clustering(res["labels"], best["labels"], k))):
            best = dict(res, winner=run)
    return dict(labels=best["labels"], centres=(best["centres"] + mu[None, :]).astype(np.float32), centres_c=best["centres"], inertia=best["inertia"],
                n_iter=best["n_iter"], seed_rows=np.array(seed_rows), winner=best["winner"], ratio=ratio, margin=margin, shift_margin=shift_margin,
                cerr=best["cerr"], mu=mu)


def lloyd_from64(x, init, max_iter=100, defect=None):
    """clusters.lloyd restated: init in the input's coordinates"""
    x = np.asarray(x, dtype=np.float32)
    mu, tol = centre_stats(x)
    xp = (x - mu[None, :]).astype(np.float32)
    res = lloyd64(xp, (np.asarray(init, dtype=np.float32) - mu[None, :]).astype(np.float32), max_iter, tol, defect, raw=x)
    return dict(res, centres_c=res["centres"], centres=(res["centres"] + mu[None, :]).astype(np.float32), mu=mu)


# ---------------------------------------------------------------------------------------------------------------- the fixtures
def _blobs(seed, n, d, k, spread, noise, mean=0.0):
    rng = rng_of(seed)
    c = rng.uniform(-spread, spread, (k, d))
    return (mean + c[rng.integers(0, k, n)] + noise * rng.standard_normal((n, d))).astype(np.float32)


def _spectra(seed, n, d, k, amp, noise):
    rng = rng_of(seed)
    shapes = np.abs(rng.standard_normal((k, d))) * np.exp(-np.arange(d) / 40.0)[None, :]
    return (20.0 + amp * shapes[rng.integers(0, k, n)] + noise * np.abs(rng.standard_normal((n, d)))).astype(np.float32)


# name: (corpus recipe, its arguments, n_clusters, random_seed, fewest iterations, max_iter) - tests/golden/make_golden_kmeans.py checks
# the conditions
FIT_FIXTURES = {
    "blobs": (_blobs, (11, 600, 16, 16, 4.0, 0.3), 16, 42, 1, 100),
    "overlap": (_blobs, (12, 2000, 16, 16, 1.0, 0.6), 16, 45, 15, 100),
    "wide": (_blobs, (13, 400, 257, 8, 1.0, 0.5), 8, 42, 1, 100),
    "spectra": (_spectra, (14, 1000, 129, 12, 1.0, 1.5), 12, 45, 10, 100),
    # both seedings reach the same three blobs after the one iteration allowed, the second with the smaller inertia and other cluster
    # numbers: the first run is kept only because the two are the same clustering
    "renamed": (_blobs, (21, 300, 4, 3, 3.0, 0.5), 3, 1, 1, 1),
}
# name: (corpus arguments, rows of the corpus that are centres, the last centre) - one Lloyd run from a given init
LLOYD_FIXTURES = {
    "far": ((15, 300, 8, 5, 3.0, 0.4), (3, 50, 120, 200), "far"),       # a centre far from all data: one cluster is empty at iteration 0
}


@functools.lru_cache(maxsize=None)
def fit_corpus(name):
    recipe, args = FIT_FIXTURES[name][:2]
    x = recipe(*args)
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def lloyd_corpus(name):
    args, rows, last = LLOYD_FIXTURES[name]
    x = _blobs(*args)
    init = np.concatenate([x[list(rows)], np.full((1, x.shape[1]), 100.0, dtype=np.float32)])
    x.setflags(write=False)
    init.setflags(write=False)
    return x, init


def checksum(x):
    return float(np.asarray(x, dtype=np.float64).sum())


@functools.lru_cache(maxsize=None)
def fit_result(name, defect=None):
    k, seed, _, max_iter = FIT_FIXTURES[name][2:]
    return fit64(fit_corpus(name), k, max_iter=max_iter, seed=seed, defect=defect)


@functools.lru_cache(maxsize=None)
def lloyd_result(name, defect=None):
    return lloyd_from64(*lloyd_corpus(name), defect=defect)


# ---------------------------------------------------------------------------------------------------------------- special inputs
COPY_ROWS = (5, 150)          # two identical rows, in different workgroups of the assignment
ZERO_ROW = 77                 # x' = 0 exactly
SAME_CENTRES = (1, 4)         # two identical centres, near row 10: the lower index takes the rows
FAR_CENTRE = 3                # a centre with no member


@functools.lru_cache(maxsize=None)
def special_case(with_offset=True):
    """(x (200, 33), offset or None, centres (6, 33)) with the special inputs above"""
    n, d, k = 200, 33, 6
    rng = rng_of(99 if with_offset else 98)
    offset = (3.0 + rng.standard_normal(d)).astype(np.float32) if with_offset else None
    x = rng.standard_normal((n, d)).astype(np.float32)
    if with_offset:
        x = (x + offset).astype(np.float32)
    x[COPY_ROWS[1]] = x[COPY_ROWS[0]]
    x[ZERO_ROW] = 0.0 if offset is None else offset
    centres = (0.3 * rng.standard_normal((k, d))).astype(np.float32)
    centres[SAME_CENTRES[0]] = centred(x, offset)[10]
    centres[SAME_CENTRES[1]] = centres[SAME_CENTRES[0]]
    centres[FAR_CENTRE] = 100.0
    for a in (x, centres):
        a.setflags(write=False)
    return x, offset, centres
