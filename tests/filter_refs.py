"""float64 references, cases and derived error bounds of the first-order filter section and the row normalisation (include/mmk.h:
mmk_lfilter1_f32, mmk_row_normalize_f32), shared by tests/test_filter_refs.py (CPU) and tests/test_gpu_filters.py.  In the style of
tests/f64_bounds.py: u = 2^-24, every bound is derived from the roundings the computation makes, none is fitted to the kernel.

The filter:  y[n] = f[n] + p y[n-1],  f[n] = b0 x[n] + b1 x[n-1],  p = -a1,  so  y[n] = sum_m p^(n-m) f[m].  With
    g[n]  = |b0 x[n]| + |b1 x[n-1]|
    S[n]  = sum_m |p|^(n-m) g[m]                   = lfilter([1], [1, -|a1|], g)      bounds every partial sum that ends at n
    S2[n] = sum_m |p|^(n-m) S[m]                   = lfilter([1], [1, -|a1|], S)      = sum_m (n - m + 1) |p|^(n-m) g[m]
the error at n, to first order in u, is made of

* the sample-by-sample roundings.  Sample m rounds a few values no larger than S[m] and the recurrence carries that on as |p|^(n-m):
  C_IIR u S2[n].  A scan makes the same roundings on partial sums of the same terms (a run's recurrence from a zero state), which
  are no larger.  C_IIR is not chosen: it is twice the worst  err / (u S2)  of the plain sequential fp32 recurrence on the CPU (numpy
  float32, one fmaf-free update per sample, as torchaudio's core loop) over the inputs of every case below, rounded up.  Worst ratio
  per filter (tests/test_filter_refs.py repeats the measurement and holds the constant to it):
      Emphasis 0: 0.00   0.5: 1.00   0.97: 1.64   0.999: 1.79         Deemphasis 0: 0.00   0.5: 0.78   0.97: 0.89   0.999: 0.83
      RemoveDC: 1.06     (1, 0.3, 0.9): 0.59                           uniform(0, 1) input, Deemphasis 0.97: 0.57
  worst 1.79, twice that rounded up: 4.
* what the scan adds (csrc/filters.hip; none of it for a1 = 0, which is one streaming pass):
  - joins.  Carries are joined level by level: 6 shuffle steps over the lanes of a wave and 4 joins of the waves, in the launch that
    writes the chunk ends and in the one that stores (the same levels over other samples); 6 shuffle steps over the chunk ends and one
    join per round of 64 ends; one join for the lane's carry and one for the sample.  A join is one fmaf: it rounds a partial sum of
    the terms p^(n-m) f[m].  The joins of one level cover disjoint stretches of samples, so carried to n they add up to at most
    u sum_m |p|^(n-m) g[m] = u S[n] per level:     (18 + rounds) u S[n],  rounds = ceil((chunks - 1) / 64).
  - powers.  The factor p^(n-m) of a term is a product of computed powers (p^16 2^b, p^1024, p^4096 2^b by repeated squaring, p^(i+1)
    by a product chain).  Squaring doubles the relative error of its operand and adds one rounding, so p^k carries (k - 1) u however it
    is multiplied up, and the factors of one term have exponents that add up to n - m:
        u sum_m (n - m) |p|^(n-m) g[m] = u (S2[n] - S[n]) <= u S2[n].
  bound[n] = (C_IIR + 1) u S2[n] + (18 + rounds) u S[n]    for a1 != 0,      C_IIR u S2[n] = C_IIR u g[n]    for a1 = 0.

Coefficients are the fp32 values the kernel receives, widened: their rounding is not part of the error.

The normalisation: y = x / max(norm, eps).  p = inf: the maximum is exact, one division: u |y| ... asserted as 2 u |y|.  p = 1, 2: the sum of
non-negative terms goes through NORM_DEPTH(n) roundings on the longest path (16 of a lane's run, 6 butterfly steps, 3 joins of the waves,
ceil(chunks / 64) partials per lane, 6 butterfly steps), each relative to a partial sum that is at most the whole:
    p = 1: (depth + 1) u |y|       p = 2: (depth / 2 + 2) u |y|       (the square root halves the sum's error and rounds, the division rounds).
"""
import functools
import math

import numpy as np
from scipy.signal import lfilter

from mimikit_amd import native

U = 2.0 ** -24
CHUNK, RUN, WG = native.LFILTER1_CHUNK, native.LFILTER1_RUN, native.LFILTER1_WG
C_IIR = 4.0
SCAN_LEVELS = 18
EPS = 1e-12


def f32(v):
    return float(np.float32(v))


def emphasis_coeffs(e):
    return f32(1.0), f32(-e), f32(0.0)


def deemphasis_coeffs(e):
    return f32(1 - e), f32(0.0), f32(-e)


REMOVE_DC = (f32(1.0), f32(-1.0), f32(-0.99))
EMPHASES = (0.0, 0.5, 0.97, 0.999)
# name -> (b0, b1, a1) as the kernel receives them
FILTERS = {**{f"emphasis_{e}": emphasis_coeffs(e) for e in EMPHASES}, **{f"deemphasis_{e}": deemphasis_coeffs(e) for e in EMPHASES},
           "remove_dc": REMOVE_DC, "alternating": (f32(1.0), f32(0.3), f32(0.9))}
LENGTHS = (1, 2, RUN - 1, RUN, RUN + 1, 64 * RUN + 1, CHUNK - 1, CHUNK, CHUNK + 1, 3 * CHUNK + 17)
BATCHES = (1, 3)
POSITIVE_CASE = ("deemphasis_0.97", 3 * CHUNK + 17)        # the uniform(0, 1) input: every carry is large


@functools.lru_cache(maxsize=None)
def case_input(n, positive=False):
    """(3, n) float32, seeded by the length; a batch of 1 is its first row"""
    rng = np.random.default_rng(2000 + n + (7 if positive else 0))
    x = rng.uniform(0.0 if positive else -1.0, 1.0, size=(3, n)).astype(np.float32)
    x.setflags(write=False)
    return x


def _coeff(c, x):
    return np.asarray(c, dtype=x.dtype)


def lfilter1_ref(x, b0, b1, a1, defect=None, at=CHUNK, chunk=CHUNK):
    """y[n] = b0 x[n] + b1 x[n-1] - a1 y[n-1] along the last axis from a zero state, in x's dtype (float64: the reference; float32:
    the plain sequential fp32 recurrence, every product and sum rounded).  b0, b1, a1: scalars, or arrays that broadcast against x's batch axes x.shape[:-1].
    Defects at sample `at`, the first of a chunk: 'carry': its carry-in is dropped; 'b1': its b1 x[n-1] term is missing;
    'power': the chunk of `chunk` samples from `at` applies its carry-in as p^i, not p^(i+1)."""
    b0, b1, a1 = (_coeff(c, x) for c in (b0, b1, a1))
    shape = np.broadcast_shapes(x.shape[:-1], b0.shape, b1.shape, a1.shape)
    n = x.shape[-1]
    y = np.zeros(shape + (n,), dtype=x.dtype)
    prev_y = np.zeros(shape, dtype=x.dtype)
    prev_x = np.zeros(x.shape[:-1], dtype=x.dtype)
    for i in range(n):
        f = b0 * x[..., i] if (defect == "b1" and i == at) else b0 * x[..., i] + b1 * prev_x
        prev_y = f if (defect == "carry" and i == at) else f - a1 * prev_y
        y[..., i] = prev_y
        prev_x = x[..., i]
    if defect == "power" and 0 < at < n:
        p = -a1
        m = min(chunk, n - at)
        y[..., at:at + m] += (p[..., None] != 0) * (1 - p[..., None]) * p[..., None] ** np.arange(m) * y[..., at - 1:at]
    return y


def lfilter1_sums(x64, b0, b1, a1):
    """S and S2 of the module's comment"""
    b0, b1, a1 = (_coeff(c, x64)[..., None] for c in (b0, b1, a1))
    xp = np.concatenate([np.zeros_like(x64[..., :1]), x64[..., :-1]], -1)
    g = np.abs(b0 * x64) + np.abs(b1 * xp)
    g, pole = np.broadcast_arrays(g, np.abs(a1))
    S, S2 = np.empty_like(g), np.empty_like(g)
    for idx in np.ndindex(g.shape[:-1]):
        a = [1.0, -float(pole[idx][0])]
        S[idx] = lfilter([1.0], a, g[idx])
        S2[idx] = lfilter([1.0], a, S[idx])
    return S, S2


def scan_rounds(n):
    return math.ceil((math.ceil(n / CHUNK) - 1) / 64)


def lfilter1_bound(x64, b0, b1, a1):
    S, S2 = lfilter1_sums(x64, b0, b1, a1)
    scan = (_coeff(a1, x64)[..., None] != 0).astype(np.float64)
    return C_IIR * U * S2 + scan * (U * S2 + (SCAN_LEVELS + scan_rounds(x64.shape[-1])) * U * S)


def filter_arrays(names=None):
    names = list(FILTERS) if names is None else list(names)
    co = np.array([FILTERS[k] for k in names], dtype=np.float64)
    return names, co[:, 0], co[:, 1], co[:, 2]


@functools.lru_cache(maxsize=None)
def case_reference(n, positive=False):
    """names, want (filters, 3, n) float64 and bound of every filter over case_input(n) - computed once, shared, never written to"""
    names, b0, b1, a1 = filter_arrays([POSITIVE_CASE[0]] if positive else None)
    x64 = case_input(n, positive).astype(np.float64)
    want = lfilter1_ref(x64, b0[:, None], b1[:, None], a1[:, None])
    bound = lfilter1_bound(x64, b0[:, None], b1[:, None], a1[:, None])
    for a in (want, bound):
        a.setflags(write=False)
    return names, want, bound


def emphasis_io(e, q_levels=256, mlp_dim=32):
    """the mu-law IOSpec of IOSpec.mulaw_io (embedding input) with a pre-emphasis in front of the codec on both sides (e = None: without)"""
    import mimikit_amd as mmk
    mu_law = mmk.MuLawCompress(q_levels)
    tr = mu_law if e is None else mmk.Compose(mmk.Emphasis(e), mu_law)
    ext = mmk.Extractor("signal", mmk.Compose(mmk.FileToSignal(16000), mmk.Normalize(), mmk.RemoveDC()))
    return mmk.IOSpec(inputs=(mmk.InputSpec("signal", tr, mmk.EmbeddingIO()).bind_to(ext),),
                      targets=(mmk.TargetSpec("signal", tr, mmk.MLPIO(hidden_dim=mlp_dim, n_hidden_layers=0, min_temperature=1e-4), objective=mmk.Objective("categorical_dist")).bind_to(ext),))


def outside(got, want, bound):
    """elements of `got` outside the bound (NaN counts as outside)"""
    return ~(np.abs(np.asarray(got, dtype=np.float64) - want) <= bound)


# ---------------------------------------------------------------------------------------------------------------- normalisation
def norm_depth(n):
    return RUN + 6 + (WG // 64 - 1) + math.ceil(math.ceil(n / CHUNK) / 64) + 6


def normalize_ref(x64, p, skip_chunk=None):
    """x / max(||x||_p, eps) over the last axis; defect skip_chunk = j: the norm misses the samples of chunk j"""
    a = np.abs(x64)
    if skip_chunk is not None:
        a = a.copy()
        a[..., skip_chunk * CHUNK:(skip_chunk + 1) * CHUNK] = 0
    norm = a.max(-1, keepdims=True) if p == math.inf else (a.sum(-1, keepdims=True) if p == 1 else np.sqrt((a * a).sum(-1, keepdims=True)))
    return x64 / np.maximum(norm, EPS)


def normalize_bound(y64, p, n):
    if p == math.inf:
        return 2 * U * np.abs(y64)
    d = norm_depth(n)
    return ((d + 1) if p == 1 else (d / 2 + 2)) * U * np.abs(y64)
