"""float64 references and derived error bounds for MelSpec / MFCC (csrc/melbank.h, csrc/melbank.hip, mimikit_amd/features/mel.py).

PROVENANCE.  The mel filter bank below is a RESTATEMENT of librosa.filters.mel (norm="slaney", dtype=float32, sr=22050) and of
hz_to_mel / mel_to_hz / mel_frequencies, written from librosa's published source.  librosa is not installed where this was written: THE
BANK HAS NOT BEEN RUN AGAINST LIBROSA.  What ties it to librosa are the values librosa's documentation prints (ANCHORS below) and the
structure its bank is known to have.  The DCT matrices are restated from scipy's documented definitions and ARE compared with scipy's own
output (tests/golden/melspec.npz, written by tests/golden/make_golden_melspec.py).  This module is written separately from
mimikit_amd/features/mel.py (scalar loops here, array expressions there) so that the two can check each other.

THE ARITHMETIC UNDER TEST.  u = 2^-24.  A band is one fmaf chain from 0 over its n_m bins in ascending order,
    y = fl(w_{n-1} x_{n-1} + fl(... fl(w_1 x_1 + fl(w_0 x_0)))),
n_m roundings, every term non-negative (weights and magnitudes are), so no cancellation: the standard bound for recursive summation
gives |y - s| <= gamma_n s with gamma_n = n u / (1 - n u) and s the exact sum of the same float32 weights and inputs.  The tests use
    BANK:   |y - ref64| <= (n_m + 2) u ref64 + n_m 2^-149
where ref64 is s evaluated in float64 (its own error, n 2^-53 s, and gamma_n - n u are far inside the two spare u) and the last term
is half a subnormal step per rounding, for sums below FLT_MIN, where a rounding is no longer relative.  A band of length 0 is exactly 0.

    DCT:    |z_c - ref64_c| <= (n_mels + 2) u sum_m |d_cm| |x_m| + n_mels 2^-149
the same chain with signed terms: the bound is on the sum of magnitudes.

    BANK + DCT (the bands stay in LDS as float32): the DCT sees bands y_m = mel64_m (1 + e_m), |e_m| <= (n_m + c + 2) u, so
            |z_c - ref64_c| <= u sum_m |d_cm| mel64_m (n_m + c + 2 + n_mels + 2) (1 + 2^-10) + (n_mels + max n_m) 2^-149
    (the factor 1 + 2^-10 covers the product of the two relative errors, at most (n + 4) u < 2^-10 of either for n < 16000).

    FUSED (signal -> mel): the reference is the float64 bank on the float32 magnitudes the existing MagSpec returns, so c is the
    relative distance, in u, between those magnitudes and the ones the mode-6 epilogue holds:
      pad_mode="constant": MagSpec runs output mode 4 and mode 6 evaluates the same expressions: c = 0, and the fused result equals
        MelSpec()(MagSpec()(x)) bit for bit (same magnitudes, weights and order).
      pad_mode="reflect": MagSpec takes the polar kernel's sqrtf(re^2 + im^2).  Either path squares two exact numbers, adds them (2 u: a
        rounded product and the rounded sum, contracted or not), takes a root (halves that: u) that is within one ulp = 2 u (the
        hardware root of modes 4 / 6; sqrtf is at least as good) and scales by an exact 1/2: 3 u each, C_REFLECT = 6 u between them.
"""
import functools
import math

import numpy as np

U = 2.0 ** -24
SUB = 2.0 ** -149
C_REFLECT = 6
SR = 22050.0

# librosa's documentation: mel_frequencies(n_mels=40) (fmin=0, fmax=11025), elements 1, 2, 11, 12, 13, 38, to 3 decimals; and the docstring
# examples hz_to_mel(60) = 0.9, mel_to_hz(3) = 200, hz_to_mel(1000) = 15 (Slaney)
ANCHOR_MEL40 = {1: 85.317, 2: 170.635, 11: 938.49, 12: 1024.856, 13: 1119.114, 38: 10096.408}
ANCHOR_SCALE = (("hz_to_mel", 60.0, 0.9), ("mel_to_hz", 3.0, 200.0), ("hz_to_mel", 1000.0, 15.0))

# (n_mels, fmin, fmax, htk)
BANK_SETS = {"slaney128": (128, 0.0, None, False), "band40": (40, 300.0, 8000.0, False), "htk8": (8, 0.0, None, True),
             "slaney8": (8, 0.0, None, False), "slaney20": (20, 0.0, None, False)}
BANK_BINS = (33, 129, 513, 1025)
DCT_TYPES = (1, 2, 3)
DCT_NORMS = (None, "ortho")
DCT_MELS = (128, 40)


def hz_to_mel(f, htk=False):
    if htk:
        return 2595.0 * math.log10(1.0 + f / 700.0)
    f_sp = 200.0 / 3
    if f >= 1000.0:
        return 1000.0 / f_sp + math.log(f / 1000.0) / (math.log(6.4) / 27.0)
    return f / f_sp


def mel_to_hz(m, htk=False):
    if htk:
        return 700.0 * (10.0 ** (m / 2595.0) - 1.0)
    f_sp = 200.0 / 3
    min_log_mel = 1000.0 / f_sp
    if m >= min_log_mel:
        return 1000.0 * math.exp((math.log(6.4) / 27.0) * (m - min_log_mel))
    return f_sp * m


def mel_frequencies(n, fmin, fmax, htk=False):
    mels = np.linspace(hz_to_mel(fmin, htk), hz_to_mel(fmax, htk), n)
    return np.array([mel_to_hz(float(m), htk) for m in mels], dtype=np.float64)


@functools.lru_cache(maxsize=None)
def mel_bank(n_bins, n_mels, fmin=0.0, fmax=None, htk=False, slaney=True):
    """(n_mels, n_bins) float32, read-only: librosa.filters.mel(sr=22050, n_fft=2 (n_bins - 1)).  slaney=False: the near miss without the
    area normalisation"""
    n_fft = 2 * (n_bins - 1)
    fmax = SR / 2 if fmax is None else fmax
    mel_f = mel_frequencies(n_mels + 2, fmin, fmax, htk)
    out = np.zeros((n_mels, n_bins), dtype=np.float32)
    for i in range(n_mels):
        for k in range(n_bins):
            f = k * SR / n_fft
            lower = (f - mel_f[i]) / (mel_f[i + 1] - mel_f[i])
            upper = (mel_f[i + 2] - f) / (mel_f[i + 2] - mel_f[i + 1])
            out[i, k] = max(0.0, min(lower, upper))
        if slaney:
            out[i] *= np.float32(2.0 / (mel_f[i + 2] - mel_f[i]))
    out.setflags(write=False)
    return out


def band_runs(dense):
    """(first bin, length) per band; length 0 where a band has no weight.  Asserts that a band's non-zeros are one run."""
    lo, length = [], []
    for row in dense:
        nz = np.flatnonzero(row)
        if len(nz) == 0:
            lo.append(0), length.append(0)
            continue
        assert nz[-1] - nz[0] + 1 == len(nz), "a band's non-zero weights are not contiguous"
        lo.append(int(nz[0])), length.append(len(nz))
    return np.array(lo), np.array(length)


def shifted(dense):
    """the near miss of a band start that is off by one bin"""
    out = np.zeros_like(dense)
    out[:, 1:] = dense[:, :-1]
    return out


def dct64(n_mfcc, n_mels, dct_type=2, norm="ortho", lifter=0):
    """(n_mfcc, n_mels) float64: scipy.fft.dct(x, type, norm)[:n_mfcc] as a matrix, row c times 1 + (lifter / 2) sin(pi (c + 1) / lifter)"""
    if lifter < 0:
        raise ValueError("lifter must be non-negative")
    N = n_mels
    d = np.zeros((n_mfcc, N))
    for k in range(n_mfcc):
        for n in range(N):
            if dct_type == 2:
                v = 2.0 * math.cos(math.pi * k * (2 * n + 1) / (2 * N))
                if norm == "ortho":
                    v *= math.sqrt(1.0 / (4 * N)) if k == 0 else math.sqrt(1.0 / (2 * N))
            elif dct_type == 3:
                if norm == "ortho":
                    v = 1.0 / math.sqrt(N) if n == 0 else math.sqrt(2.0 / N) * math.cos(math.pi * n * (2 * k + 1) / (2 * N))
                else:
                    v = 1.0 if n == 0 else 2.0 * math.cos(math.pi * n * (2 * k + 1) / (2 * N))
            else:
                edge = n in (0, N - 1)
                v = (1.0 if n == 0 else (-1.0) ** k) if edge else 2.0 * math.cos(math.pi * k * n / (N - 1))
                if norm == "ortho":                    # scipy: x[0], x[N-1] times sqrt(2); y times sqrt(2 / (N-1)) / 2; y[0], y[N-1] by 1/sqrt(2)
                    v *= (math.sqrt(2.0) if edge else 1.0) * 0.5 * math.sqrt(2.0 / (N - 1)) * (math.sqrt(0.5) if k in (0, N - 1) else 1.0)
            d[k, n] = v
        if lifter > 0:
            d[k] *= 1.0 + (lifter / 2.0) * math.sin(math.pi * (k + 1) / lifter)
    return d


# ---------------------------------------------------------------------------------------------------------------- application and bounds
def mel64(s, dense):
    """(..., n_bins) float32 magnitudes -> (..., n_mels) float64: the exact sums of the float32 weights and inputs, to float64 rounding"""
    return np.asarray(s, dtype=np.float64) @ np.asarray(dense, dtype=np.float64).T


def bank_bound(ref64, dense, c=0):
    _, n = band_runs(dense)
    return (n + c + 2) * U * ref64 + n * SUB


def dct_apply64(x, d64_as_f32):
    return np.asarray(x, dtype=np.float64) @ np.asarray(d64_as_f32, dtype=np.float64).T


def dct_bound(x, d32):
    n_mels = d32.shape[1]
    return (n_mels + 2) * U * (np.abs(np.asarray(x, dtype=np.float64)) @ np.abs(np.asarray(d32, dtype=np.float64)).T) + n_mels * SUB


def mfcc_bound(mel_ref64, dense, d32, c=0):
    """bank + DCT with the bands in float32 between them"""
    _, n = band_runs(dense)
    n_mels = d32.shape[1]
    per_band = (n + c + 2 + n_mels + 2) * mel_ref64
    return U * (per_band @ np.abs(np.asarray(d32, dtype=np.float64)).T) * (1 + 2.0 ** -10) + (n_mels + int(n.max())) * SUB


def outside(got, want, bound):
    return ~(np.abs(np.asarray(got, dtype=np.float64) - want) <= bound)


def assert_inside(got, want, bound, what):
    bad = outside(got, want, bound)
    if bad.any():
        i = tuple(int(a[0]) for a in np.nonzero(bad))
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.size} elements outside the derived bound; at {i}: got {float(got[i]):.9g}, "
                             f"want {want[i]:.9g}, error {abs(float(got[i]) - want[i]):.3e} > bound {bound[i]:.3e}")
    return float(np.max(np.abs(np.asarray(got, dtype=np.float64) - want) / np.maximum(bound, 1e-300)))


def assert_near_miss_leaves(defect, want, bound, what):
    assert bool(outside(defect, want, bound).any()), f"{what}: a near miss stays inside the bound - the bound is too loose"


# ---------------------------------------------------------------------------------------------------------------- inputs
@functools.lru_cache(maxsize=None)
def spectrogram(rows, n_bins, seed=650):
    """non-negative float32 (rows, n_bins), read-only: a wide dynamic range, exact zeros and a few subnormals"""
    rng = np.random.default_rng(seed + 7 * rows + n_bins)
    s = (rng.exponential(1.0, (rows, n_bins)) ** 3).astype(np.float32)
    s[rng.random(s.shape) < 0.05] = 0.0
    s[:, n_bins // 3] *= np.float32(1e-39)
    s.setflags(write=False)
    return s


@functools.lru_cache(maxsize=None)
def mel_frames(rows, n_mels, seed=680):
    """float32 (rows, n_mels), read-only, non-negative as mel frames are"""
    rng = np.random.default_rng(seed + 3 * rows + n_mels)
    x = (rng.exponential(1.0, (rows, n_mels)) ** 2).astype(np.float32)
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def signal(batch, n, seed=22050):
    """seeded noise plus a sinusoid per clip, float32 (batch, n), read-only"""
    rng = np.random.default_rng(seed + batch + n)
    t = np.arange(n)
    x = 0.1 * rng.standard_normal((batch, n)) + 0.5 * np.sin(2 * np.pi * (0.01 + 0.013 * np.arange(batch))[:, None] * t[None, :])
    x = x.astype(np.float32)
    x.setflags(write=False)
    return x
