"""Host side of ``MelSpec`` / ``MFCC``: librosa's mel filter bank in banded form and scipy's DCT matrices, numpy only.

Both are restatements written from the published sources (``librosa.filters.mel``, ``librosa.core.convert.hz_to_mel`` /
``mel_to_hz`` / ``mel_frequencies``, ``librosa.feature.mfcc``, ``scipy.fft.dct``); neither library is needed at run time.
The reference calls ``melspectrogram(S=...)`` and ``mfcc(S=...)`` without ``sr``, so the sample rate is librosa's
default 22050 whatever the audio's rate, and ``n_fft`` follows from the input's last dimension.
"""
import functools
from typing import NamedTuple, Optional

import numpy as np

__all__ = ["hz_to_mel", "mel_to_hz", "mel_frequencies", "MelBank", "mel_filter_bank", "dct_matrix", "device_bank", "device_dct"]

SR = 22050
_F_SP = 200.0 / 3
_MIN_LOG_HZ = 1000.0
_MIN_LOG_MEL = _MIN_LOG_HZ / _F_SP
_LOGSTEP = np.log(6.4) / 27.0


def hz_to_mel(f, htk: bool = False):
    f = np.asanyarray(f, dtype=np.float64)
    if htk:
        return 2595.0 * np.log10(1.0 + f / 700.0)
    # Slaney: linear below 1000 Hz, logarithmic above
    return np.where(f >= _MIN_LOG_HZ, _MIN_LOG_MEL + np.log(np.maximum(f, _MIN_LOG_HZ) / _MIN_LOG_HZ) / _LOGSTEP, f / _F_SP)


def mel_to_hz(m, htk: bool = False):
    m = np.asanyarray(m, dtype=np.float64)
    if htk:
        return 700.0 * (10.0 ** (m / 2595.0) - 1.0)
    return np.where(m >= _MIN_LOG_MEL, _MIN_LOG_HZ * np.exp(_LOGSTEP * (m - _MIN_LOG_MEL)), _F_SP * m)


def mel_frequencies(n_mels: int, fmin: float = 0.0, fmax: float = 11025.0, htk: bool = False):
    """``n_mels`` frequencies evenly spaced on the mel scale from fmin to fmax (float64)"""
    return mel_to_hz(np.linspace(hz_to_mel(fmin, htk), hz_to_mel(fmax, htk), n_mels), htk)


class MelBank(NamedTuple):
    """band m weighs bins ``lo[m] .. lo[m] + length[m] - 1`` with ``weights[offset[m] .. offset[m] + length[m] - 1]``"""
    n_bins: int
    lo: np.ndarray          # (n_mels,) int32
    length: np.ndarray      # (n_mels,) int32, may hold zeros
    offset: np.ndarray      # (n_mels,) int32
    weights: np.ndarray     # (sum of lengths,) float32

    @property
    def n_mels(self) -> int:
        return len(self.lo)

    def dense(self) -> np.ndarray:
        """(n_mels, n_bins) float32, the array librosa.filters.mel returns"""
        out = np.zeros((self.n_mels, self.n_bins), np.float32)
        for m in range(self.n_mels):
            out[m, self.lo[m]:self.lo[m] + self.length[m]] = self.weights[self.offset[m]:self.offset[m] + self.length[m]]
        return out

    def table(self) -> np.ndarray:
        """(n_mels, 3) int32 rows (lo, length, offset): the layout of include/mmk.h"""
        return np.ascontiguousarray(np.stack((self.lo, self.length, self.offset), axis=1).astype(np.int32))


def dense_mel_filter_bank(n_bins: int, n_mels: int, fmin: float = 0.0, fmax: Optional[float] = None, htk: bool = False,
                          sr: float = SR) -> np.ndarray:
    """librosa.filters.mel(sr=sr, n_fft=2 * (n_bins - 1), n_mels, fmin, fmax, htk, norm="slaney", dtype=float32), (n_mels, n_bins)"""
    n_bins, n_mels = int(n_bins), int(n_mels)
    if n_bins < 2 or n_mels < 1:
        raise ValueError(f"mel_filter_bank: needs n_bins >= 2 and n_mels >= 1, got {n_bins} and {n_mels}")
    n_fft = 2 * (n_bins - 1)
    fmax = float(sr) / 2 if fmax is None else float(fmax)
    fmin = float(fmin)
    if not 0 <= fmin < fmax:
        raise ValueError(f"mel_filter_bank: needs 0 <= fmin < fmax, got {fmin} and {fmax}")
    fftfreqs = np.arange(n_bins, dtype=np.float64) * float(sr) / n_fft
    mel_f = mel_frequencies(n_mels + 2, fmin, fmax, htk)
    fdiff = np.diff(mel_f)
    ramps = np.subtract.outer(mel_f, fftfreqs)
    weights = np.zeros((n_mels, n_bins), np.float32)
    for i in range(n_mels):
        lower = -ramps[i] / fdiff[i]
        upper = ramps[i + 2] / fdiff[i + 1]
        weights[i] = np.maximum(0, np.minimum(lower, upper)) + 0.0     # float64, stored as float32 (+ 0.0: a -0.0 at f == mel_f[i] becomes 0.0)
    enorm = (2.0 / (mel_f[2:n_mels + 2] - mel_f[:n_mels])).astype(np.float32)      # Slaney: unit area per band
    return weights * enorm[:, None]                                     # a float32 product


def mel_filter_bank(n_bins: int, n_mels: int, fmin: float = 0.0, fmax: Optional[float] = None, htk: bool = False, sr: float = SR) -> MelBank:
    """the bank in banded form.  Every band's non-zeros are one run of bins (min(lower, upper) is positive on one interval); a band
    narrower than the bin spacing may have none, its length is then 0."""
    dense = dense_mel_filter_bank(n_bins, n_mels, fmin, fmax, htk, sr)
    lo = np.zeros(n_mels, np.int32)
    length = np.zeros(n_mels, np.int32)
    runs = []
    for m in range(n_mels):
        nz = np.flatnonzero(dense[m])
        if len(nz):
            lo[m], length[m] = nz[0], nz[-1] - nz[0] + 1
            runs.append(dense[m, nz[0]:nz[-1] + 1])
    offset = (np.cumsum(length) - length).astype(np.int32)
    weights = np.concatenate(runs).astype(np.float32) if runs else np.zeros(0, np.float32)
    return MelBank(int(n_bins), lo, length, offset, weights)


def dct_matrix_f64(n_mfcc: int, n_mels: int, dct_type: int = 2, norm: Optional[str] = "ortho", lifter: float = 0) -> np.ndarray:
    """(n_mfcc, n_mels) float64: the first rows of scipy.fft.dct(type, norm) along an axis of n_mels, librosa's lifter folded in"""
    n_mfcc, N = int(n_mfcc), int(n_mels)
    if N < 1 or not 1 <= n_mfcc <= N:
        raise ValueError(f"dct_matrix: needs 1 <= n_mfcc <= n_mels, got {n_mfcc} and {n_mels}")
    if dct_type not in (1, 2, 3):
        raise ValueError(f"dct_matrix: dct_type must be 1, 2 or 3, got {dct_type!r}")
    if norm not in (None, "ortho"):
        raise ValueError(f"dct_matrix: norm must be None or 'ortho', got {norm!r}")
    if lifter < 0:
        raise ValueError(f"dct_matrix: lifter must be non-negative, got {lifter}")
    k = np.arange(N, dtype=np.float64)[:, None]       # output index
    n = np.arange(N, dtype=np.float64)[None, :]       # input index
    if dct_type == 2:
        d = 2.0 * np.cos(np.pi * k * (2 * n + 1) / (2 * N))
        if norm == "ortho":
            d *= np.sqrt(1.0 / (2 * N))
            d[0] *= np.sqrt(0.5)
    elif dct_type == 3:
        d = 2.0 * np.cos(np.pi * n * (2 * k + 1) / (2 * N))
        d[:, 0] = 1.0
        if norm == "ortho":
            d *= np.sqrt(1.0 / (2 * N))
            d[:, 0] *= np.sqrt(2.0)
    else:
        if N < 2:
            raise ValueError("dct_matrix: dct_type 1 needs n_mels >= 2")
        d = 2.0 * np.cos(np.pi * k * n / (N - 1))
        d[:, 0] = 1.0
        d[:, N - 1] = np.where(np.arange(N) % 2 == 0, 1.0, -1.0)
        if norm == "ortho":
            d[:, 0] *= np.sqrt(2.0)
            d[:, N - 1] *= np.sqrt(2.0)
            d *= 0.5 * np.sqrt(2.0 / (N - 1))
            d[0] *= np.sqrt(0.5)
            d[N - 1] *= np.sqrt(0.5)
    d = d[:n_mfcc]
    if lifter > 0:
        d = d * (1.0 + (lifter / 2.0) * np.sin(np.pi * np.arange(1, n_mfcc + 1, dtype=np.float64) / lifter))[:, None]
    return np.ascontiguousarray(d)


def dct_matrix(n_mfcc: int, n_mels: int, dct_type: int = 2, norm: Optional[str] = "ortho", lifter: float = 0) -> np.ndarray:
    return dct_matrix_f64(n_mfcc, n_mels, dct_type, norm, lifter).astype(np.float32)


class DeviceBank(NamedTuple):
    n_bins: int
    n_mels: int
    table_host: np.ndarray      # (n_mels, 3) int32, kept alive for the checks of every call
    table: "torch.Tensor"       # the same on the device
    weights: "torch.Tensor"


@functools.lru_cache(maxsize=32)
def _device_bank(n_bins, n_mels, fmin, fmax, htk, device):
    import torch
    bank = mel_filter_bank(n_bins, n_mels, fmin, fmax, htk)
    table = bank.table()
    return DeviceBank(bank.n_bins, bank.n_mels, table, torch.from_numpy(table).to(device), torch.from_numpy(bank.weights).to(device))


def device_bank(n_bins: int, n_mels: int, fmin: float, fmax: Optional[float], htk: bool, device) -> DeviceBank:
    """the bank on ``device``, one copy per parameter set"""
    return _device_bank(int(n_bins), int(n_mels), float(fmin), None if fmax is None else float(fmax), bool(htk), str(device))


@functools.lru_cache(maxsize=32)
def _device_dct(n_mfcc, n_mels, dct_type, norm, lifter, device):
    import torch
    d = dct_matrix(n_mfcc, n_mels, dct_type, norm, lifter)
    return torch.from_numpy(np.ascontiguousarray(d.T)).to(device)


def device_dct(n_mfcc: int, n_mels: int, dct_type: int, norm: Optional[str], lifter: float, device):
    """the DCT matrix TRANSPOSED, (n_mels, n_mfcc) float32 on ``device`` (the layout of include/mmk.h), one copy per parameter set"""
    return _device_dct(int(n_mfcc), int(n_mels), int(dct_type), norm, float(lifter), str(device))
