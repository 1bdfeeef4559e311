"""Feature functionals on the generate path.

Protocol and names follow the reference's ``mimikit/features/functionals.py``
(``Functional`` :81-111): a functional is a config dataclass that maps arrays to
arrays, dispatching on the input type, and knows its inverse, its time ``unit``
and its ``elem_type``.  Only the functionals the generate path touches exist
here:

* ``MuLawCompress`` / ``MuLawExpand`` (:313-373) and ``STFT`` / ``MagSpec``
  (:450-528, :576-606): the torch path runs as HIP kernels on the MI355X
  (``mimikit_amd/csrc/features.hip``); a tensor that is not on the HIP device is
  an error, there is no eager fallback.
* ``FileToSignal``, ``Compose``, ``Identity``: unit / elem_type carriers needed to build an ``IOSpec`` (decoding
  audio files is out of scope).
* ``Emphasis`` / ``Deemphasis`` (:256-288), ``RemoveDC`` (:216-233) and ``Normalize`` (:236-253), the signal
  conditioning around the mu-law codec: on a device tensor the three filters are one first-order section each
  (``native.lfilter1``, a chunked scan in ``csrc/filters.hip``) and Normalize a two-stage row reduction
  (``native.row_normalize``); float32 only.
* ``ISTFT`` / ``GLA`` (:531-573, :609-646), the ``inv`` of STFT / MagSpec at the loop's tail, run on the HIP
  kernels of ``csrc/istft.hip`` / ``spectral2048.hip``; GLA's parity is unpinned (torchaudio is not installed in the
  build container).
* ``Envelop`` / ``EnvelopBank`` / ``Interpolate`` / ``Derivative`` (:794-1004), the envelope followers the reference's
  ``Samplifyer`` is built on: frame energies as an epilogue of the STFT kernels (``native.stft_energy``: the spectrogram
  is never written), interpolation and the lagged-difference stencil in ``csrc/envelope.hip``.  Results stay on the device.
* ``PCA`` (:1114-1138), the dimension reduction of the clusterizer's pre-processing pipeline: column statistics, an fp64 MFMA
  covariance, a block subspace iteration for the leading eigenvectors and the projection, all in ``csrc/pca.hip``.
* ``HarmonicSource`` / ``PercussiveSource`` (:736-791), librosa's median-filter harmonic / percussive separation of a magnitude
  spectrogram: both running medians, the soft masks and the product in one launch (``native.hpss``, ``csrc/hpss.hip``).
* ``MelSpec`` / ``MFCC`` (:650-707), librosa's mel filter bank in banded form and scipy's DCT behind it (``features/mel.py``,
  ``csrc/melbank.hip``): on a spectrogram (``native.melbank``) or, through ``from_signal``, as an epilogue of the STFT kernels
  (``native.stft_mel``: one launch from the signal to the mel or MFCC frames, the spectrogram is never written).
* ``NearestNeighborFilter`` (:1083-1111), librosa's mutual k-nearest-neighbour median (or mean, max, min) of the frames: the k-best
  search of ``csrc/neighbors.hip`` and one gather-and-aggregate launch behind it (``native.nn_aggregate``, ``csrc/nn_filter.hip``).
* ``NMF`` (:1141-1170), sklearn's non-negative matrix factorisation with its defaults: the NNDSVDA start from the PCA kernels' Gram
  matrix and eigenpairs, and the cyclic coordinate-descent solver with its stop rule on the device (``csrc/nmf.hip``).
* ``AutoConvolve`` / ``F0Filter`` (:1007-1080), the two harmonic filters of a magnitude spectrogram: a float64 weight per bin (the log of
  a product over neighbouring frames; overtone samples minus interpolated undertone samples), normalised over the frame and multiplied
  onto the input, one launch each (``native.auto_convolve``, ``native.f0_filter``, ``csrc/spec_filter.hip``).
* ``FactorAnalysis`` (:1173-1203), sklearn's EM factor analysis in Gram form: one covariance pass by the PCA kernels, then the whole EM
  loop on the device on the D x D matrix alone (``native.fa_fit``, ``csrc/factor_analysis.hip``), the scores by ``native.pca_project``.
* float64 tensors are computed in fp32 on the device (the kernels are fp32; the reference computes in the input's
  dtype, so float64 mu-law codes may differ from it for inputs within one fp32 ulp of a bin edge).
"""
import abc
import dataclasses as dtc
import functools
from typing import Optional, Tuple, Union

import numpy as np
import torch

from ..config import Config
from .item_spec import Frame, Sample, Unit, convert

__all__ = [
    "Continuous", "Discrete", "Functional", "Identity", "Compose", "FileToSignal", "RemoveDC", "Normalize", "Emphasis", "Deemphasis",
    "MuLawCompress", "MuLawExpand", "STFT", "ISTFT", "MagSpec", "GLA", "Resample", "Envelop", "EnvelopBank", "Interpolate", "Derivative",
    "PCA", "HarmonicSource", "PercussiveSource", "MelSpec", "MFCC", "NearestNeighborFilter", "NMF", "AutoConvolve", "F0Filter",
    "FactorAnalysis",
]

N_FFT = 2048
HOP_LENGTH = 512
SR = 22050
Q_LEVELS = 256


@dtc.dataclass
class Continuous:
    min_value: Union[float, int]
    max_value: Union[float, int]
    size: int


@dtc.dataclass
class Discrete:
    size: int


EventType = Union[Continuous, Discrete]


@dtc.dataclass
class Functional(Config, abc.ABC):
    """array -> array map with numpy and torch twins"""

    @property
    def unit(self) -> Optional[Unit]:
        return None

    @property
    def elem_type(self) -> Optional[EventType]:
        return None

    @abc.abstractmethod
    def np_func(self, inputs):
        ...

    @abc.abstractmethod
    def torch_func(self, inputs):
        ...

    def __call__(self, inputs):
        if isinstance(inputs, np.ndarray):
            return self.np_func(inputs)
        if isinstance(inputs, torch.Tensor):
            return self.torch_func(inputs)
        raise KeyError(type(inputs))

    @property
    @abc.abstractmethod
    def inv(self) -> "Functional":
        ...


@dtc.dataclass
class Identity(Functional):
    def np_func(self, inputs):
        return inputs

    def torch_func(self, inputs):
        return inputs

    @property
    def inv(self) -> Functional:
        return Identity()


@dtc.dataclass
class Compose(Functional):
    functionals: Tuple[Functional, ...] = ()

    def __init__(self, *funcs: Functional, functionals=()):
        self.functionals = tuple(funcs) or tuple(functionals)

    def _last(self, attr):
        found = [getattr(f, attr) for f in self.functionals if getattr(f, attr) is not None]
        return found[-1] if found else None

    @property
    def unit(self) -> Optional[Unit]:
        return self._last("unit")

    @property
    def elem_type(self) -> Optional[EventType]:
        return self._last("elem_type")

    def np_func(self, inputs):
        return self(inputs)

    def torch_func(self, inputs):
        return self(inputs)

    def __call__(self, inputs):
        for f in self.functionals:
            inputs = f(inputs)
        return inputs

    @property
    def inv(self) -> Functional:
        return Compose(*(f.inv for f in reversed(self.functionals)))


@dtc.dataclass
class FileToSignal(Functional):
    """Head of an extraction chain: carries the sample rate (reference :150-176).
    Decoding audio files (librosa) belongs to dataset preparation, not to this path."""
    sr: int = SR
    offset: float = 0.
    duration: Optional[float] = None

    @property
    def unit(self) -> Optional[Unit]:
        return Sample(self.sr)

    @property
    def elem_type(self) -> Optional[EventType]:
        return Continuous(-float("inf"), float("inf"), 1)

    def np_func(self, path):
        raise NotImplementedError("decoding audio files is dataset preparation and outside this package's scope")

    def torch_func(self, path):
        return self.np_func(path)

    def __call__(self, path):
        return self.np_func(path)

    @property
    def inv(self) -> Functional:
        return Identity()


@dtc.dataclass
class RemoveDC(Functional):
    """DC-blocking one-pole filter of the extraction chain (reference :216-233): b = [1, -1], a = [1, -0.99].
    The torch path runs that filter - the one of ``np_func`` - as a HIP kernel.  The reference's own torch path (:226-229) hands
    ``lfilter`` its arguments in the wrong order (the coefficient vectors where the waveform belongs) and fails for every (B, T)
    input, so there is no torch behaviour of the reference to differ from."""

    def np_func(self, inputs):
        from scipy.signal import lfilter
        return lfilter([1.0, -1.0], [1.0, -0.99], inputs, axis=-1).astype(inputs.dtype)

    def torch_func(self, inputs):
        from .. import native
        return native.lfilter1(inputs, 1.0, -1.0, -0.99)

    @property
    def inv(self) -> Functional:
        return Identity()


@dtc.dataclass
class Emphasis(Functional):
    """reference :256-271: y[n] = x[n] - emphasis x[n-1] (torchaudio's lfilter with b = [1, -e], a = [1, 0] on the torch path)"""
    emphasis: float = 0.

    def np_func(self, inputs):
        from scipy.signal import lfilter
        return lfilter([1, -self.emphasis], [1], inputs).astype(inputs.dtype)

    def torch_func(self, inputs):
        from .. import native
        return native.lfilter1(inputs, 1.0, -self.emphasis, 0.0)

    @property
    def inv(self) -> Functional:
        return Deemphasis(self.emphasis)


@dtc.dataclass
class Deemphasis(Functional):
    """reference :274-288: y[n] = (1 - emphasis) x[n] + emphasis y[n-1] (b = [1 - e, 0], a = [1, -e]).  With the gain 1 - e this
    is not the exact inverse of Emphasis: Deemphasis(e)(Emphasis(e)(x)) = (1 - e) x, as in the reference."""
    emphasis: float = 0.

    def np_func(self, inputs):
        from scipy.signal import lfilter
        return lfilter([1 - self.emphasis], [1, -self.emphasis], inputs).astype(inputs.dtype)

    def torch_func(self, inputs):
        from .. import native
        return native.lfilter1(inputs, 1 - self.emphasis, 0.0, -self.emphasis)

    @property
    def inv(self) -> Functional:
        return Emphasis(self.emphasis)


@functools.lru_cache(maxsize=16)
def resample_filter_bank(orig_sr: int, target_sr: int, lowpass_filter_width: int = 6, rolloff: float = 0.99):
    """(orig, new, width, table (new, 2 width + orig) fp32): the Hann-windowed sinc filter bank of
    torchaudio.functional.resample (2.0.1: ``_get_sinc_resample_kernel``, sinc_interp_hann, computed in float64), built with
    torch ops on the host - a filter table like the FFT's twiddles, not a data path."""
    import math
    g = math.gcd(int(orig_sr), int(target_sr))
    orig, new = int(orig_sr) // g, int(target_sr) // g
    base_freq = min(orig, new) * rolloff
    width = math.ceil(lowpass_filter_width * orig / base_freq)
    idx = torch.arange(-width, width + orig, dtype=torch.float64)[None, None] / orig
    t = torch.arange(0, -new, -1, dtype=torch.float64)[:, None, None] / new + idx
    t = (t * base_freq).clamp_(-lowpass_filter_width, lowpass_filter_width)
    window = torch.cos(t * math.pi / lowpass_filter_width / 2) ** 2
    t = t * math.pi
    scale = base_freq / orig
    kernels = torch.where(t == 0, torch.tensor(1.0, dtype=torch.float64), t.sin() / t)
    kernels = kernels * window * scale
    return orig, new, width, kernels.reshape(new, 2 * width + orig).to(torch.float32).contiguous()


_RESAMPLE_TABLES = {}


@dtc.dataclass
class Resample(Functional):
    """reference :292-310.  The torch path is ``torchaudio.functional.resample`` there; here its polyphase windowed-sinc
    filter runs as a HIP kernel (``csrc/features.hip``).  Parity is UNPINNED (torchaudio is not installed in the build
    container): the oracle restates torchaudio 2.0.1's published algorithm, see DESIGN.md section 4."""
    orig_sr: int = SR
    target_sr: int = 16000

    @property
    def unit(self) -> Optional[Unit]:
        return Sample(self.target_sr)

    def np_func(self, inputs):
        raise NotImplementedError("the numpy path of Resample is librosa's soxr resampler (dataset preparation, out of scope)")

    def torch_func(self, inputs):
        from .. import native
        native.require_device(inputs)
        if int(self.orig_sr) == int(self.target_sr):
            return inputs
        orig, new, width, table = resample_filter_bank(int(self.orig_sr), int(self.target_sr))
        key = (int(self.orig_sr), int(self.target_sr), str(inputs.device))
        if key not in _RESAMPLE_TABLES:
            _RESAMPLE_TABLES[key] = table.to(inputs.device)
        return native.resample(inputs, _RESAMPLE_TABLES[key], orig, new, width)

    @property
    def inv(self) -> Functional:
        return Resample(self.target_sr, self.orig_sr)


@dtc.dataclass
class Normalize(Functional):
    p: float = float("inf")
    dim: int = -1

    @property
    def elem_type(self) -> Optional[EventType]:
        return Continuous(-1., 1., 1)

    def np_func(self, inputs):
        norm = np.linalg.norm(inputs, ord=self.p, axis=self.dim, keepdims=True)
        return (inputs / np.maximum(norm, np.finfo(inputs.dtype).tiny)).astype(inputs.dtype)

    def torch_func(self, inputs):
        """reference :248-249: torch.nn.functional.normalize(inputs, p, dim) (eps 1e-12); over the last dimension for p in {inf, 1, 2}"""
        from .. import native
        if not isinstance(inputs, torch.Tensor) or inputs.dim() == 0 or self.dim not in (-1, inputs.dim() - 1):
            raise NotImplementedError(f"Normalize(dim={self.dim}) is not on the HIP path: the last dimension only")
        if self.p not in native.NORM_ORDERS:
            raise NotImplementedError(f"Normalize(p={self.p}) is not on the HIP path: p in (inf, 1, 2) only")
        return native.row_normalize(inputs, self.p)

    @property
    def inv(self) -> Functional:
        return Identity()


# ---------------------------------------------------------------------------
# mu-law
# ---------------------------------------------------------------------------
def _mulaw_formula_cpu(x: torch.Tensor, q_levels: int, compression: float) -> torch.Tensor:
    """The reference quantisation formula (:330-338), fp32 torch ops on the host.
    Used ONLY to derive the decision-threshold table the kernel quantises with."""
    mu = torch.tensor(q_levels - 1.0, dtype=torch.float32)
    c = torch.tensor(compression, dtype=torch.float32)
    y = torch.sign(x) * torch.log1p(mu * torch.abs(x) * c) / torch.log1p(mu * c)
    return ((y + 1) / 2 * mu + 0.5).to(torch.int64)


def _ordered_key(x: torch.Tensor) -> torch.Tensor:
    """monotone int64 key of fp32 values"""
    bits = x.view(torch.int32).to(torch.int64)
    return torch.where(bits >= 0, bits, -(bits & 0x7FFFFFFF))


def _from_key(k: torch.Tensor) -> torch.Tensor:
    bits = torch.where(k >= 0, k, (-k) | 0x80000000)
    bits = torch.where(bits >= 2 ** 31, bits - 2 ** 32, bits)
    return bits.to(torch.int32).view(torch.float32)


@functools.lru_cache(maxsize=16)
def mulaw_edges(q_levels: int, compression: float) -> torch.Tensor:
    """edges[c-1] = smallest fp32 x in [-1, 1] whose reference code is >= c (c = 1..q-1).
    Found by bisection over the fp32 number line against the formula above, so the
    kernel's table quantiser reproduces the reference's own rounding at every bin edge."""
    n = q_levels - 1
    targets = torch.arange(1, q_levels, dtype=torch.int64)
    lo = _ordered_key(torch.full((n,), -1.0))   # code(lo) < c
    hi = _ordered_key(torch.full((n,), 1.0))    # code(hi) >= c
    pad = (-n) % 16 + 16                        # keep the evaluation in torch's vectorised loop
    for _ in range(34):
        mid = (lo + hi) // 2
        x = _from_key(torch.cat([mid, mid[-1:].expand(pad)]))
        code = _mulaw_formula_cpu(x, q_levels, compression)[:n]
        ge = code >= targets
        hi = torch.where(ge, mid, hi)
        lo = torch.where(ge, lo, mid)
    return _from_key(hi).contiguous()


@functools.lru_cache(maxsize=16)
def mulaw_table(q_levels: int, compression: float) -> torch.Tensor:
    """expanded value of every in-range code (reference :361-369), fp32 torch ops on the host"""
    codes = torch.arange(q_levels, dtype=torch.float32)
    mu = torch.tensor(q_levels - 1.0, dtype=torch.float32)
    c = torch.tensor(compression, dtype=torch.float32)
    x = (codes / mu) * 2 - 1.0
    return (torch.sign(x) * (torch.exp(torch.abs(x) * torch.log1p(mu * c)) - 1.0) / (mu * c)).contiguous()


_DEVICE_TABLES = {}


def _device_table(kind: str, q_levels: int, compression: float, device) -> torch.Tensor:
    key = (kind, q_levels, float(compression), str(device))
    if key not in _DEVICE_TABLES:
        host = mulaw_edges(q_levels, float(compression)) if kind == "edges" else mulaw_table(q_levels, float(compression))
        _DEVICE_TABLES[key] = host.to(device)
    return _DEVICE_TABLES[key]


@dtc.dataclass
class MuLawCompress(Functional):
    q_levels: int = Q_LEVELS
    compression: float = 1.

    @property
    def elem_type(self) -> Optional[EventType]:
        return Discrete(self.q_levels)

    def np_func(self, inputs):
        mu = self.q_levels - 1.0
        y = np.sign(inputs) * np.log1p(mu * np.abs(inputs) * self.compression) / np.log1p(mu * self.compression)
        return ((y + 1) / 2 * mu + 0.5).astype(np.int64)

    def torch_func(self, inputs):
        from .. import native
        native.require_device(inputs)
        edges = _device_table("edges", self.q_levels, self.compression, inputs.device)
        return native.mulaw_compress(inputs, self.q_levels, float(self.compression), edges)

    @property
    def inv(self) -> Functional:
        return MuLawExpand(self.q_levels, self.compression)


@dtc.dataclass
class MuLawExpand(Functional):
    q_levels: int = Q_LEVELS
    compression: float = 1.

    @property
    def elem_type(self) -> Optional[EventType]:
        return Continuous(-1., 1., 1)

    def np_func(self, inputs):
        mu = self.q_levels - 1.0
        x = (inputs / mu) * 2 - 1.0
        return np.sign(x) * (np.exp(np.abs(x) * np.log1p(mu * self.compression)) - 1.0) / (mu * self.compression)

    def torch_func(self, inputs):
        from .. import native
        native.require_device(inputs)
        if inputs.is_floating_point():
            raise TypeError("MuLawExpand on the HIP path takes integer class indices")
        table = _device_table("table", self.q_levels, self.compression, inputs.device)
        return native.mulaw_expand(inputs, self.q_levels, float(self.compression), table)

    @property
    def inv(self) -> Functional:
        return MuLawCompress(self.q_levels, self.compression)


# ---------------------------------------------------------------------------
# STFT family
# ---------------------------------------------------------------------------
@dtc.dataclass
class STFT(Functional):
    n_fft: int = N_FFT
    hop_length: int = HOP_LENGTH
    coordinate: str = "pol"
    center: bool = True
    window: Optional[str] = "hann"
    pad_mode: str = "constant"
    alignment: Optional[str] = "end"

    @property
    def unit(self) -> Optional[Unit]:
        return Frame(self.n_fft, self.hop_length, padding=self.center)

    @property
    def elem_type(self) -> Optional[EventType]:
        return Continuous(0., float("inf"), 1 + self.n_fft // 2)

    def fixed_length(self, n_samples: int) -> int:
        """number of samples kept by the reference's ``_fix_length`` (:468-486)"""
        n_frames = convert(n_samples, Sample(1), self.unit, as_length=True) + int(self.center)
        return convert(n_frames, self.unit, Sample(1), as_length=True)

    def _fix_length(self, inputs):
        if self.alignment is None:
            return inputs
        keep = self.fixed_length(inputs.shape[-1])
        if self.alignment == "end":
            return inputs[..., -keep:]
        if self.alignment == "start":
            return inputs[..., :keep]
        return inputs

    def np_func(self, inputs):
        raise NotImplementedError("the numpy (librosa) STFT belongs to dataset extraction; use the torch path on the HIP device")

    def torch_func(self, inputs):
        from .. import native
        native.require_device(inputs)
        # the reference ignores self.window on the torch path and always applies a periodic Hann (:513)
        inputs = self._fix_length(inputs)
        if self.coordinate == "mag" and self.pad_mode == "constant":
            return native.stft_mag(inputs, self.n_fft, self.hop_length, bool(self.center))
        if self.coordinate in native.STFT_COORDINATES:
            return native.stft(inputs, self.n_fft, self.hop_length, bool(self.center), self.pad_mode, self.coordinate)
        if self.coordinate == "mag":
            return native.stft(inputs, self.n_fft, self.hop_length, bool(self.center), self.pad_mode, "pol")[..., 0]
        raise ValueError(f"unknown STFT coordinate '{self.coordinate}'")

    @property
    def inv(self) -> Functional:
        return ISTFT(self.n_fft, self.hop_length, self.coordinate, self.center, self.window)


@dtc.dataclass
class ISTFT(Functional):
    n_fft: int = N_FFT
    hop_length: int = HOP_LENGTH
    coordinate: str = "pol"
    center: bool = True
    window: Optional[str] = None
    pad_mode: str = "constant"

    @property
    def unit(self) -> Optional[Unit]:
        return Sample(None)

    @property
    def elem_type(self) -> Optional[EventType]:
        return Continuous(-1., 1., 1)

    def np_func(self, inputs):
        raise NotImplementedError("the numpy (librosa) ISTFT belongs to dataset extraction; use the torch path on the HIP device")

    def torch_func(self, inputs):
        """reference :553-564: torch.istft with torch's defaults -- ``self.center`` and ``self.window`` are ignored
        there (centre trimming always on, periodic Hann always applied), and so they are here."""
        from .. import native
        native.require_device(inputs)
        if self.coordinate == "pol":
            return native.istft(inputs, self.n_fft, self.hop_length, polar=True)
        if self.coordinate == "car":
            # the reference forms ``inputs[..., 0] * (1j * inputs[..., 1])`` (:558): a purely imaginary spectrum
            # whose imaginary part is the PRODUCT of the two planes.  Kept as is.
            prod = inputs[..., 0] * inputs[..., 1]
            return native.istft(torch.stack((torch.zeros_like(prod), prod), dim=-1), self.n_fft, self.hop_length, polar=False)
        raise RuntimeError(f"ISTFT: coordinate '{self.coordinate}' leaves a real tensor, torch.istft (and this path) "
                           "needs a complex spectrum ('pol' or 'car')")

    @property
    def inv(self) -> Functional:
        return STFT(self.n_fft, self.hop_length, self.coordinate, self.center, self.window, self.pad_mode)


@dtc.dataclass
class MagSpec(Functional):
    n_fft: int = N_FFT
    hop_length: int = HOP_LENGTH
    center: bool = True
    window: Optional[str] = "hann"
    pad_mode: str = "constant"
    alignment: Optional[str] = "end"

    @property
    def stft(self) -> STFT:
        return STFT(self.n_fft, self.hop_length, "mag", self.center, self.window, self.pad_mode, alignment=self.alignment)

    @property
    def unit(self) -> Optional[Unit]:
        return Frame(self.n_fft, self.hop_length, padding=self.center)

    @property
    def elem_type(self) -> Optional[EventType]:
        return Continuous(0., float("inf"), 1 + self.n_fft // 2)

    def np_func(self, inputs):
        return self.stft.np_func(inputs)

    def torch_func(self, inputs):
        return self.stft.torch_func(inputs)

    @property
    def inv(self) -> Functional:
        return GLA(self.n_fft, self.hop_length, self.center, self.window, self.pad_mode)


@dtc.dataclass
class GLA(Functional):
    n_fft: int = N_FFT
    hop_length: int = HOP_LENGTH
    center: bool = True
    window: Optional[str] = None
    pad_mode: str = "constant"
    n_iter: int = 32

    @property
    def unit(self) -> Optional[Unit]:
        return Sample(None)

    @property
    def elem_type(self) -> Optional[EventType]:
        return Continuous(-1., 1., 1)

    def np_func(self, inputs):
        raise NotImplementedError("the numpy (librosa) Griffin-Lim belongs to dataset extraction; use the torch path on the HIP device")

    # torchaudio.transforms.GriffinLim defaults; the reference does not forward ``self.n_iter`` on the torch path (:637)
    TORCH_N_ITER = 32
    TORCH_MOMENTUM = 0.99

    def torch_func(self, inputs, init=None):
        """reference :634-642: torchaudio's GriffinLim(n_fft, hop_length, power=1.) over (time x freq) magnitudes with
        its defaults: 32 iterations, momentum 0.99, random initial phases (``torch.rand`` of a complex dtype).  ``init``
        lets a caller (the parity tests) supply those initial estimates instead of drawing them."""
        from .. import native
        native.require_device(inputs)
        if init is None:
            init = torch.rand(inputs.shape, dtype=torch.complex64, device=inputs.device)
        return native.griffin_lim(inputs, self.n_fft, self.hop_length, self.TORCH_N_ITER, self.TORCH_MOMENTUM, init)

    @property
    def inv(self) -> Functional:
        return MagSpec(self.n_fft, self.hop_length, self.center, self.window, self.pad_mode)


# ---------------------------------------------------------------------------
# envelope followers
# ---------------------------------------------------------------------------
def get_metadata(x, key: str, default=None):
    """reference :143-147: the metadata of a numpy dtype, or an attribute of any other array"""
    if isinstance(x, np.ndarray):
        return dict(x.dtype.metadata or {}).get(key, default)
    return getattr(x, key, default)


@dtc.dataclass
class Interpolate(Functional):
    """reference :867-916.  On a device tensor the last axis is resampled by ``native.interp1d``: ``mode="linear"`` at the positions of
    ``torch.nn.functional.interpolate(mode="linear")`` (align_corners=False), with the reference's ``.squeeze()`` of the result;
    ``mode="previous"`` at scipy's positions ``np.linspace(0, n - 1, N)`` - the reference sends every non-linear mode through scipy on
    the host and moves the result back, here it stays on the device; ``mode="quadratic"`` is scipy's interpolating spline at the same
    positions (``native.spline2_coef`` / ``native.spline2_eval``: not-a-knot ends, float64 inside, at least 3 points).  Other modes and
    other axes raise NotImplementedError."""
    axis: int = -1
    mode: str = "linear"
    length: Optional[int] = None
    factor: Optional[int] = None
    metadata_key: str = "n_samples"

    @property
    def unit(self) -> Optional[Unit]:
        return None

    @property
    def elem_type(self) -> Optional[EventType]:
        return Continuous(-float("inf"), float("inf"), 1)

    @property
    def inv(self) -> Functional:
        return Identity()

    def _get_target_length(self, x):
        if self.length is not None:
            return self.length
        if self.factor is not None:
            return self.factor * x.shape[self.axis]
        n = get_metadata(x, self.metadata_key)
        if n is None:
            raise ValueError("No target length provided. One of length or factor must not be None,"
                             f" or inputs must have the metadata key {self.metadata_key}")
        return n

    def np_func(self, inputs):
        from scipy.interpolate import interp1d
        n_in = inputs.shape[self.axis]
        f = interp1d(np.arange(n_in), inputs, kind=self.mode, axis=self.axis, assume_sorted=True, copy=False)
        return f(np.linspace(0, n_in - 1, self._get_target_length(inputs))).astype(inputs.dtype)

    def torch_func(self, inputs):
        from .. import native
        if self.mode not in native.INTERP_MODES and self.mode != "quadratic":
            raise NotImplementedError(f"Interpolate(mode='{self.mode}') is not on the HIP path: 'linear', 'previous' or 'quadratic'")
        if not isinstance(inputs, torch.Tensor) or inputs.dim() == 0 or self.axis not in (-1, inputs.dim() - 1):
            raise NotImplementedError(f"Interpolate(axis={self.axis}) is not on the HIP path: the last axis only")
        n_out = self._get_target_length(inputs)
        if self.mode == "linear":
            return native.interp1d(inputs, n_out, "linear", align=False).squeeze()
        if self.mode == "quadratic":
            return native.spline2_eval(native.spline2_coef(inputs), n_out)
        return native.interp1d(inputs, n_out, "previous", align=True)


@dtc.dataclass
class Derivative(Functional):
    """reference :931-1004: the mean over lags 1 .. max_lag of the centred differences, over the last axis, for any leading dimensions
    (``native.derivative``; ``max_lag`` up to ``native.DERIV_MAX_LAG``, rows longer than ``max_lag``).  The reference's
    ``derivative_torch`` takes 1-D input only (its reflection does not broadcast over a batch); rows are taken one by one here, as
    ``derivative_np_2d`` takes them.

    ``normalize=True`` divides each row by its largest magnitude (``native.row_normalize(p=inf)``).  That is the meaning of the numpy
    path: the reference's torch path fails for it (``abs(g).max(dim=-1, keepdims=True)`` is a (values, indices) tuple, and a tensor
    cannot be divided by one).  A row whose derivative is zero everywhere gives zeros where numpy gives NaN (0 / 0), because
    ``row_normalize`` clamps the divisor at 1e-12."""
    max_lag: int = 3
    normalize: bool = False

    @property
    def unit(self) -> Optional[Unit]:
        return None

    @property
    def elem_type(self) -> Optional[EventType]:
        return Continuous(-float("inf"), float("inf"), 1)

    def np_func(self, inputs):
        """derivative_np (:931-957) in plain numpy, without numba: float32 throughout (a Python scalar does not widen a float32 array),
        the lag terms added in lag order; 1-D or 2-D input"""
        if inputs.ndim not in (1, 2):
            raise ValueError(f"Expected input array to have 1 or 2 dimensions. Got {inputs.ndim}")
        y = np.asarray(inputs, dtype=np.float32)
        n = y.shape[-1]
        grads = np.zeros(y.shape, dtype=np.float32)
        for lag in range(1, self.max_lag + 1):
            y_p = np.zeros(y.shape[:-1] + (n + 2 * lag,), dtype=np.float32)
            y_p[..., lag:-lag] = y
            y_p[..., :lag] = y[..., :1] + (y[..., :1] - y[..., 1:1 + lag])[..., ::-1]
            y_p[..., -lag:] = y[..., -1:] + (y[..., -1:] - y[..., -lag - 1:-1])[..., ::-1]
            a, b = y_p[..., :n], y_p[..., 2 * lag:]
            g = (1 / lag) * ((b - y) + (y - a)) / 2
            grads += g / self.max_lag
        if self.normalize:
            grads /= abs(grads).max(axis=-1, keepdims=True)
        return grads

    def torch_func(self, inputs):
        from .. import native
        g = native.derivative(inputs, self.max_lag)
        if self.normalize:
            g = native.row_normalize(g, float("inf"))
        return g

    @property
    def inv(self) -> Functional:
        return Identity()


@dtc.dataclass
class Envelop(Functional):
    """reference :794-830: the sum over the bins of a reflect-padded magnitude spectrogram, interpolated back to the time domain and
    divided by its maximum.  On the device: ``STFT._fix_length`` of ``MagSpec(n_fft, hop, center=True, pad_mode="reflect")``
    (alignment "end"), ``native.stft_energy`` (one float per frame; the spectrogram is never written), ``native.interp1d`` at scipy's
    positions (the reference's torch path IS its numpy path: ``Interpolate(length=T)`` through scipy, T the length before
    ``_fix_length``) and ``native.row_normalize(p=inf)``.

    Deviations from the reference: the result is a float32 tensor on the input's device, not a CPU tensor; a ``(B, T)`` input is taken
    row by row (the reference takes ``(T,)`` only); a silent row gives zeros where the reference gives NaN (0 / 0: ``row_normalize``
    clamps the divisor at 1e-12); ``n_fft`` is a power of two in [64, 4096]; ``window`` is ignored, the periodic Hann window of the
    torch STFT is always applied."""
    n_fft: int = N_FFT
    hop_length: int = HOP_LENGTH
    normalize: bool = True
    window: str = "hann"
    interp_to_time_domain: bool = True

    @property
    def fft(self) -> MagSpec:
        return MagSpec(self.n_fft, self.hop_length, center=True, window=self.window, pad_mode="reflect")

    @property
    def unit(self) -> Optional[Unit]:
        return Sample(None) if self.interp_to_time_domain else self.fft.unit

    @property
    def elem_type(self) -> Optional[EventType]:
        return Continuous(0., 1. if self.normalize else float("inf"), 1)

    def np_func(self, inputs):
        return self.fft.np_func(inputs)          # (raises: the numpy MagSpec is librosa's)

    def torch_func(self, inputs):
        from .. import native
        native.require_device(inputs)
        if inputs.dim() not in (1, 2):
            raise ValueError(f"Envelop takes (T,) or (B, T), got shape {tuple(inputs.shape)}")
        n_samples = inputs.shape[-1]
        e = native.stft_energy(self.fft.stft._fix_length(inputs), self.n_fft, self.hop_length, True, "reflect")
        if self.interp_to_time_domain:
            e = native.interp1d(e, n_samples, "linear", align=True)
        if self.normalize:
            e = native.row_normalize(e, float("inf"))
        return e

    @property
    def inv(self) -> Functional:
        return Identity()


@dtc.dataclass
class EnvelopBank(Functional):
    """reference :833-864: the envelopes of several (n_fft, hop) pairs, always interpolated to the time domain, joined by
    ``torch.cat(dim=-1)``.  That follows the reference's ``np.hstack``, which for 1-D envelopes is a concatenation along time - a
    ``(len(n_fft) * T,)`` result - whatever the ``elem_type.size`` of ``len(n_fft)`` suggests."""
    n_fft: Tuple[int, ...] = (N_FFT,)
    hop_length: Tuple[int, ...] = (HOP_LENGTH,)
    normalize: bool = True

    @property
    def envelops(self):
        return tuple(Envelop(n_fft, hop, self.normalize, interp_to_time_domain=True) for n_fft, hop in zip(self.n_fft, self.hop_length))

    @property
    def unit(self) -> Optional[Unit]:
        return Sample(None)

    @property
    def elem_type(self) -> Optional[EventType]:
        return Continuous(0., 1. if self.normalize else float("inf"), len(self.envelops))

    def np_func(self, inputs):
        return np.hstack([e(inputs) for e in self.envelops])

    def torch_func(self, inputs):
        return torch.cat([e(inputs) for e in self.envelops], dim=-1)

    @property
    def inv(self) -> Functional:
        return Identity()


@dtc.dataclass
class PCA(Functional):
    """reference :1114-1138: ``sklearn.decomposition.PCA(n_components).fit_transform(StandardScaler().fit_transform(x))`` for (N, D) float32
    frames on the device, computed in float64 and returned as (N, n_components) float32 scores (``csrc/pca.hip``):

        native.pca_colstats   mean and population standard deviation of every bin (a constant bin gets scale 1, by sklearn's rule), with the
                              mean sklearn's PCA subtracts after the scaler folded in
        native.pca_cov        C = Z^T Z / (N - 1), Z = (x - mean_) / scale_, by v_mfma_f64_16x16x4_f64; Z is never written
        native.pca_eig        the n_components leading eigenvectors of C by block subspace iteration (no D x D eigendecomposition); waits for
                              the stream every 8 iterations
        native.pca_project    Z components_^T

    The sign of a component makes its entry of largest magnitude positive: the ``svd_flip(u_based_decision=False)`` of sklearn 1.5 and
    later (older versions decide by the scores' largest entry, and may return a component and its scores negated).  A component whose
    eigenvalue is below the solver's resolution (the rank of the frames is below n_components) is some unit vector of C's null space,
    as it is in sklearn; its scores are zero to about 1e-8 of the largest score.  ``random_seed`` is kept for the YAML form and unused:
    nothing here is random.  ``fit`` stores ``mean_``, ``scale_``, ``components_`` (n_components, D), ``explained_variance_`` (float64,
    on the device) and ``n_iter_`` (int); ``transform`` projects any (M, D) float32 device tensor with them."""
    n_components: int = 16
    random_seed: int = 42

    def __post_init__(self):
        self.mean_: Optional[torch.Tensor] = None
        self.scale_: Optional[torch.Tensor] = None
        self.components_: Optional[torch.Tensor] = None
        self.explained_variance_: Optional[torch.Tensor] = None
        self.n_iter_: Optional[int] = None

    @property
    def unit(self) -> Optional[Unit]:
        return None

    @property
    def elem_type(self) -> Optional[EventType]:
        return None

    @staticmethod
    def _frames(x, what: str) -> torch.Tensor:
        if not isinstance(x, torch.Tensor):
            raise TypeError(f"{what}: expected a torch.Tensor, got {type(x)}")
        if x.dtype != torch.float32:
            raise TypeError(f"{what} takes float32 frames on the HIP path, got {x.dtype}")
        if x.dim() != 2 or x.shape[1] < 1:
            raise ValueError(f"{what}: x must be (N, D >= 1) frames, got shape {tuple(x.shape)}")
        return x

    def fit(self, x: torch.Tensor) -> "PCA":
        from .. import native
        x = self._frames(x, "PCA")
        n, d = x.shape
        k = int(self.n_components)
        if n < 2:
            raise ValueError(f"PCA: N = {n} frames, at least 2 are needed (the covariance divides by N - 1)")
        if not 1 <= k <= min(n, d):
            raise ValueError(f"PCA: n_components = {k} must lie in [1, min(N, D) = {min(n, d)}]")
        if d > native.PCA_MAX_D:
            raise NotImplementedError(f"PCA: D = {d} bins, the limit of the HIP path is {native.PCA_MAX_D} (native.PCA_MAX_D)")
        if k > native.PCA_MAX_COMPONENTS:
            raise NotImplementedError(f"PCA: n_components = {k}, the limit of the HIP path is {native.PCA_MAX_COMPONENTS} "
                                      "(native.PCA_MAX_COMPONENTS)")
        native.require_device(x)
        self.mean_, self.scale_ = native.pca_colstats(x)
        c = native.pca_cov(x, self.mean_, self.scale_)
        self.components_, self.explained_variance_, self.n_iter_ = native.pca_eig(c, k)
        return self

    def transform(self, y: torch.Tensor) -> torch.Tensor:
        from .. import native
        if self.components_ is None:
            raise RuntimeError("PCA.transform before PCA.fit")
        y = self._frames(y, "PCA.transform")
        if y.shape[0] < 1 or y.shape[1] != self.mean_.shape[0]:
            raise ValueError(f"PCA.transform: y must be (M >= 1, D = {self.mean_.shape[0]}), got shape {tuple(y.shape)}")
        native.require_device(y)
        return native.pca_project(y, self.mean_, self.scale_, self.components_)

    def np_func(self, inputs):
        raise NotImplementedError("PCA runs on device tensors only (csrc/pca.hip): pass a float32 tensor on the HIP device; this package has "
                                  "no CPU path")

    def torch_func(self, inputs):
        return self.fit(inputs).transform(inputs)

    @property
    def inv(self) -> Functional:
        return Identity()


@dtc.dataclass
class NMF(Functional):
    """reference :1141-1170: ``sklearn.decomposition.NMF(n_components, tol=tol, max_iter=max_iter).fit_transform(x)`` for (N, D) non-negative
    float32 frames on the device, computed in float64 and returned as W (N, n_components) float32 (``csrc/nmf.hip``, ``include/mmk_nmf.h``):

        native.nmf_start   sklearn's NNDSVDA start from the k leading eigenpairs of X^T X (``native.pca_cov``'s kernel with mean 0 and
                           scale 1, ``native.pca_eig``'s subspace iteration).  NNDSVD does not see the sign of a singular pair, so any
                           accurate top-k decomposition gives sklearn's start - where the frames have a spectral gap
        native.nmf_solve   the cyclic coordinate descent (no shuffle, no regularisation, Frobenius loss) with sklearn's stop rule
                           ``violation / violation_init <= tol`` held on the device; waits for the stream every 8 iterations

    ``torch_func`` / ``__call__`` are ``fit_transform``, NOT ``fit(x).transform(x)``: as in sklearn, ``transform`` solves for W again from
    zeros with ``components_`` fixed.  ``fit`` stores ``components_`` (n_components, D) float64 on the device and ``n_iter_`` (int).
    ``random_seed`` is kept for the YAML form and unused: sklearn's seed enters its randomised SVD only, whose result the start does not
    depend on beyond rounding (DESIGN.md 5.6.12 - frames without a spectral gap, such as white noise, are not pinned by sklearn itself).

    ValueError: a negative entry; n_components outside [1, min(N, D)] (sklearn starts at random there); n_components beyond the
    numerical rank of the frames (all-zero frames included: the reference's start is arbitrary there).  NotImplementedError: D >
    ``native.NMF_MAX_D``, n_components > ``native.NMF_MAX_COMPONENTS``.  Reaching ``max_iter`` with ``tol > 0`` warns, and then
    ``n_iter_ == max_iter``, as in sklearn.  Not built: the ``mu`` solver, other ``beta_loss``, regularisation, ``shuffle``, other
    ``init`` modes, ``reconstruction_err_``, NaN / inf handling."""
    n_components: int = 16
    tol: float = 1e-4
    max_iter: int = 200
    random_seed: int = 42

    def __post_init__(self):
        self.components_: Optional[torch.Tensor] = None
        self.n_iter_: Optional[int] = None

    @property
    def unit(self) -> Optional[Unit]:
        return None

    @property
    def elem_type(self) -> Optional[EventType]:
        return None

    def _check(self, x, what: str) -> torch.Tensor:
        x = PCA._frames(x, what)
        if int(self.max_iter) < 1 or not float(self.tol) >= 0.0:
            raise ValueError(f"{what}: max_iter = {self.max_iter} must be at least 1 and tol = {self.tol} 0 or above")
        return x

    def _warn(self, n_iter: int, what: str):
        if n_iter == int(self.max_iter) and float(self.tol) > 0:
            import warnings
            warnings.warn(f"{what}: maximum number of iterations {self.max_iter} reached. Increase it to improve convergence.", RuntimeWarning)

    def fit_transform(self, x: torch.Tensor) -> torch.Tensor:
        from .. import native
        x = self._check(x, "NMF")
        n, d = x.shape
        k = int(self.n_components)
        if not 1 <= k <= min(n, d):
            raise ValueError(f"NMF: n_components = {k} must lie in [1, min(N, D) = {min(n, d)}] (beyond it the reference starts at random)")
        if d > native.NMF_MAX_D:
            raise NotImplementedError(f"NMF: D = {d} bins, the limit of the HIP path is {native.NMF_MAX_D} (native.NMF_MAX_D)")
        if k > native.NMF_MAX_COMPONENTS:
            raise NotImplementedError(f"NMF: n_components = {k}, the limit of the HIP path is {native.NMF_MAX_COMPONENTS} "
                                      "(native.NMF_MAX_COMPONENTS)")
        if n < 2:
            raise ValueError(f"NMF: N = {n} frames, at least 2 are needed")
        native.require_device(x)
        w, ht, _, _, _ = native.nmf_start(x, k)
        self.n_iter_ = native.nmf_solve(x, w, ht, True, self.tol, self.max_iter)
        self.components_ = ht.t().contiguous()
        self._warn(self.n_iter_, "NMF")
        return w.to(torch.float32)

    def fit(self, x: torch.Tensor) -> "NMF":
        self.fit_transform(x)
        return self

    def transform(self, y: torch.Tensor) -> torch.Tensor:
        from .. import native
        if self.components_ is None:
            raise RuntimeError("NMF.transform before NMF.fit")
        y = self._check(y, "NMF.transform")
        k, d = self.components_.shape
        if y.shape[0] < 1 or y.shape[1] != d:
            raise ValueError(f"NMF.transform: y must be (M >= 1, D = {d}), got shape {tuple(y.shape)}")
        native.require_device(y)
        w = torch.zeros((y.shape[0], k), dtype=torch.float64, device=y.device)
        n_iter = native.nmf_solve(y, w, self.components_.t().contiguous(), False, self.tol, self.max_iter, check_nonneg=True)
        self._warn(n_iter, "NMF.transform")
        return w.to(torch.float32)

    def np_func(self, inputs):
        raise NotImplementedError("NMF runs on device tensors only (csrc/nmf.hip): pass a float32 tensor on the HIP device; this package has "
                                  "no CPU path")

    def torch_func(self, inputs):
        return self.fit_transform(inputs)

    @property
    def inv(self) -> Functional:
        return Identity()


@dtc.dataclass
class FactorAnalysis(Functional):
    """reference :1173-1203: ``sklearn.decomposition.FactorAnalysis(n_components, tol=tol, max_iter=max_iter).fit_transform(x)`` for (N, D)
    float32 frames on the device, computed in float64 (sklearn converts float32 frames itself) and returned as (N, n_components) float32
    scores (``csrc/factor_analysis.hip``, ``include/mmk_factor_analysis.h``).  sklearn's EM in Gram form: per step it needs the k leading
    singular values and right vectors of ``Xc / (sqrt(psi) sqrt(N))``, which are the k leading eigenpairs of ``S C S`` with
    ``C = Xc^T Xc / N`` and ``S = diag(1 / (sqrt(psi) + 1e-12))`` - so the frames are read once:

        native.pca_colstats          ``mean_``
        native.pca_cov               C (scale 1), by v_mfma_f64_16x16x4_f64, times (N - 1) / N
        native.fa_fit                the whole EM loop on the device: the PCA kernels' block subspace iteration on S C S, warm-started from
                                     one EM step to the next, the log-likelihood, sklearn's stop ``ll - old < tol`` and the psi update
        native.fa_transform_matrix   A = (I + Wpsi W^T)^-1 Wpsi by a Cholesky in one workgroup; ``transform`` is native.pca_project with A

    ``torch_func`` / ``__call__`` are ``fit(x).transform(x)``, which is what sklearn's ``fit_transform`` is for this estimator.  ``fit``
    stores ``mean_`` (D,), ``components_`` (n_components, D), ``noise_variance_`` (D,) and ``loglike_`` (n_iter_,) as float64 on the device
    and ``n_iter_`` (int).  The sign of a component makes its entry of largest magnitude positive (PCA's rule; sklearn's own sign is an
    artefact of its SVD).  ``random_seed`` is kept for the YAML form and unused: sklearn's seed enters its randomised SVD only, which
    approximates exactly the eigenpairs computed here.

    Known limit: where n_components exceeds the number of factors in the frames, S C S has no gap after its k-th eigenvalue (the noise
    eigenvalues all sit near 1); the subspace iteration converges slowly there and may reach its cap (a RuntimeError naming the EM step
    and the residual), and sklearn's own default (randomised) method does not reproduce its exact method there either.

    ValueError: N < 2, n_components outside [1, min(N, D)].  NotImplementedError: D > ``native.PCA_MAX_D``, n_components >
    ``native.PCA_MAX_COMPONENTS``.  Running out of ``max_iter`` warns (RuntimeWarning); then ``n_iter_ == max_iter`` and
    ``noise_variance_`` is the psi updated after the last W, as sklearn's ``for ... else`` leaves it.  Not built: ``rotation``,
    ``noise_variance_init``, ``score``, ``get_covariance``."""
    n_components: int = 16
    tol: float = 1e-2
    max_iter: int = 1000
    random_seed: int = 42

    def __post_init__(self):
        self.mean_: Optional[torch.Tensor] = None
        self.components_: Optional[torch.Tensor] = None
        self.noise_variance_: Optional[torch.Tensor] = None
        self.loglike_: Optional[torch.Tensor] = None
        self.n_iter_: Optional[int] = None
        self._ones: Optional[torch.Tensor] = None
        self._matrix: Optional[torch.Tensor] = None

    @property
    def unit(self) -> Optional[Unit]:
        return None

    @property
    def elem_type(self) -> Optional[EventType]:
        return None

    def fit(self, x: torch.Tensor) -> "FactorAnalysis":
        from .. import native
        x = PCA._frames(x, "FactorAnalysis")
        n, d = x.shape
        k = int(self.n_components)
        if int(self.max_iter) < 1 or not float(self.tol) >= 0.0:
            raise ValueError(f"FactorAnalysis: max_iter = {self.max_iter} must be at least 1 and tol = {self.tol} 0 or above")
        if n < 2:
            raise ValueError(f"FactorAnalysis: N = {n} frames, at least 2 are needed")
        if not 1 <= k <= min(n, d):
            raise ValueError(f"FactorAnalysis: n_components = {k} must lie in [1, min(N, D) = {min(n, d)}]")
        if d > native.PCA_MAX_D:
            raise NotImplementedError(f"FactorAnalysis: D = {d} bins, the limit of the HIP path is {native.PCA_MAX_D} (native.PCA_MAX_D)")
        if k > native.PCA_MAX_COMPONENTS:
            raise NotImplementedError(f"FactorAnalysis: n_components = {k}, the limit of the HIP path is {native.PCA_MAX_COMPONENTS} "
                                      "(native.PCA_MAX_COMPONENTS)")
        native.require_device(x)
        mean, _ = native.pca_colstats(x)
        ones = torch.ones((d,), dtype=torch.float64, device=x.device)
        c = native.pca_cov(x, mean, ones) * ((n - 1) / n)
        components, noise, loglike, n_iter, converged, _ = native.fa_fit(c, n, k, self.tol, self.max_iter)
        self.mean_, self.components_, self.noise_variance_, self.loglike_, self.n_iter_, self._ones = mean, components, noise, loglike, n_iter, ones
        self._matrix = native.fa_transform_matrix(components, noise)
        if not converged:
            import warnings
            warnings.warn(f"FactorAnalysis did not converge: maximum number of iterations {self.max_iter} reached. You might want to increase it.",
                          RuntimeWarning)
        return self

    def transform(self, y: torch.Tensor) -> torch.Tensor:
        from .. import native
        if self.components_ is None:
            raise RuntimeError("FactorAnalysis.transform before FactorAnalysis.fit")
        y = PCA._frames(y, "FactorAnalysis.transform")
        if y.shape[0] < 1 or y.shape[1] != self.mean_.shape[0]:
            raise ValueError(f"FactorAnalysis.transform: y must be (M >= 1, D = {self.mean_.shape[0]}), got shape {tuple(y.shape)}")
        native.require_device(y)
        return native.pca_project(y, self.mean_, self._ones, self._matrix)

    def fit_transform(self, x: torch.Tensor) -> torch.Tensor:
        return self.fit(x).transform(x)

    def np_func(self, inputs):
        raise NotImplementedError("FactorAnalysis runs on device tensors only (csrc/factor_analysis.hip): pass a float32 tensor on the HIP "
                                  "device; this package has no CPU path")

    def torch_func(self, inputs):
        return self.fit(inputs).transform(inputs)

    @property
    def inv(self) -> Functional:
        return Identity()


# ---------------------------------------------------------------------------
# harmonic / percussive separation
# ---------------------------------------------------------------------------
@dtc.dataclass
class _HPSSSource(Functional):
    """reference :736-791: ``librosa.decompose.hpss(S=inputs.T, kernel_size, power, margin)[which].T`` of (T, F) or (B, T, F) non-negative
    float32 magnitudes on the device, as one launch of ``native.hpss`` asking for the one output: the running median of every bin along
    time and of every frame along frequency (scipy's ``median_filter(mode="reflect")``, bit for bit), librosa's soft masks, the product.
    ``kernel_size`` and ``margin`` are a scalar or a pair (harmonic, percussive), as librosa takes them.

    Differences from librosa: windows up to ``native.HPSS_MAX_KERNEL``; an axis shorter than half its window raises (scipy reflects it
    more than once there); real input only (no ``magphase`` branch); negative or NaN bins are not looked for - librosa raises on
    negative ones, here their results are unspecified; a batch is separated clip by clip."""
    kernel_size: Union[int, Tuple[int, int]] = 31
    power: float = 1.
    margin: Union[float, Tuple[float, float]] = 1.

    _which = 0

    @property
    def unit(self) -> Optional[Unit]:
        return None

    @property
    def elem_type(self) -> Optional[EventType]:
        return None

    def np_func(self, inputs):
        raise NotImplementedError("the numpy (librosa) HPSS belongs to dataset extraction; use the torch path on the HIP device")

    def torch_func(self, inputs):
        from .. import native
        return native.hpss(inputs, self.kernel_size, self.power, self.margin, harmonic=self._which == 0, percussive=self._which == 1)[0]

    @property
    def inv(self) -> Functional:
        return Identity()


@dtc.dataclass
class HarmonicSource(_HPSSSource):
    _which = 0


@dtc.dataclass
class PercussiveSource(_HPSSSource):
    _which = 1


# ---------------------------------------------------------------------------
# nearest-neighbour filter
# ---------------------------------------------------------------------------
@dtc.dataclass
class NearestNeighborFilter(Functional):
    """reference :1083-1111: ``librosa.decompose.nn_filter(inputs, aggregate=getattr(np, aggregate), metric=metric, sym=True, sparse=True,
    k=n_neighbors, axis=0)`` of (T, F) or (B, T, F) float32 frames on the device.  librosa is not installed where this was written: what
    follows restates the published ``librosa.segment.recurrence_matrix`` (width 1, connectivity mode, ``sym=True``) and ``nn_filter`` from
    memory.  Every frame is replaced, bin by bin, by the aggregate of the frames that are among its k nearest other frames AND have it among
    theirs; a frame without such a neighbour keeps its values.  Two launches: ``native.nn_topk(x, x, min(n_neighbors, T - 1), metric,
    self_exclude=True)`` and ``native.nn_aggregate`` (``csrc/nn_filter.hip``), behind nn_topk's norm / shift helpers; nothing is read back
    and the (T, k, F) block of neighbour frames is never written.  ``aggregate`` is one of ``native.NN_AGGREGATES``; a batch is filtered
    clip by clip, neighbours never cross clips.

    Differences from librosa:
      * librosa asks sklearn for min(T - 1, k + 2) neighbours and then keeps "the k closest" by an argsort of the stored values, which in
        connectivity mode are all 1: which k of the k + 2 survive is whatever numpy's unstable sort does with equal keys.  Here the
        documented meaning is implemented: the k nearest.  Where T - 1 <= k nothing is trimmed and the two readings agree;
      * "mean" adds the neighbours in float64, in rising order of nearness, and rounds once (numpy: a float32 running sum); median, max
        and min return numpy's bits on float32;
      * the search orders by float32 keys (``native.nn_topk``): two frames closer to each other in distance than those roundings may swap
        places across the k | k + 1 boundary;
      * librosa refuses (from memory) fewer than about five frames at width 1; here two frames are enough;
      * metrics "cosine" and "euclidean"; at most ``native.NN_TOPK_MAX`` neighbours."""
    n_neighbors: int = 16
    metric: str = "cosine"
    aggregate: str = "median"

    @property
    def unit(self) -> Optional[Unit]:
        return None

    @property
    def elem_type(self) -> Optional[EventType]:
        return None

    def np_func(self, inputs):
        raise NotImplementedError("the numpy (librosa) nn_filter belongs to dataset extraction; use the torch path on the HIP device")

    def torch_func(self, inputs):
        from .. import native
        if not isinstance(inputs, torch.Tensor):
            raise TypeError(f"NearestNeighborFilter: expected a torch.Tensor, got {type(inputs)}")
        if inputs.dtype != torch.float32:
            raise TypeError(f"NearestNeighborFilter runs in float32 on the HIP path, got {inputs.dtype}")
        if inputs.dim() not in (2, 3):
            raise ValueError(f"NearestNeighborFilter takes (T, F) or (B, T, F), got shape {tuple(inputs.shape)}")
        k = int(self.n_neighbors)
        if k < 1:
            raise ValueError(f"NearestNeighborFilter: n_neighbors = {k} < 1")
        if k > native.NN_TOPK_MAX:
            raise NotImplementedError(f"NearestNeighborFilter: n_neighbors = {k}, the limit of the HIP path is {native.NN_TOPK_MAX} "
                                      "(native.NN_TOPK_MAX)")
        if self.metric not in native.NN_TOPK_METRICS:
            raise NotImplementedError(f"NearestNeighborFilter: metric={self.metric!r} is not on the HIP path "
                                      f"({', '.join(native.NN_TOPK_METRICS)})")
        if self.aggregate not in native.NN_AGGREGATES:
            raise ValueError(f"NearestNeighborFilter: aggregate={self.aggregate!r} is none of {', '.join(native.NN_AGGREGATES)}")
        frames, bins = inputs.shape[-2:]
        if frames < 2 or bins < 1:
            raise ValueError(f"NearestNeighborFilter: {frames} frames of {bins} bins, at least two frames are needed")
        native.require_device(inputs)
        if inputs.dim() == 3:
            if inputs.shape[0] < 1:
                raise ValueError(f"NearestNeighborFilter: empty batch {tuple(inputs.shape)}")
            return torch.stack([self._clip(clip) for clip in inputs])
        return self._clip(inputs)

    def _clip(self, x: torch.Tensor) -> torch.Tensor:
        from .. import native
        x = x if x.stride(-1) == 1 or x.shape[-1] == 1 else x.contiguous()       # (nn_topk's self_exclude wants the very rows it is given)
        index, _ = native.nn_topk(x, x, min(int(self.n_neighbors), x.shape[0] - 1), self.metric, self_exclude=True)
        return native.nn_aggregate(x, index, self.aggregate, mutual=True)

    @property
    def inv(self) -> Functional:
        return Identity()


# ---------------------------------------------------------------------------
# harmonic spectrogram filters
# ---------------------------------------------------------------------------
@dtc.dataclass
class AutoConvolve(Functional):
    """reference :1007-1036 on (T, F) or (B, T, F) non-negative float32 magnitudes on the device, one launch of ``native.auto_convolve``
    (``csrc/spec_filter.hip``).  With k = ``window_size``, frame t is weighted over the frames t - k // 2 ... t - k // 2 + k - 1 of its
    clip: p[t, b] is the float64 product of their values at bin b in rising frame order, a frame outside [0, T) counting as 1;
    z = log(1.0 + p) (the rounded sum, not log1p); out = z / (sum_b z + 1e-8) * inputs.  An even k gives the lopsided window this
    formula gives (k = 2: frames t - 1 and t).  Nothing of size k x T x F is written.

    The reference builds its window with ``np.pad`` and ``librosa.feature.stack_memory(n_steps=k, delay=-1, constant_values=1)``; librosa
    is not installed where this was written, and its part is restated from memory of the published source (block s of the stack at time
    t' is padded[t' + s]).

    Differences from the reference: the result is float32, rounded once from the float64 value (the reference returns float64); a batch
    (B, T, F) is filtered clip by clip, the window never crosses a clip (the reference takes 2-D input only); ``window_size`` < 2 raises
    ValueError (the reference's own slice ``[:, :-0]`` is empty at 1) and above ``native.AUTO_CONVOLVE_MAX_WINDOW`` (64)
    NotImplementedError; at most ``native.SPEC_FILTER_MAX_BINS`` (4097) bins; NaN, negative or infinite bins are not looked for and
    their results are unspecified."""
    window_size: int = 3

    @property
    def unit(self) -> Optional[Unit]:
        return None

    @property
    def elem_type(self) -> Optional[EventType]:
        return None

    def np_func(self, inputs):
        raise NotImplementedError("the numpy (librosa) AutoConvolve belongs to dataset extraction; use the torch path on the HIP device")

    def torch_func(self, inputs):
        from .. import native
        return native.auto_convolve(inputs, self.window_size)

    @property
    def inv(self) -> Functional:
        return Identity()


@dtc.dataclass
class F0Filter(Functional):
    """reference :1039-1080 on (T, F) or (B, T, F) non-negative float32 magnitudes on the device, one launch of ``native.f0_filter``
    (``csrc/spec_filter.hip``).  The reference samples every frame z at the harmonics of its bins with ``librosa.interp_harmonics(z,
    librosa.fft_frequencies(), harmonics)``, which is ``scipy.interpolate.interp1d(freqs, z, kind="linear", bounds_error=False,
    fill_value=0)`` evaluated at h * freqs; librosa is not installed where this was written, and that part is restated from memory of the
    published source.  The grid is uniform from 0, so harmonic h of bin b sits at bin position h * b whatever the sample rate, and the
    device forms every index in integers:

      sl[b]  = sum over h = 1 .. n_overtone - 1 of z[h b], a term counting only where h b <= F - 1 (0 beyond: ``fill_value``)
      sl2[b] = sum over x = 2 .. n_undertone - 1 of z[lo] + (z[min(lo + 1, F - 1)] - z[lo]) * (r / x), lo = b // x, r = b % x
      y = sl - sl2;  ``soft``: y+ = y where y > 0 else 0, otherwise y+ = 1 where y > 0 else 0;  ``normalize``: y+ /= sum_b y+ + 1e-8
      out = inputs * y+

    all in float64, rounded to float32 once.  ``n_overtone`` <= 1 makes sl zero and ``n_undertone`` <= 2 makes sl2 zero.

    Differences from the reference: any F from 2 to ``native.SPEC_FILTER_MAX_BINS`` (4097) (the reference works at F = 1025 only, its grid
    being the default one); the result is float32 (the reference returns float64); a batch (B, T, F) is filtered clip by clip (the
    reference takes 2-D input only); at most ``native.F0_FILTER_MAX_OVERTONE`` / ``native.F0_FILTER_MAX_UNDERTONE`` (16 each); NaN,
    negative or infinite bins are not looked for.  scipy does not compute exactly the definition above: it subtracts the two float32
    knots in float32 before it goes to float64, and it may take an integer harmonic's knot as the upper end of [h b - 1, h b], returning
    z[h b - 1] + fl32(difference) for z[h b].  The device evaluates the definition; DESIGN.md 5.6.14 bounds the gap."""
    n_overtone: int = 4
    n_undertone: int = 4
    soft: bool = True
    normalize: bool = True

    @property
    def unit(self) -> Optional[Unit]:
        return None

    @property
    def elem_type(self) -> Optional[EventType]:
        return None

    def np_func(self, inputs):
        raise NotImplementedError("the numpy (librosa) F0Filter belongs to dataset extraction; use the torch path on the HIP device")

    def torch_func(self, inputs):
        from .. import native
        return native.f0_filter(inputs, self.n_overtone, self.n_undertone, self.soft, self.normalize)

    @property
    def inv(self) -> Functional:
        return Identity()


# ---------------------------------------------------------------------------
# mel spectrogram / MFCC
# ---------------------------------------------------------------------------
def _mel_input(inputs, who: str):
    if not isinstance(inputs, torch.Tensor):
        raise TypeError(f"{who}: expected a torch.Tensor, got {type(inputs)}")
    if inputs.dtype != torch.float32:
        raise TypeError(f"{who} runs in float32 on the HIP path, got {inputs.dtype}")
    if inputs.dim() not in (2, 3):
        raise ValueError(f"{who} takes (T, F) or (B, T, F), got shape {tuple(inputs.shape)}")


def _mel_signal(x, who: str):
    if not isinstance(x, torch.Tensor):
        raise TypeError(f"{who}.from_signal: expected a torch.Tensor, got {type(x)}")
    if x.dim() not in (1, 2):
        raise ValueError(f"{who}.from_signal takes (T,) or (B, T), got shape {tuple(x.shape)}")


@dtc.dataclass
class MelSpec(Functional):
    """reference :650-676: ``librosa.feature.melspectrogram(S=inputs.T, n_mels, fmin, fmax, htk).T`` of (T, F) or (B, T, F) float32
    magnitudes on the device.  As there, no ``sr`` is passed: the bank is librosa's for 22050 Hz and ``n_fft = 2 (F - 1)``, whatever the
    audio's rate (``features/mel.py``: a restatement of librosa's published source, Slaney-normalised, held in banded form).
    ``from_signal`` goes from the signal to the mel frames in one launch."""
    n_mels: int = 128
    fmin: float = 0.
    fmax: Optional[float] = None
    htk: bool = False

    @property
    def unit(self) -> Optional[Unit]:
        return None

    @property
    def elem_type(self) -> Optional[EventType]:
        return Continuous(0., float("inf"), self.n_mels)

    def np_func(self, inputs):
        raise NotImplementedError("the numpy (librosa) MelSpec belongs to dataset extraction; use the torch path on the HIP device")

    def _bank(self, n_bins: int, device):
        from . import mel
        return mel.device_bank(n_bins, self.n_mels, self.fmin, self.fmax, self.htk, device)

    def torch_func(self, inputs):
        from .. import native
        _mel_input(inputs, "MelSpec")
        native.require_device(inputs)
        return native.melbank(inputs, self._bank(inputs.shape[-1], inputs.device))

    def from_signal(self, x, magspec: "MagSpec"):
        """``self(magspec(x))`` for x (T,) or (B, T) as one launch of ``native.stft_mel``; bit-identical to the two calls with
        ``pad_mode="constant"``"""
        from .. import native
        _mel_signal(x, "MelSpec")
        native.require_device(x)
        return native.stft_mel(magspec.stft._fix_length(x), magspec.n_fft, magspec.hop_length, bool(magspec.center), magspec.pad_mode,
                               self._bank(magspec.n_fft // 2 + 1, x.device))

    @property
    def inv(self) -> Functional:
        return Identity()


@dtc.dataclass
class MFCC(Functional):
    """reference :680-707: ``librosa.feature.mfcc(S=inputs.T, n_mfcc, dct_type, norm, lifter).T`` of (T, n_mels) or (B, T, n_mels) float32
    on the device: the first ``n_mfcc`` outputs of ``scipy.fft.dct(type, norm)`` along the mel axis, librosa's lifter folded into the
    matrix.  As there, no logarithm is taken: the DCT of whatever it is given.  ``from_signal`` goes from the signal to the coefficients
    in one launch; neither the spectrogram nor the mel frames are written."""
    n_mfcc: int = 20
    dct_type: int = 2
    norm: Optional[str] = "ortho"
    lifter: int = 0

    @property
    def unit(self) -> Optional[Unit]:
        return None

    @property
    def elem_type(self) -> Optional[EventType]:
        return Continuous(0., float("inf"), self.n_mfcc)

    def np_func(self, inputs):
        raise NotImplementedError("the numpy (librosa) MFCC belongs to dataset extraction; use the torch path on the HIP device")

    def _dct(self, n_mels: int, device):
        from . import mel
        return mel.device_dct(self.n_mfcc, n_mels, self.dct_type, self.norm, self.lifter, device)

    def torch_func(self, inputs):
        from .. import native
        _mel_input(inputs, "MFCC")
        native.require_device(inputs)
        return native.melbank(inputs, None, self._dct(inputs.shape[-1], inputs.device))

    def from_signal(self, x, magspec: "MagSpec", melspec: MelSpec):
        """``self(melspec(magspec(x)))`` for x (T,) or (B, T) as one launch of ``native.stft_mel``"""
        from .. import native
        _mel_signal(x, "MFCC")
        native.require_device(x)
        return native.stft_mel(magspec.stft._fix_length(x), magspec.n_fft, magspec.hop_length, bool(magspec.center), magspec.pad_mode,
                               melspec._bank(magspec.n_fft // 2 + 1, x.device), self._dct(melspec.n_mels, x.device))

    @property
    def inv(self) -> Functional:
        return Identity()
