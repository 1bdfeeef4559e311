"""Cutting a signal at its attacks on the MI355X: the multi-scale envelope segmenter of the reference's ``mimikit/extract/samplify.py``
(``Samplifyer`` :178-303, ``Periods`` :125-175, ``attack_decay`` :56-70).

Every level is an envelope follower - ``Envelop(n_fft, n_fft // overlap, normalize=True, interp_to_time_domain=False)`` and its
``Derivative(grad_max_lag, normalize=True)`` - brought to the T samples of the signal by scipy's quadratic interpolating spline.  The
attacks of the coarsest level's gradient (a crossing from below to above zero) are scored by the rise of its envelope up to the next
peak, kept above ``sensitivity``, moved to the minimum of ``0.9 e + 0.1 (1 - g)`` of every finer level in turn where the finest envelope
falls below the coarse one on the right, and snapped to the nearest zero crossing of the signal.

The reference interpolates both curves of every level to T floats through scipy and runs numba loops over them.  Here a level is its n
B-spline coefficients per curve (``native.spline2_coef``, float64); the kernels of ``csrc/samplify.hip`` evaluate the float32 value of a
sample where they need one, through ONE device function, and ``fit`` writes no T-long float array: ``coarse_env``, ``coarse_grad`` and
``fine_envs`` are evaluated when first read.  A ``fit`` waits for the device twice: for the number of attacks and for the number kept.

Differences from the reference:
  * ``n_fft`` is a power of two in [64, 4096] (``native.stft_energy``), so the default ``filter_level=0``, whose first level is 8192,
    raises NotImplementedError: use ``filter_level >= 1`` or ``levels_def``.  ``window`` must be "hann" (the periodic Hann window of the
    torch STFT) and ``interp_mode`` "quadratic"; at most ``native.SAMPLIFY_MAX_LEVELS`` levels;
  * a level needs at least 3 frames (scipy refuses a quadratic spline through 2) and more frames than ``grad_max_lag``;
  * zero crossings are ``signbit(y[i]) != signbit(y[i - 1])``, with ``z[0] = True``: librosa's ``zero_crossings`` without its clipping
    of magnitudes <= 1e-10 to zero;
  * where the outward walk of the snap leaves the signal on the right, the reference reads ``z[T]`` (out of bounds under numba); here
    the walk goes on to the left alone, and ``z[0]`` ends it;
  * a cut whose side is 0 (left) is not refined: the reference sets ``d = c; c = c - (d - c)``, which leaves ``c`` where it was with an
    empty range.  That is kept: a left-side cut is its coarse cut snapped to a zero crossing;
  * spline values are computed in float64 and rounded to float32 once; scipy's differ from them by the rounding of the result and of a
    float64 solve (tests/samplify_refs.py).  A decision closer to a tie than that may fall the other way;
  * results are int64 / float32 tensors on the signal's device; the plots and the module-level ``samplify(audio)`` (which passes an
    ``sr=`` the dataclass does not have) are not carried over.
Device float32 tensors only: a CPU tensor raises, as everywhere in this package.
"""
import dataclasses as dtc
from typing import Dict, List

import torch

from .. import native
from ..features.functionals import Derivative, Envelop, Functional, Identity

__all__ = ["Samplifyer", "Periods", "attack_decay"]

# the reference's default levels (:197-202): (n_fft, overlap, grad_max_lag)
DEFAULT_LEVELS = ((8192, 32, 9), (4096, 64, 33), (2048, 32, 17), (1024, 16, 9), (512, 8, 9), (256, 8, 9))
N_FFT_MIN, N_FFT_MAX = 64, 4096          # csrc/istft.hip: check_fft


@dtc.dataclass
class _EnvelopAndGrad:
    """one level (reference :19-51): the envelope frames, their gradient and the spline coefficients of both"""
    n_fft: int
    overlap: int
    grad_max_lag: int
    window: str = "hann"
    interp_mode: str = "quadratic"

    def __post_init__(self):
        self.coef = None             # (2, n_frames) float64: envelope, gradient
        self.T = 0

    @property
    def hop_length(self) -> int:
        return self.n_fft // self.overlap

    @property
    def env_ex(self) -> Envelop:
        return Envelop(self.n_fft, self.hop_length, normalize=True, window=self.window, interp_to_time_domain=False)

    @property
    def dx(self) -> Derivative:
        return Derivative(self.grad_max_lag, normalize=True)

    def n_frames(self, n_samples: int) -> int:
        return 1 + self.env_ex.fft.stft.fixed_length(n_samples) // self.hop_length

    def check(self, n_samples: int):
        """every refusal of a level, by name, before anything is launched"""
        who = f"Samplifyer level (n_fft={self.n_fft}, overlap={self.overlap}, grad_max_lag={self.grad_max_lag})"
        if self.interp_mode != "quadratic":
            raise NotImplementedError(f"{who}: interp_mode='{self.interp_mode}' is not on the HIP path: 'quadratic' only")
        if self.window != "hann":
            raise NotImplementedError(f"{who}: window='{self.window}' is not on the HIP path: 'hann' only")
        n_fft = int(self.n_fft)
        if n_fft < N_FFT_MIN or n_fft > N_FFT_MAX or n_fft & (n_fft - 1):
            hint = " (the first level of the default filter_level=0: use filter_level >= 1)" if n_fft == 8192 else ""
            raise NotImplementedError(f"{who}: n_fft = {n_fft}{hint}; the frame energies of native.stft_energy take a power of two in "
                                      f"[{N_FFT_MIN}, {N_FFT_MAX}]")
        if self.overlap < 2 or self.overlap > n_fft:
            raise ValueError(f"{who}: overlap = {self.overlap} gives a hop of {n_fft // max(self.overlap, 1)}, which must lie in [1, n_fft)")
        if self.grad_max_lag < 1:
            raise ValueError(f"{who}: grad_max_lag must be at least 1, got {self.grad_max_lag}")
        if self.grad_max_lag > native.DERIV_MAX_LAG:
            raise NotImplementedError(f"{who}: grad_max_lag = {self.grad_max_lag}, the limit is {native.DERIV_MAX_LAG}")
        if n_samples <= n_fft // 2:
            raise ValueError(f"{who}: reflect padding of {n_fft // 2} needs more than {n_fft // 2} samples, got {n_samples}")
        frames = self.n_frames(n_samples)
        if frames < 3:
            raise ValueError(f"{who}: {frames} frames of {n_samples} samples; a quadratic spline needs at least 3 frames")
        if frames <= self.grad_max_lag:
            raise ValueError(f"{who}: {frames} frames of {n_samples} samples are no more than grad_max_lag = {self.grad_max_lag}")

    def fit(self, y: torch.Tensor):
        self.T = y.shape[-1]
        env = self.env_ex(y)
        grad = self.dx(env[None, :])[0]
        self.coef = native.spline2_coef(torch.stack((env, grad)))
        return self

    @property
    def env_coef(self) -> torch.Tensor:
        return self.coef[0]

    @property
    def grad_coef(self) -> torch.Tensor:
        return self.coef[1]

    @property
    def env(self) -> torch.Tensor:
        return native.spline2_eval(self.coef[0], self.T)

    @property
    def grad(self) -> torch.Tensor:
        return native.spline2_eval(self.coef[1], self.T)


def _signal(y, who: str, device: bool = True) -> torch.Tensor:
    if not isinstance(y, torch.Tensor):
        raise TypeError(f"{who}: expected a torch.Tensor, got {type(y)}")
    if device:
        native.require_device(y)
    if y.dtype != torch.float32:
        raise TypeError(f"{who} runs in float32 on the HIP path, got {y.dtype}")
    if y.dim() != 1:
        raise ValueError(f"{who} takes one (T,) row, got shape {tuple(y.shape)}")
    return y


def attack_decay(y: torch.Tensor):
    """y (T,) float32 on the device, an oscillating curve such as a gradient -> (att_i, dec_i), int64 on the device, rising: the samples
    where y goes from below to above zero, and for each the first sample from there on, before the next attack, where y goes from above
    to below zero (T - 1 if there is none)."""
    p = Periods().fit(y)
    return p.att_i, p.dec_i


class Periods:
    """reference :125-175: the attack and peak indices of a gradient; the commented-out metrics are not carried over"""

    def __init__(self):
        self.y = None
        self.att_i = None
        self.dec_i = None
        self.peak_i = None
        self.T = 0

    def fit(self, y: torch.Tensor):
        """y (T,) float32 on the device, taken as it is"""
        y = _signal(y, "Periods.fit")
        self.y, self.T = y, y.shape[0]
        self.att_i, self.dec_i, self.peak_i = native.periods(None, self.T, row=y)
        return self

    def fit_spline(self, coef: torch.Tensor, n_samples: int):
        """the same on the n_samples float32 values of a spline given by its coefficients, which are never written"""
        self.T = int(n_samples)
        self.att_i, self.dec_i, self.peak_i = native.periods(coef, self.T)
        return self


@dtc.dataclass
class Samplifyer(Functional):
    """``Samplifyer(filter_level, sensitivity, levels_def).fit(y)``: y (T,) float32 on the device -> ``cuts`` (int64, in the order of
    the rising ``coarse_cuts``), with ``coarse_cuts``, ``coarse_peaks``, ``scores``, ``sides``, ``windows``, ``mins_rank`` and ``maxs_rank``
    beside them.  ``label(y)`` / ``__call__`` number the samples by the segment they fall in."""
    filter_level: int = 0
    sensitivity: float = 0.
    levels_def: List[Dict] = dtc.field(default_factory=lambda: [{}])

    def __post_init__(self):
        self.y = None
        self.T = None
        if self.filter_level > 4 or self.filter_level < 0:
            raise ValueError("filter_level must be between 0 and 4")
        if self.levels_def and self.levels_def[0]:
            self.levels = [_EnvelopAndGrad(**dict(ldef)) for ldef in self.levels_def]
        else:
            self.levels = [_EnvelopAndGrad(n_fft=n, overlap=o, grad_max_lag=g) for n, o, g in DEFAULT_LEVELS][self.filter_level:]
        self.coarse_cuts = self.coarse_peaks = self.scores = self.cuts = self.sides = self.windows = None
        self.mins_rank = self.maxs_rank = self.left_right_scores = None
        self._lazy = {}

    # -- the T-long curves, evaluated from the coefficients when first read
    def _curve(self, name, make):
        if self.T is None:
            return None
        if name not in self._lazy:
            self._lazy[name] = make()
        return self._lazy[name]

    @property
    def coarse_env(self):
        return self._curve("coarse_env", lambda: self.levels[0].env)

    @property
    def coarse_grad(self):
        return self._curve("coarse_grad", lambda: self.levels[0].grad)

    @property
    def fine_envs(self):
        return self._curve("fine_envs", lambda: [level.env for level in self.levels[1:]])

    def fit(self, y: torch.Tensor):
        y = _signal(y, "Samplifyer.fit", device=False)
        T = y.shape[0]
        if len(self.levels) > native.SAMPLIFY_MAX_LEVELS:
            raise NotImplementedError(f"Samplifyer: {len(self.levels)} levels, the limit is {native.SAMPLIFY_MAX_LEVELS}")
        for level in self.levels:
            level.check(T)
        native.require_device(y)
        y = y.contiguous()
        self.y, self.T, self._lazy = y, T, {}
        # I. the levels: frame energies, their gradient, the spline coefficients of both
        for level in self.levels:
            level.fit(y)
        coarse = self.levels[0]
        # II. the attacks of the coarse gradient, kept where the coarse envelope rises by more than `sensitivity` up to the peak
        att, dec, _ = native.periods(coarse.grad_coef, T)                                   # (waits: the number of attacks)
        scores, env_att, env_dec, keep = native.samplify_scores(coarse.env_coef, T, att, dec, self.sensitivity)
        kept = torch.nonzero(keep).reshape(-1)                                              # (waits: the number kept)
        self.scores, self.coarse_cuts, self.coarse_peaks = scores[kept], att[kept], dec[kept]
        ranks = torch.arange(kept.shape[0], device=y.device)
        self.mins_rank, self.maxs_rank = torch.zeros_like(ranks), torch.zeros_like(ranks)
        self.mins_rank[torch.argsort(env_att[kept], stable=True)] = ranks
        self.maxs_rank[torch.argsort(1 - env_dec[kept], stable=True)] = ranks
        # III. the side of every cut, the refinement through the finer levels and the snap to a zero crossing
        self.windows = torch.clamp(self.coarse_peaks - self.coarse_cuts, max=native.SAMPLIFY_MAX_WINDOW)
        self.sides, self.left_right_scores, self.cuts = native.samplify_cuts(
            y, [lv.env_coef for lv in self.levels], [lv.grad_coef for lv in self.levels], self.coarse_cuts, self.coarse_peaks)
        return self

    def label(self, y: torch.Tensor) -> torch.Tensor:
        cuts = self.fit(y).cuts
        labels = torch.zeros(y.shape[0], dtype=torch.int64, device=y.device)
        labels[cuts] = 1
        return torch.cumsum(labels, 0)

    def np_func(self, y):
        raise NotImplementedError("Samplifyer takes device tensors only: the numpy path of the reference is numba's")

    def torch_func(self, y):
        return self.label(y)

    def export_as_list(self):
        """the pieces of the signal between the cuts (np.split: before the first cut, between two cuts, after the last)"""
        bounds = [0] + [int(c) for c in self.cuts.tolist()] + [self.T]
        return [self.y[a:b] for a, b in zip(bounds[:-1], bounds[1:])]

    def export_with_silence(self, insert_sec=1., sr=44100):
        gap = torch.zeros(int(sr * insert_sec), dtype=self.y.dtype, device=self.y.device)
        return torch.cat([p for x in self.export_as_list() for p in (x, gap)])

    @property
    def inv(self) -> Functional:
        return Identity()
