"""Cutting the frames of a corpus into segments on the MI355X: the recurrence-matrix segmentation of the reference's
``mimikit/extract/segment.py`` (:21-174).

A checkerboard kernel of 2 h + 1 frames is slid along the diagonal of the frames' cosine self-distance matrix; where its sum peaks, the
frames before and after differ from each other and resemble their own side: a cut.  With d(r, c) = 1 - <X_r, X_c> / (|X_r| |X_c|),
d(r, r) = 0 and d = 1 where a frame is zero, for every half-width h_q of ``kernel_sizes``

    raw_q[i]  = 1 / (4 h_q^2) sum_{a, b = -h_q .. h_q, a b != 0} -sign(a) sign(b) d(i + a, i - 1 + b)       (terms outside the matrix: 0)
    scores[q] = raw_q - min_i raw_q,        dg = mean_q scores[q]

- the board is centred on (i, i - 1), as the reference's is (``kdiv2 = k`` in its ``pwdk_cosine``) - and the cuts are the peaks of dg that
``pick_globally_sorted_maxes`` accepts, kept where min_dur < m < T - min_dur.  The reference writes the band of the distance matrix out as
a (T, 2 K - 1) float64 array from numba loops; here ``native.novelty`` forms the Gram tile of a run of frames on the fp32 matrix pipe and
sums the boards of every half-width from LDS (csrc/novelty.hip): neither the band nor the matrix exists in memory.  The scores, the peak
tests and the suppression of peaks that lie within ``min_dur`` of a higher one are kernels of the same file; the ONE host synchronisation
of a call is the ``torch.nonzero`` that reads the number of cuts.

Differences from the reference:
  * ``pwdk_cosine`` allocates 2 k - 1 columns and addresses 2 k + 1.  Under numba the two overflowing writes of row i land in columns 0 and
    1 of row i + 1, where they race with that row's own values and stay where it has none (i + 1 < k); in plain Python the function
    raises IndexError for any T > k - 1.  The device path computes the in-bounds meaning above: it can differ from a numba run only in
    raw_{h_max}[i] for i <= h_max and at the thread-chunk boundaries of that run;
  * distances are fp32 MFMA sums in one fixed order, board sums fp64; the reference works in float64.  Peaks of dg closer to one of the
    picker's thresholds than those roundings may be decided differently (tests/segment_refs.py: ``robust``);
  * equal values of dg are taken lower index first; the reference's ``argsort`` is not stable there;
  * a constant dg (no contrast: max = min, the reference divides by zero) returns no cuts;
  * ``mx2`` (librosa's ``peak_pick``, the "old method" that is only plotted) and ``plot_diagonals`` are not carried over:
    ``from_recurrence_matrix`` returns (cuts, scores).
Device float32 tensors only: a CPU tensor raises, as everywhere in this package.
"""
from typing import List, Sequence

import torch

from .. import native

__all__ = ["discontinuity_scores", "pick_globally_sorted_maxes", "from_recurrence_matrix", "CutsFromRecurrenceMatrix"]


def _scores_and_mean(X: torch.Tensor, kernel_sizes: Sequence[int]):
    if not isinstance(X, torch.Tensor):
        raise TypeError(f"discontinuity_scores: expected a torch.Tensor, got {type(X)}")
    if X.dim() not in (2, 3):
        raise ValueError(f"discontinuity_scores: X must be (T, D) or (B, T, D) frames, got shape {tuple(X.shape)}")
    if X.shape[-2] < 2:
        raise ValueError(f"discontinuity_scores: at least two frames are needed, got T = {X.shape[-2]}")
    inv_norm = native.inv_row_norm(X)            # one read of X; the kernel's own norms would re-read the rows two tiles share
    return native.novelty_finish(native.novelty(X, kernel_sizes, inv_norm))


def discontinuity_scores(X: torch.Tensor, kernel_sizes: Sequence[int]) -> torch.Tensor:
    """X (T, D) or (B, T, D) float32 on the device, kernel_sizes: half-widths h (the boards are 2 h + 1 wide) -> scores (len(kernel_sizes), T)
    or (B, len(kernel_sizes), T) float32, each row shifted so that its minimum is 0"""
    return _scores_and_mean(X, kernel_sizes)[0]


def pick_globally_sorted_maxes(x: torch.Tensor, wait_before: int, wait_after: int, min_strength: float = 0.02) -> torch.Tensor:
    """x (T,) float32 on the device -> the accepted peak indices, int64 on the device, rising.  A constant x returns none."""
    return torch.nonzero(native.pick_peaks(x, wait_before, wait_after, min_strength)).reshape(-1)


def from_recurrence_matrix(X: torch.Tensor, kernel_sizes: Sequence[int] = (6,), min_dur: int = 4, min_strength: float = 0.03):
    """X (T, D) float32 on the device -> (cuts, scores): the frames at which a segment starts (int64, rising, min_dur < cut < T - min_dur)
    and the (len(kernel_sizes), T) discontinuity scores they are the peaks of"""
    if not isinstance(X, torch.Tensor) or X.dim() != 2:
        raise ValueError(f"from_recurrence_matrix: X must be (T, D) frames, got {tuple(X.shape) if isinstance(X, torch.Tensor) else type(X)}")
    scores, dg = _scores_and_mean(X, kernel_sizes)
    picked = native.pick_peaks(dg, min_dur, min_dur, min_strength)
    m = torch.arange(X.shape[0], device=X.device)
    cuts = torch.nonzero(picked & (m > min_dur) & (m < X.shape[0] - min_dur)).reshape(-1)
    return cuts, scores


class CutsFromRecurrenceMatrix:
    """``CutsFromRecurrenceMatrix(kernel_size, factors, min_dur, min_strength)(X)``: the cuts of X (T, D) with half-widths
    int(f * kernel_size); ``.mx`` holds the cuts and ``.diagonals`` the scores of the last call"""

    def __init__(self, kernel_size: int = 6, factors: List[float] = (1.,), min_dur: int = 4, min_strength: float = 0.03):
        self.kernel_sizes = [int(f * kernel_size) for f in factors]
        self.min_dur = min_dur
        self.min_strength = min_strength
        self.mx = self.diagonals = None

    def __call__(self, X: torch.Tensor) -> torch.Tensor:
        self.mx, self.diagonals = from_recurrence_matrix(X, self.kernel_sizes, self.min_dur, self.min_strength)
        return self.mx
