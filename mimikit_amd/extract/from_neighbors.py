"""Scoring generated clips against the training corpus on the MI355X.

Behaviour of the reference's ``mimikit/extract/from_neighbors.py`` as ``demos/checkpoint_k_bests.py:36-46`` uses it: every generated
frame's nearest corpus frame by angular distance (``nearest_neighbor``), how quickly a clip keeps visiting new corpus frames
(``cum_entropy``), and the order of the clips by that score.  ``csrc/neighbors.hip`` holds the two kernels: a cosine GEMM on the fp32
matrix pipe whose epilogue is the row arg-max - the (rows, M) distance matrix the reference materialises is never formed - and the
entropy of the running histogram from occurrence ranks, without the reference's (items, T) table.

What the reference's code does, found by running it (tests/golden/make_golden_neighbors.py records it):
  * ``nearest_neighbor`` as written is degenerate: ``AngularDistance()`` defaults to ``reduction="mean"``, so it returns (the mean distance,
    index 0) for any input.  Implemented here is the evident meaning, ``AngularDistance(reduction="none")(X, Y)`` then ``torch.min(dim=-1)``.
  * ``cum_entropy(n)`` with its default ``neg_diff=True`` raises IndexError (``torch.diff(..., dim=1)`` on a 1-D tensor); only
    ``neg_diff=False`` has a meaning, and ``neg_diff=True`` raises NotImplementedError here.
  * ``repeat_rate`` raises TypeError in the reference and is not carried over.
Differences: a non-zero row pair with |x| |y| < 1e-8 is not special-cased (the reference divides by 1e-8 there;
a zero row has cosine 0 on both sides); ties go to the lowest index; the index is taken on the cosine, not on the rounded distance
(several cosines can round to one fp32 distance, of which the reference's argmin takes the first).  Device float32 / int64 tensors only:
a CPU tensor raises, as everywhere in this package.
"""
import math
from typing import Tuple

import torch

from .. import native

__all__ = ["nearest_neighbor", "cum_entropy", "hist_transform", "NeighborScorer"]


def _has_negatives(t: torch.Tensor) -> bool:
    return bool((t < 0).any())


def angular_distance_of_cosine(cos: torch.Tensor, nonneg: bool) -> torch.Tensor:
    """AngularDistance.forward (mimikit/modules/loss_functions.py:159-178) past the cosine: (1 + nonneg) acos(clamp(cos)) / pi.  The reference's
    clamp limits -1 + eps / 2 and 1 - eps / 2 (eps = 1e-8) round to -1 and 1 in float32; ``nonneg`` is ONE flag for the whole call"""
    return (2.0 if nonneg else 1.0) * torch.acos(torch.clamp(cos, min=-1.0, max=1.0)) / math.pi


def _check_queries(X, bins: int, what: str) -> torch.Tensor:
    if not isinstance(X, torch.Tensor):
        raise TypeError(f"{what}: expected a torch.Tensor, got {type(X)}")
    if X.dtype != torch.float32:
        raise TypeError(f"{what} runs in float32 on the HIP path, got {X.dtype}")
    if X.dim() < 2:
        raise ValueError(f"{what}: X must be (*, N, D) frames, got shape {tuple(X.shape)}")
    if X.shape[-1] != bins:
        raise ValueError(f"{what}: X has {X.shape[-1]} bins, the corpus {bins}")
    if X.numel() == 0:
        raise ValueError(f"{what}: empty input {tuple(X.shape)}")
    native.require_device(X)
    return X


class NeighborScorer:
    """Holds the corpus ``S`` (M, D) with its inverse norms and its sign flag, computed once, and scores batches of generated frames against
    it.  Nothing of size rows x M is ever allocated."""

    def __init__(self, corpus: torch.Tensor):
        if not isinstance(corpus, torch.Tensor):
            raise TypeError(f"NeighborScorer: expected a torch.Tensor, got {type(corpus)}")
        if corpus.dtype != torch.float32:
            raise TypeError(f"NeighborScorer runs in float32 on the HIP path, got {corpus.dtype}")
        if corpus.dim() != 2 or corpus.shape[0] < 1 or corpus.shape[1] < 1:
            raise ValueError(f"NeighborScorer: the corpus must be (M >= 1, D >= 1) frames, got {tuple(corpus.shape)}")
        native.require_device(corpus)
        self.corpus = corpus.contiguous()
        self.inv_norm = native.inv_row_norm(self.corpus)
        self.corpus_has_negatives = _has_negatives(self.corpus)

    @property
    def n_frames(self) -> int:
        return self.corpus.shape[0]

    @property
    def n_bins(self) -> int:
        return self.corpus.shape[1]

    def neighbors(self, X: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
        """X (*, N, D) -> (nn (*, N) int64, cos (*, N) fp32): the arg-max of the cosine and its value"""
        X = _check_queries(X, self.n_bins, "NeighborScorer")
        index, best = native.nn_cosine(X.reshape(-1, X.shape[-1]), self.corpus, self.inv_norm)
        return index.reshape(X.shape[:-1]), best.reshape(X.shape[:-1])

    def __call__(self, X: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
        """X (*, N, D) -> (dists (*, N) fp32, nn (*, N) int64), the reference's return order"""
        nn, cos = self.neighbors(X)
        nonneg = not (self.corpus_has_negatives or _has_negatives(X))
        return angular_distance_of_cosine(cos, nonneg), nn

    def entropy(self, X: torch.Tensor) -> torch.Tensor:
        """X (B, N, D) -> (B,) scores: cum_entropy(nn, neg_diff=False) of every clip's neighbours"""
        nn, _ = self.neighbors(X)
        return cum_entropy(nn.reshape(-1, nn.shape[-1])).reshape(nn.shape[:-1])

    def k_bests(self, X: torch.Tensor, k: int) -> Tuple[torch.Tensor, torch.Tensor]:
        """X (B, N, D) -> (the indices of the k clips of lowest score, in rising order of score as the demo's ``torch.argsort(hx)`` lists
        them - equal scores in clip order - and their scores)"""
        scores = self.entropy(X).reshape(-1)
        k = int(k)
        if k < 1 or k > scores.shape[0]:
            raise ValueError(f"k_bests: k = {k} of {scores.shape[0]} clips")
        order = torch.argsort(scores, stable=True)[:k]
        return order, scores[order]


def nearest_neighbor(X: torch.Tensor, Y: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """X (*, N, D), Y (M, D) -> (dists (*, N), nn (*, N)): every row's nearest row of Y by angular distance"""
    return NeighborScorer(Y)(X)


def cum_entropy(neighbors: torch.Tensor, reduce: str = "sum", neg_diff: bool = False) -> torch.Tensor:
    """neighbors (T,) or (B, T) int64, row by row: e[t] = the entropy (natural log) of the histogram of neighbors[:t + 1].
    ``reduce="sum"``: the sum over t, () or (B,); anything else: e itself, (T,) or (B, T)"""
    if neg_diff:
        raise NotImplementedError("cum_entropy(neg_diff=True) raises in the reference too (IndexError: torch.diff over dim 1 of a 1-D "
                                  "tensor); only neg_diff=False has a meaning to compute")
    if not isinstance(neighbors, torch.Tensor):
        raise TypeError(f"cum_entropy: expected a torch.Tensor, got {type(neighbors)}")
    if neighbors.dim() not in (1, 2):
        raise ValueError(f"cum_entropy: expected (T,) or (B, T) neighbours, got shape {tuple(neighbors.shape)}")
    rows = neighbors.unsqueeze(0) if neighbors.dim() == 1 else neighbors
    if reduce == "sum":
        out = native.cum_entropy(rows)
    else:
        out = native.cum_entropy(rows, per_step=True)[1]
    return out[0] if neighbors.dim() == 1 else out


def hist_transform(neighbors: torch.Tensor, bins: int = 256) -> torch.Tensor:
    """neighbors (*, T) -> (*, bins): every series' histogram, ``torch.histc`` over the series' own value range (plain torch, no kernel)"""
    series = neighbors.reshape(-1, neighbors.shape[-1])
    counts = torch.stack([torch.histc(row, bins=bins) for row in series])
    return counts.reshape(neighbors.shape[:-1] + (bins,))
