"""Labelling the frames of a corpus on the MI355X: the two deterministic estimators of the reference's ``mimikit/extract/clusters.py``.

``HCluster`` (clusters.py:157-205) merges every frame with its nearest other frame by cosine distance, takes the connected components of
that graph as clusters, replaces each cluster by the unweighted mean of ITS ROWS OF THE LEVEL BEFORE (not of the original frames) and
repeats on the means until one cluster is left: ``labels_[:, i]`` is every frame's cluster at level i.  The reference forms the full
(N, N) distance matrix at every level; here one level is

    native.inv_row_norm -> native.nn_cosine_self -> native.nn_components -> a gather for the label column -> native.segment_mean

(csrc/neighbors.hip, csrc/hcluster.hip) and nothing of size N x N is allocated: the peak is O(N D).  The number of clusters is read back
once per level to size the next one - at most ``max_iter`` synchronisations.  The members of a cluster reach ``segment_mean`` through a
stable ``torch.sort`` of the labels and a ``torch.bincount`` / ``cumsum`` (plumbing: O(N) integers).

``ArgMax`` (clusters.py:207-230) is ``torch.unique(x.argmax(1), return_inverse=True)`` on the device: plain torch, no kernel.

Differences from the reference:
  * the reference drops every pair at distance exactly 0 (``Da[Da == 0] = inf``), so two exact duplicate rows cannot be each other's
    nearest; here only j == i is dropped, and duplicates find each other (the lower index among equals);
  * the reference computes in the input's dtype with sklearn's ``pairwise_distances``; here the cosines are fp32 MFMA sums in one fixed
    order and the means fp64 sums rounded to fp32 once.  Where a frame's best and second-best cosine are closer than those roundings
    the two may pick different neighbours;
  * a zero row has cosine 0 to everything, as in sklearn.
``KMeans``, ``SpectralClustering``, ``QCluster`` and ``GCluster`` are not carried over: random initialisation, sklearn's solvers or an
Adam loop leave no reference result to pin.  Device float32 tensors only: a CPU tensor raises, as everywhere in this package.
"""
import dataclasses as dtc
from typing import Optional

import torch

from .. import native
from ..features.functionals import Functional, Identity

__all__ = ["HCluster", "ArgMax"]


def _check_frames(x, what: str) -> torch.Tensor:
    if not isinstance(x, torch.Tensor):
        raise TypeError(f"{what}: expected a torch.Tensor, got {type(x)}")
    if x.dtype != torch.float32:
        raise TypeError(f"{what} runs in float32 on the HIP path, got {x.dtype}")
    if x.dim() != 2 or x.shape[0] < 1 or x.shape[1] < 1:
        raise ValueError(f"{what}: x must be (N >= 1, D >= 1) frames, got shape {tuple(x.shape)}")
    native.require_device(x)
    return x


def _no_numpy(name: str):
    raise NotImplementedError(f"{name} runs on device tensors only (csrc/neighbors.hip, csrc/hcluster.hip): pass a float32 tensor on the HIP "
                              "device; this package has no CPU path")


@dtc.dataclass
class HCluster(Functional):
    max_iter: int = 32
    metric: str = "cosine"

    def __post_init__(self):
        self.K_: Optional[int] = None
        self.labels_: Optional[torch.Tensor] = None

    def fit(self, x: torch.Tensor) -> "HCluster":
        """x (N, D) float32 on the device -> ``labels_`` (N, levels) int64 on the device and ``K_`` = the number of levels if the last one
        has a single cluster, else None (``labels_`` then has ``max_iter`` columns) - as the reference sets them"""
        if self.metric != "cosine":
            raise NotImplementedError(f"HCluster(metric={self.metric!r}) is not on the HIP path: 'cosine' only")
        x = _check_frames(x, "HCluster")
        self.K_, self.labels_ = None, None
        n = x.shape[0]
        max_iter = int(self.max_iter)
        if max_iter < 1:
            self.labels_ = torch.zeros((n, 0), dtype=torch.int64, device=x.device)
            return self
        if n == 1:          # the reference's only frame has no neighbour; its argmin over a row of inf is 0: one cluster at level 0
            self.labels_, self.K_ = torch.zeros((1, 1), dtype=torch.int64, device=x.device), 1
            return self
        columns = []
        xa, frame_labels = x, None
        for i in range(max_iter):
            nearest, _ = native.nn_cosine_self(xa)
            labels, count = native.nn_components(nearest)
            frame_labels = labels if frame_labels is None else labels[frame_labels]
            columns.append(frame_labels)
            k = int(count)                          # the level's one synchronisation
            if k == 1:
                self.K_ = i + 1
                break
            if i + 1 < max_iter:
                order = torch.sort(labels, stable=True)[1]
                offsets = torch.zeros((k + 1,), dtype=torch.int64, device=x.device)
                torch.cumsum(torch.bincount(labels, minlength=k), 0, out=offsets[1:])
                xa = native.segment_mean(xa, order, offsets)
        self.labels_ = torch.stack(columns, dim=1)
        return self

    def np_func(self, inputs):
        _no_numpy("HCluster")

    def torch_func(self, inputs):
        return self.fit(inputs).labels_

    @property
    def inv(self) -> Functional:
        return Identity()


@dtc.dataclass
class ArgMax(Functional):
    """every frame labelled by the rank of its largest bin among the bins that are some frame's largest (plain torch, no kernel)"""

    def __post_init__(self):
        self.K_: Optional[int] = None
        self.labels_: Optional[torch.Tensor] = None

    def fit(self, x: torch.Tensor) -> "ArgMax":
        x = _check_frames(x, "ArgMax")
        uniques, self.labels_ = torch.unique(x.argmax(1), return_inverse=True)
        self.K_ = int(uniques.shape[0])
        return self

    def np_func(self, inputs):
        _no_numpy("ArgMax")

    def torch_func(self, inputs):
        return self.fit(inputs).labels_

    @property
    def inv(self) -> Functional:
        return Identity()
