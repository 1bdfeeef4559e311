"""Labelling the frames of a corpus on the MI355X: the three deterministic estimators of the reference's ``mimikit/extract/clusters.py``.

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

``QCluster`` (clusters.py:27-98, the clusterizer app's "quantile clustering") is a k-nearest-neighbour graph, an in-degree quantile and
connected components - no random start, no solver.  With qe = 1 - cores_prop, n = n_neighbors (int(sqrt(N)) if None) and
k = core_neighborhood_size (int(qe n) if None):

    native.nn_topk(x, x, max(n, k), metric, self_exclude=True)      every frame's nearest OTHER frames, nearest first
    in_degree[j] = the number of i with j among the first n of i's list;  is_core = in_degree >= quantile(in_degree, qe)
    edges: core i - every core among the first k of i's list;  non-core i - its nearest core (native.nn_topk of the non-cores against
    the gathered core rows, t = 1)
    native.edge_components(src, dst, N)                             labels_, numbered by rising smallest member, and K_

(csrc/qcluster.hip, csrc/hcluster.hip).  The in-degree (``bincount``), the quantile (a ``sort`` and numpy's own "linear" expression on the
two order statistics, evaluated in float64 ON THE DEVICE: a + (b - a) g, or b - (b - a) (1 - g) where g >= 0.5), the masks and the gather
are torch plumbing on O(N max(n, k)) integers; nothing of size N x N is allocated.  Synchronisations per ``fit``: one to size the core set
(``nonzero``), one per four rounds of hooking inside ``edge_components`` (its changed-flag; a handful for a k-NN graph), one to read K_.

Differences from the reference:
  * only j == i is dropped from a frame's list.  The reference's in-degree ignores every pair at distance exactly 0, and sklearn finds
    "self" in a list by its distance, so exact duplicate frames may count differently there;
  * keys are fp32 MFMA sums in one fixed order (cosine: scaled by the two inverse norms; euclidean: <x, y> - |y|^2 / 2, never
    |x|^2 + |y|^2 - 2 <x, y>).  Two neighbours closer than those roundings may swap places;
  * a single core: the reference raises (its 2-nearest-cores query finds one sample); here every frame joins it: one cluster;
  * metric "manhattan" is not on the HIP path, and max(n, k) is limited to ``native.NN_TOPK_MAX`` - ``n_neighbors=None`` asks for sqrt(N)
    neighbours and raises on a corpus of more than (NN_TOPK_MAX + 1)^2 - 1 frames.
``KMeans``, ``SpectralClustering`` and ``GCluster`` are not carried over: random initialisation, sklearn's solvers or an Adam loop
leave no reference result to pin.  Device float32 tensors only: a CPU tensor raises, as everywhere in this package.
"""
import dataclasses as dtc
import math
from typing import Optional

import torch

from .. import native
from ..features.functionals import Functional, Identity

__all__ = ["QCluster", "HCluster", "ArgMax"]


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
    raise NotImplementedError(f"{name} runs on device tensors only (csrc/neighbors.hip, csrc/hcluster.hip, csrc/qcluster.hip): pass a float32 tensor on the HIP "
                              "device; this package has no CPU path")


@dtc.dataclass
class QCluster(Functional):
    cores_prop: float = .5
    n_neighbors: Optional[int] = 8
    core_neighborhood_size: Optional[int] = 8
    metric: str = "euclidean"

    def __post_init__(self):
        self.qe = 1 - self.cores_prop
        self.n_neighbs = self.n_neighbors
        self.k = self.core_neighborhood_size
        self.is_core_: Optional[torch.Tensor] = None
        self.labels_: Optional[torch.Tensor] = None
        self.K_: Optional[int] = None

    def fit(self, x: torch.Tensor) -> "QCluster":
        """x (N, D) float32 on the device -> ``labels_`` (N,) int64 and ``is_core_`` (N,) bool on the device, ``K_`` (int) the number of
        clusters - as the reference sets them.  Synchronises to size the core set, inside ``native.edge_components`` and to read K_"""
        self.__post_init__()
        if self.metric not in native.NN_TOPK_METRICS:
            raise NotImplementedError(f"QCluster(metric={self.metric!r}) is not on the HIP path: {' or '.join(native.NN_TOPK_METRICS)}")
        x = _check_frames(x, "QCluster")
        if not 0.0 <= self.qe <= 1.0:
            raise ValueError(f"QCluster: cores_prop = {self.cores_prop} must lie in [0, 1]")
        N, dev = x.shape[0], x.device
        if self.n_neighbs is None:
            self.n_neighbs = int(math.sqrt(N))
        if self.k is None:
            self.k = int(self.qe * self.n_neighbs)
        n, k = int(self.n_neighbs), int(self.k)
        if n < 1 or k < 0:
            raise ValueError(f"QCluster: n_neighbors = {n} (at least 1), core_neighborhood_size = {k} (at least 0)")
        if max(n, k) > native.NN_TOPK_MAX:
            raise NotImplementedError(f"QCluster: max(n_neighbors, core_neighborhood_size) = {max(n, k)} neighbours per frame, the limit of "
                                      f"the HIP path is {native.NN_TOPK_MAX} (native.NN_TOPK_MAX)")
        if N <= n:
            raise ValueError(f"QCluster: n_neighbors = {n} needs more than {n} frames, got N = {N}")
        lists, _ = native.nn_topk(x, x, max(n, k), self.metric, self_exclude=True)        # -1 past a frame's N - 1 other frames (k only)
        in_degree = torch.bincount(lists[:, :n].reshape(-1), minlength=N)
        # numpy's quantile(in_degree, qe), method "linear": the two order statistics around (N - 1) qe and its own float64 expression
        virtual = (N - 1) * self.qe
        prev = N - 1 if virtual >= N - 1 else int(math.floor(virtual))
        g = virtual - prev
        ordered = torch.sort(in_degree)[0].to(torch.float64)
        a, b = ordered[prev], ordered[min(prev + 1, N - 1)]
        diff = b - a
        threshold = b - diff * (1 - g) if g >= 0.5 else a + diff * g
        is_core = in_degree.to(torch.float64) >= threshold
        cores_idx = is_core.nonzero()[:, 0]                                                 # (synchronises: the size of the core set)
        frames = torch.arange(N, dtype=torch.int64, device=dev)
        src, dst = [], []
        if k > 0:       # core i - core j among the first k of i's list; every other pair becomes the self-loop i - i (no compaction)
            near = lists[:, :k]
            keep = is_core[:, None] & (near >= 0) & is_core[near.clamp(min=0)]
            src.append(frames[:, None].expand(N, k).reshape(-1))
            dst.append(torch.where(keep, near, frames[:, None]).reshape(-1))
        if cores_idx.shape[0] < N:
            others = (~is_core).nonzero()[:, 0]
            nearest, _ = native.nn_topk(x[others], x[cores_idx], 1, self.metric)
            src.append(others)
            dst.append(cores_idx[nearest[:, 0]])
        if src:
            labels, count = native.edge_components(torch.cat(src), torch.cat(dst), N)
        else:
            labels, count = native.edge_components(frames[:0], frames[:0], N)
        self.K_, self.labels_, self.is_core_ = int(count), labels, is_core
        return self

    def np_func(self, inputs):
        _no_numpy("QCluster")

    def torch_func(self, inputs):
        return self.fit(inputs).labels_

    @property
    def inv(self) -> Functional:
        return Identity()


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
