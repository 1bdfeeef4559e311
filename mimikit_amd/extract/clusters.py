"""Labelling the frames of a corpus on the MI355X: the three deterministic estimators of the reference's ``mimikit/extract/clusters.py``
and ``KMeans``, whose random draws can all be made before the first launch.

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
``SpectralClustering`` and ``GCluster`` are not carried over: sklearn's eigen-solver with its random start, or an Adam loop, leave no
reference result to pin.  Device float32 tensors only: a CPU tensor raises, as everywhere in this package.

``KMeans`` (clusters.py:233-262, the clusterizer app's "kmeans") is ``sklearn.cluster.KMeans(n_clusters, n_init, max_iter,
random_state=random_seed)`` - init "k-means++", algorithm "lloyd", tol 1e-4 - as sklearn 1.7 runs it on dense float32 frames with unit
weights.  Its random numbers are ``numpy.random.RandomState`` draws whose number does not depend on the data, so all of them are made on
the host before the first launch, and the rest is deterministic (csrc/kmeans.hip, include/mmk_kmeans.h):

  1. tol = 1e-4 x the mean over the columns of the population variance of x.  The column mean mu is taken in float64
     (``native.pca_colstats``) and rounded to float32; every kernel works on x' = fl32(x - mu), subtracted while loading - the centred
     corpus is never written - and ``cluster_centers_`` gets mu added back at the end.
  2. draws: rs = RandomState(random_seed), one generator for all n_init runs; per run first = rs.choice(N, p=full(N, 1 / N)), then
     n_clusters - 1 times rs.uniform(size=T) with T = 2 + int(log(n_clusters)).
  3. seeding: closest[r] = |x'_r - x'_first|^2, pot = sum(closest); for every further centre the candidates are
     clip(searchsorted(cumsum(closest), u pot, side="left"), N - 1), candidate t gives m_t = min(closest, |x' - x'_cand_t|^2) and
     pot_t = sum(m_t), the FIRST t with the smallest pot_t wins: closest = m_t, pot = pot_t, the centre is row cand_t
     (``native.kmeans_pp_step``).  Distances, closest, the pots and the scan are float64 on the device (the difference of two floats is
     exact there, the squares are added in one fixed order); ``torch.cumsum`` / ``torch.searchsorted`` are plumbing on N numbers; u pot is
     multiplied on the device: seeding reads nothing back.
  4. Lloyd (``lloyd``), at most max_iter times: every frame goes to the FIRST centre with the largest <x'_r, c_j> - |c_j|^2 / 2
     (``native.kmeans_assign``: fp32 MFMA sums in one fixed order); the new centres are the means of their members, summed in float64 in
     one fixed order and rounded to float32 once (``native.kmeans_label_sums``; the division is torch on K x D numbers).  Empty clusters:
     the n_e frames farthest from their own old centre - by |x'_r - c_old[label_r]|^2 computed directly, in descending order, ties to
     the lower index - become the centres of the n_e empty clusters in rising cluster number and leave their old clusters' sums and
     counts (their labels stay).  For one empty cluster this is sklearn's rule; for two or more sklearn's order comes out of
     ``argpartition`` and is no contract.  Stop with "strict convergence" when the labels equal the previous iteration's; otherwise stop
     when sum_j |c_new_j - c_old_j|^2 <= tol, and in that case, and when max_iter runs out, assign once more against the final centres.
     inertia = sum_r |x'_r - c_label_r|^2, computed directly in float64.  n_iter as sklearn counts it.
  5. the run kept: the first, then any later run with a strictly smaller inertia whose labelling is not the same clustering up to renaming
     (sklearn's ``_is_same_clustering``: every label of the one maps to a single label of the other).

Synchronisations: at most two small host reads per Lloyd iteration - one of (the number of changed labels, the number of empty
clusters), one of the shift against tol, only when labels changed - plus, per run, its inertia and, for a run that could replace the kept
one, the same-clustering test; an iteration that has empty clusters reads their numbers (``nonzero``) as well.  Nothing of size N x K is
allocated anywhere.

Differences from sklearn: sklearn centres with numpy's float32 column mean, measures the seeding distances by
|x|^2 + |y|^2 - 2 <x, y> in float32 and sums the members in float32; where a frame's best and second-best centre, or a draw and a boundary of
the scan, are closer than those roundings the two may part ways.  ``n_clusters`` is limited to ``native.KMEANS_MAX_K``, D to
``native.PCA_MAX_D`` (the column statistics); no sample_weight, no other init, no Elkan, no predict / transform.
"""
import dataclasses as dtc
import math
from typing import Optional

import numpy as np
import torch

from .. import native
from ..features.functionals import Functional, Identity

__all__ = ["QCluster", "HCluster", "ArgMax", "KMeans"]


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
    raise NotImplementedError(f"{name} runs on device tensors only (csrc/neighbors.hip, csrc/hcluster.hip, csrc/qcluster.hip, csrc/kmeans.hip): pass a float32 tensor on the HIP "
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


# ---------------------------------------------------------------------------------------------------------------------------- KMeans
def _column_stats(x: torch.Tensor):
    """(mu (D,) float32, the mean over the columns of the population variance of x as a float): the column means in float64 rounded once"""
    mean, scale = native.pca_colstats(x)
    var = torch.where(x.amax(0) == x.amin(0), torch.zeros_like(scale), scale * scale)      # (pca_colstats gives a constant column scale 1)
    return mean.float(), float(var.mean())


def _lloyd(x, mu, centres, max_iter: int, tol: float):
    """one run from `centres` (K, D) float32 in the coordinates of x' = fl32(x - mu) -> (labels (N,) int32, inertia () float64 on the device,
    centres in those coordinates, n_iter)"""
    n, k = x.shape[0], centres.shape[0]
    dev = x.device
    labels = torch.full((n,), -1, dtype=torch.int32, device=dev)
    changed = torch.zeros((), dtype=torch.int64, device=dev)
    strict, n_iter = False, 0
    for i in range(int(max_iter)):
        changed.zero_()
        native.kmeans_assign(x, mu, centres, labels, changed)
        sums, counts = native.kmeans_label_sums(x, mu, labels, k)
        empty = counts == 0
        n_changed, n_empty = torch.stack([changed, empty.sum()]).tolist()                   # the iteration's first host read
        if n_empty:
            d2 = native.kmeans_label_sums(x, mu, labels, k, centres=centres, row_d2=True)[3]
            far = torch.sort(d2, descending=True, stable=True)[1][:n_empty]                 # farthest first, equal distances by rising index
            rows = (x[far] - mu).double()
            was = labels[far].long()
            sums.index_add_(0, was, -rows)
            counts.index_add_(0, was, torch.full_like(was, -1))
            into = empty.nonzero()[:, 0]                                                    # rising cluster number
            sums[into] = rows
            counts[into] = 1
        new = (sums / counts.clamp(min=1).to(torch.float64)[:, None]).float()
        old, centres, n_iter = centres, new, i + 1
        if n_changed == 0:
            strict = True
            break
        if float(((new.double() - old.double()) ** 2).sum()) <= tol:                        # the second, only when labels changed
            break
    if not strict:
        native.kmeans_assign(x, mu, centres, labels)
    inertia = native.kmeans_label_sums(x, mu, labels, k, centres=centres)[2]
    return labels, inertia, centres, n_iter


def lloyd(x: torch.Tensor, init: torch.Tensor, max_iter: int = 100, tol: Optional[float] = None):
    """One Lloyd run from the given centres: x (N, D) float32 on the device, init (K, D) float32 in the input's coordinates, tol the
    absolute bound on the centres' squared shift (None: 1e-4 x the mean column variance, as ``KMeans`` sets it) -> (labels (N,) int64,
    inertia (float), centres (K, D) float32 in the input's coordinates, n_iter) - step 4 of the module docstring, what ``KMeans.fit`` runs
    once per seeding"""
    x = _check_frames(x, "lloyd")
    init = _check_frames(init, "lloyd")
    if init.shape[1] != x.shape[1] or init.shape[0] > x.shape[0]:
        raise ValueError(f"lloyd: x {tuple(x.shape)}, init {tuple(init.shape)}: the same bins, and no more centres than frames")
    if init.shape[0] > native.KMEANS_MAX_K:
        raise NotImplementedError(f"lloyd: {init.shape[0]} centres, the limit of the HIP path is {native.KMEANS_MAX_K} (native.KMEANS_MAX_K)")
    mu, var = _column_stats(x)
    labels, inertia, centres, n_iter = _lloyd(x, mu, init - mu, max_iter, 1e-4 * var if tol is None else float(tol))
    return labels.long(), float(inertia), centres + mu, n_iter


def _same_clustering(a: torch.Tensor, b: torch.Tensor, k: int) -> bool:
    """sklearn's _is_same_clustering: every label of `a` is paired with one single label of `b`"""
    a, b = a.long(), b.long()
    return int(torch.unique(a * k + b).numel()) == int(torch.unique(a).numel())


@dtc.dataclass
class KMeans(Functional):
    n_clusters: int = 16
    n_init: int = 2
    max_iter: int = 100
    random_seed: int = 42

    def __post_init__(self):
        self.labels_: Optional[torch.Tensor] = None
        self.cluster_centers_: Optional[torch.Tensor] = None
        self.inertia_: Optional[float] = None
        self.n_iter_: Optional[int] = None
        self.seed_rows_: Optional[torch.Tensor] = None

    def fit(self, x: torch.Tensor) -> "KMeans":
        """x (N >= n_clusters, D) float32 on the device -> ``labels_`` (N,) int64 and ``cluster_centers_`` (K, D) float32 on the device,
        ``inertia_`` (float), ``n_iter_`` (int) - as sklearn's KMeans sets them - and ``seed_rows_`` (n_init, K) int64, the frames every
        seeding chose.  Synchronises as the module docstring says"""
        self.__post_init__()
        x = _check_frames(x, "KMeans")
        n, dev = x.shape[0], x.device
        k, n_init, max_iter = int(self.n_clusters), int(self.n_init), int(self.max_iter)
        if k < 1 or n_init < 1 or max_iter < 1:
            raise ValueError(f"KMeans: n_clusters = {k}, n_init = {n_init}, max_iter = {max_iter} (all at least 1)")
        if k > native.KMEANS_MAX_K:
            raise NotImplementedError(f"KMeans: n_clusters = {k}, the limit of the HIP path is {native.KMEANS_MAX_K} (native.KMEANS_MAX_K)")
        if n < k:
            raise ValueError(f"KMeans: n_clusters = {k} needs at least {k} frames, got N = {n}")
        # every draw, on the host, before the first launch
        rs = np.random.RandomState(int(self.random_seed))
        trials = 2 + int(math.log(k))
        firsts, uniforms = np.zeros((n_init,), dtype=np.int64), np.zeros((n_init, max(k - 1, 1), trials), dtype=np.float64)
        for run in range(n_init):
            firsts[run] = rs.choice(n, p=np.full(n, 1 / n))
            for c in range(k - 1):
                uniforms[run, c] = rs.uniform(size=trials)
        firsts, uniforms = torch.from_numpy(firsts).to(dev), torch.from_numpy(uniforms).to(dev)
        mu, var = _column_stats(x)
        tol = 1e-4 * var
        seed_rows = torch.empty((n_init, k), dtype=torch.int64, device=dev)
        closest = torch.empty((n,), dtype=torch.float64, device=dev)
        pot = torch.empty((), dtype=torch.float64, device=dev)
        work = torch.empty((native.lib().mmk_kmeans_pp_step_workspace_bytes() // 8,), dtype=torch.float64, device=dev)
        best = None
        for run in range(n_init):
            closest.fill_(float("inf"))
            native.kmeans_pp_step(x, mu, firsts[run:run + 1], closest, pot, seed_rows[run, 0], work)
            for c in range(1, k):
                cand = torch.searchsorted(torch.cumsum(closest, 0), uniforms[run, c - 1] * pot).clamp_(max=n - 1)
                native.kmeans_pp_step(x, mu, cand, closest, pot, seed_rows[run, c], work)
            labels, inertia, centres, n_iter = _lloyd(x, mu, x[seed_rows[run]] - mu, max_iter, tol)
            inertia = float(inertia)
            if best is None or (inertia < best[1] and not _same_clustering(labels, best[0], k)):
                best = (labels, inertia, centres, n_iter)
        self.labels_, self.inertia_, self.n_iter_ = best[0].long(), best[1], best[3]
        self.cluster_centers_ = best[2] + mu
        self.seed_rows_ = seed_rows
        return self

    def np_func(self, inputs):
        _no_numpy("KMeans")

    def torch_func(self, inputs):
        return self.fit(inputs).labels_

    @property
    def inv(self) -> Functional:
        return Identity()
