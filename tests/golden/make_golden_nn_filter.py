"""Generates tests/golden/nn_filter.npz on the seeded fixtures of tests/nn_filter_refs.py.  CPU only.

    python -m tests.golden.make_golden_nn_filter            (from the repository root; needs scikit-learn and scipy)

The reference is librosa.decompose.nn_filter(x, aggregate, metric, sym=True, sparse=True, k, axis=0).  librosa is not installed where
this file was written, and nothing here imports it or reads the reference tree.
  Third-party code called itself: sklearn.neighbors.NearestNeighbors(n_neighbors=min(n - 1, k + 2), metric=metric).fit(x).kneighbors() - the
    search librosa.segment.recurrence_matrix makes (kneighbors without an argument leaves every frame out of its own list, as
    kneighbors_graph does); scipy.sparse for the link matrix and its minimum with its transpose; numpy's np.median / np.mean / np.max.
  Restated from memory of librosa's published source: that recurrence_matrix asks for min(n - 1, k + 2) neighbours, keeps "the k closest"
    per row (here: the k nearest by sklearn's own distances - the documented meaning; librosa's argsort of equal stored values keeps an
    unspecified k of the k + 2), symmetrises by rec.minimum(rec.T) for sym=True, and that nn_filter replaces every frame by
    aggregate(x[its links], axis=0) and leaves a frame without a link as it is.

The file holds results only: per fixture the neighbour counts and the median, mean and max outputs (float32, as numpy gives them), a float64
checksum of the frames (the tests regenerate them from the seed) and the library versions.  A fixture is written only where exact agreement
is a fair demand of a correct fp32 device path, and where it exercises the aggregate; the generator asserts, and refuses the fixture otherwise:
  - the smallest float64 gap at a row's k | k + 1 boundary is at least 4 x the row's derived fp32 key bound (nn_filter_refs.MIN_RATIO);
  - the float64 restatement (nn_filter_refs.nn_filter64) names the same links as sklearn;
  - the counts hold an even count, an odd count and a full count (= k), and as many rows without a neighbour as nn_filter_refs.FIXTURES
    says (four of the six fixtures have some).  The 12-frame fixture is the case n - 1 <= k: every frame lists every other, every count
    is 11, and only that is asserted of it.
"""
import os
import sys

import numpy as np
import scipy
import scipy.sparse
import sklearn
from sklearn.neighbors import NearestNeighbors

from tests import nn_filter_refs as R

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "nn_filter.npz")


def links(x, k, metric):
    """steps 1-3: the symmetric link matrix (n, n), CSR with sorted columns"""
    n = x.shape[0]
    dist, ind = NearestNeighbors(n_neighbors=min(n - 1, k + 2), metric=metric).fit(x).kneighbors()
    order = np.argsort(dist, axis=1, kind="stable")[:, :k]                     # (kneighbors sorts already: the k nearest of the k + 2)
    ind = np.take_along_axis(ind, order, 1)
    rows = np.repeat(np.arange(n), ind.shape[1])
    rec = scipy.sparse.csr_matrix((np.ones(rows.shape[0]), (rows, ind.reshape(-1))), shape=(n, n))
    rec = rec.minimum(rec.T).tocsr()
    rec.eliminate_zeros()
    rec.sort_indices()
    return rec


def filtered(x, rec, aggregate):
    """step 4"""
    out = x.copy()
    for i in range(x.shape[0]):
        nb = rec.indices[rec.indptr[i]:rec.indptr[i + 1]]
        if nb.shape[0]:
            out[i] = aggregate(x[nb], axis=0)
    return out


def checksum(x):
    return float(np.asarray(x, dtype=np.float64).sum())


def main():
    out = dict(sklearn_version=np.array(sklearn.__version__), numpy_version=np.array(np.__version__), scipy_version=np.array(scipy.__version__))
    for name, (n, d, k, metric, seed, empty) in R.FIXTURES.items():
        x = R.fixture_frames(name)
        rec = links(x, k, metric)
        counts = np.diff(rec.indptr).astype(np.int32)
        res = R.fixture_result(name, "median")
        assert res["ratio"] >= R.MIN_RATIO, f"{name}: the smallest gap at the k | k + 1 boundary is {res['ratio']:.2f} x the key bound"
        mine = R.mutual_lists64(res["index"])
        for i in range(n):
            assert sorted(mine[i].tolist()) == rec.indices[rec.indptr[i]:rec.indptr[i + 1]].tolist(), f"{name}: row {i}'s links differ from sklearn's"
        if n - 1 <= k:
            assert (counts == n - 1).all(), f"{name}: not every frame is linked to every other"
        else:
            assert (counts == k).any(), f"{name}: no full count ({np.bincount(counts).tolist()})"
            assert ((counts > 0) & (counts % 2 == 0)).any() and (counts % 2 == 1).any(), f"{name}: no even or no odd count"
        assert int((counts == 0).sum()) == empty, f"{name}: {int((counts == 0).sum())} rows without a neighbour, nn_filter_refs.FIXTURES says {empty}"
        print(f"{name} {x.shape}, k {k}, {metric}: ratio {res['ratio']:.1f}, rows per count {np.bincount(counts, minlength=min(k, n - 1) + 1).tolist()}")
        out.update({f"{name}_counts": counts, f"{name}_checksum": np.array(checksum(x))})
        for op in R.GOLDEN_OPS:
            out[f"{name}_{op}"] = filtered(x, rec, getattr(np, op)).astype(np.float32)
    np.savez_compressed(OUT, **out)
    print(f"wrote {OUT}: {os.path.getsize(OUT)} bytes")


if __name__ == "__main__":
    sys.exit(main())
