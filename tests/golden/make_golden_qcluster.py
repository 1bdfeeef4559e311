"""Generates tests/golden/qcluster.npz FROM THE REFERENCE'S OWN QCluster (mimikit/extract/clusters.py:27-98).

Run in the build container only (needs the reference tree, sklearn and scipy):
    python tests/golden/make_golden_qcluster.py
mimikit/extract/clusters.py is imported unmodified through oracle/ref_shim.py, as in make_golden_clusters.py.  What is committed are seeded
float32 inputs and the reference's ``labels_`` / ``is_core_`` / ``K_`` only.

The reference computes in its input's dtype: it is run on the float32 arrays and on their float64 copies, the two results are asserted
equal here, and one is recorded.  A case is kept only if the float64 restatement of tests/qcluster_refs.py gives the same result and every
gap the result hangs on is at least 4 of the device's derived bounds (`ratio`): choose another seed otherwise.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from tests import qcluster_refs as Q  # noqa: E402
from tests.golden.make_golden_clusters import reference_module  # noqa: E402

OUT = os.path.dirname(os.path.abspath(__file__))
K_WANT = {"euclid": 5, "euclid_q": 5, "cosine": 1, "cosine_q": 3}      # as found when the cases were chosen


def make():
    CL = reference_module()
    arrays = {}
    for name, (seed, low, frames, metric, params) in Q.FIXTURES.items():
        x = Q.fixture_frames(seed, low, frames)
        a = CL.QCluster(metric=metric, **params).fit(x.copy())
        b = CL.QCluster(metric=metric, **params).fit(x.astype(np.float64))
        assert np.array_equal(a.labels_, b.labels_) and np.array_equal(a.is_core_, b.is_core_) and a.K_ == b.K_, \
            f"{name}: the reference's float32 and float64 results differ: choose another seed"
        ours = Q.qcluster64(x, metric=metric, **params)
        assert np.array_equal(ours["labels"], a.labels_) and np.array_equal(ours["is_core"], a.is_core_) and ours["K"] == a.K_, \
            f"{name}: the restatement differs from the reference"
        assert ours["ratio"] >= 4, f"{name}: smallest gap / bound {ours['ratio']:.2f} < 4: choose another seed"
        assert name not in K_WANT or int(a.K_) == K_WANT[name], (name, a.K_)
        arrays[f"{name}_x"], arrays[f"{name}_labels"] = x, np.asarray(a.labels_, dtype=np.int64)
        arrays[f"{name}_is_core"], arrays[f"{name}_K"] = np.asarray(a.is_core_, dtype=bool), np.int64(a.K_)
        print(f"QCluster {name} ({frames} frames, {metric}, {params}): K_ {int(a.K_)}, sizes {np.bincount(a.labels_).tolist()}, "
              f"{int(a.is_core_.sum())} cores, n {ours['n']}, k {ours['k']}, smallest gap / bound {ours['ratio']:.1f}")
    path = os.path.join(OUT, "qcluster.npz")
    np.savez_compressed(path, **arrays)
    print(f"qcluster.npz: {os.path.getsize(path) / 1024:.1f} KiB, {len(arrays)} arrays")


if __name__ == "__main__":
    make()
