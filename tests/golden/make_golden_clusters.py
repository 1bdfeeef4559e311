"""Generates tests/golden/clusters.npz FROM THE REFERENCE'S OWN HCluster and ArgMax (mimikit/extract/clusters.py:157-230).

Run in the build container only (needs the reference tree, sklearn and scipy):
    python tests/golden/make_golden_clusters.py
mimikit/extract/clusters.py is imported unmodified through oracle/ref_shim.py; the package object ``mimikit.extract`` is a path-only one
made here, as in make_golden_neighbors.py.  What is committed are seeded float32 inputs and the reference's ``labels_`` / ``K_`` only
(``K_`` None is recorded as -1).

The inputs are float32, the dtype the device path takes.  The reference computes in its input's dtype: it is run on the float32 arrays
and on their float64 copies, the two results are asserted equal here, and one is recorded.
"""
import os
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from oracle.ref_shim import REFERENCE_ROOT, load_reference  # noqa: E402

OUT = os.path.dirname(os.path.abspath(__file__))

# name: (seed, low, shape) - uniform(low, 1)
CASES = {"a": (795, 0.0, (40, 33)), "b": (796, -1.0, (97, 65)), "c": (797, 0.0, (300, 17)), "d": (798, 0.0, (2, 5))}
LEVELS = {"a": [6, 1], "b": [26, 6, 1], "c": [53, 7, 1], "d": [1]}          # clusters per level, as found when the cases were chosen


def reference_module():
    load_reference()
    import importlib
    pkg = types.ModuleType("mimikit.extract")
    pkg.__path__ = [os.path.join(REFERENCE_ROOT, "mimikit", "extract")]
    sys.modules["mimikit.extract"] = pkg
    return importlib.import_module("mimikit.extract.clusters")


def fit_both(est, x):
    a = est().fit(x.copy())
    b = est().fit(x.astype(np.float64))
    assert np.array_equal(a.labels_, b.labels_) and a.K_ == b.K_, "the reference's float32 and float64 results differ: choose another seed"
    return np.asarray(a.labels_, dtype=np.int64), np.int64(-1 if a.K_ is None else a.K_)


def make():
    CL = reference_module()
    arrays = {}
    for name, (seed, low, shape) in CASES.items():
        x = np.random.default_rng(seed).uniform(low, 1.0, shape).astype(np.float32)
        labels, k = fit_both(CL.HCluster, x)
        per_level = [int(labels[:, i].max()) + 1 for i in range(labels.shape[1])]
        assert per_level == LEVELS[name] and int(k) == len(per_level), (name, per_level, k)
        arrays[f"h_{name}_x"], arrays[f"h_{name}_labels"], arrays[f"h_{name}_K"] = x, labels, k
        print(f"HCluster {name} {shape}: K_ {int(k)}, clusters per level {per_level}")
    x = np.random.default_rng(1).uniform(0.0, 1.0, (64, 9)).astype(np.float32)
    labels, k = fit_both(lambda: CL.HCluster(max_iter=2), x)
    assert labels.shape == (64, 2) and int(k) == -1 and int(labels[:, 1].max()) + 1 == 4
    arrays["h_two_x"], arrays["h_two_labels"], arrays["h_two_K"] = x, labels, k
    labels, k = fit_both(CL.ArgMax, x)
    arrays["argmax_labels"], arrays["argmax_K"] = labels, k
    path = os.path.join(OUT, "clusters.npz")
    np.savez_compressed(path, **arrays)
    print(f"clusters.npz: {os.path.getsize(path) / 1024:.1f} KiB, {len(arrays)} arrays (envelope.npz: "
          f"{os.path.getsize(os.path.join(OUT, 'envelope.npz')) / 1024:.1f} KiB)")


if __name__ == "__main__":
    make()
