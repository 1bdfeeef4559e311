"""Generates tests/golden/segment.npz FROM THE REFERENCE'S OWN FUNCTIONS of mimikit/extract/segment.py (:21-160).

Run in the build container only (needs the reference tree, scipy and sklearn):
    python tests/golden/make_golden_segment.py
mimikit/extract/segment.py is imported unmodified through oracle/ref_shim.py; the package object ``mimikit.extract`` is a path-only one made
here, as in make_golden_clusters.py, and ``librosa.sequence`` gets a stand-in module (the shim has ``librosa.util`` only).  numba's ``njit``
is the shim's identity, so the reference's loops run as plain Python.

``discontinuity_scores`` itself cannot run: it asks for ``np.float``, which numpy no longer has, and its ``pwdk_cosine`` allocates 2 k - 1
columns and addresses 2 k + 1, which outside numba raises IndexError for any T > k - 1.  So the pipeline is pinned BY PARTS, as Envelop was:
  * ``checker(h)``;
  * ``convolve_diagonals`` on seeded random diagonals;
  * ``pwdk_cosine(X, 2 h + 1)`` at T <= 2 h, the only sizes at which it stays in bounds, and on those bands the lines of
    ``discontinuity_scores`` between the two defects (slice, ``np.pad``, ``checker``, ``convolve_diagonals``) executed here with the
    reference's functions: ``raw`` before the minimum is subtracted;
  * ``pick_globally_sorted_maxes`` with ``localmax`` below (librosa.util.localmax restated for one axis) put in place of the shim's
    placeholder; scipy's ``minimum_filter1d`` is the real one.
What is committed are seeded float32 inputs and small float64 / int64 results only.  The picker inputs are float32 values handed over as
float64; each must be robust (tests/segment_refs.py: ``robust``) so that the device picker, which reads the float32 values, has to return
the same indices.
"""
import importlib
import os
import sys
import types
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from oracle.ref_shim import REFERENCE_ROOT, load_reference  # noqa: E402
from tests import segment_refs as R  # noqa: E402

OUT = os.path.dirname(os.path.abspath(__file__))

CHECKERS = (1, 2, 6)
CONV = {"a": (41, 2, 30), "b": (42, 6, 21)}                      # name: (seed, h, N outputs)
BANDS = {"a": (51, 6, 12, 9), "b": (52, 2, 4, 5), "c": (53, 12, 24, 33)}      # name: (seed, h_max, T <= 2 h_max, D); a smaller h rides along
BAND_SMALL = {"a": 2, "b": 1, "c": 6}
PICKS = {"a": (61, 60, 4, 4, 0.02), "b": (62, 300, 4, 4, 0.03), "c": (63, 300, 3, 6, 0.05), "d": (64, 200, 9, 2, 0.0),
         "e": (65, 1500, 16, 16, 0.1)}                         # name: (seed, n, wait_before, wait_after, min_strength)


def localmax(x, axis=0):
    x = np.asarray(x)
    p = np.pad(x, 1, mode="edge")
    return (x > p[:-2]) & (x >= p[2:])


def reference_module():
    load_reference()
    pkg = types.ModuleType("mimikit.extract")
    pkg.__path__ = [os.path.join(REFERENCE_ROOT, "mimikit", "extract")]
    sys.modules["mimikit.extract"] = pkg
    seq = types.ModuleType("librosa.sequence")
    seq.dtw = None
    sys.modules["librosa.sequence"] = seq
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")                        # scipy.ndimage.filters is a deprecated name of scipy.ndimage
        seg = importlib.import_module("mimikit.extract.segment")
    seg.localmax = localmax
    return seg


def pick_input(seed, n):
    """a smoothed random walk with a few bumps: peaks of many heights, some closer than the waits"""
    rng = np.random.default_rng(seed)
    x = np.convolve(rng.standard_normal(n + 8), np.hanning(9), mode="valid")[:n] + 0.3 * rng.standard_normal(n)
    return x.astype(np.float32)


def make():
    S = reference_module()
    arrays = {}
    for h in CHECKERS:
        arrays[f"checker_{h}"] = S.checker(h)
    for name, (seed, h, n) in CONV.items():
        k = 2 * h + 1
        d = np.random.default_rng(seed).uniform(0.0, 2.0, (n + k - 1, 2 * k - 1))
        arrays[f"conv_{name}_diagonals"], arrays[f"conv_{name}_out"] = d, S.convolve_diagonals(d, S.checker(h))
    for name, (seed, h, t, dim) in BANDS.items():
        x = np.random.default_rng(seed).uniform(-1.0, 1.0, (t, dim)).astype(np.float32)
        x[t // 2] = 0
        max_kernel = 2 * h + 1
        diagonals = S.pwdk_cosine(np.ascontiguousarray(x, dtype=np.float64), max_kernel)
        arrays[f"band_{name}_x"], arrays[f"band_{name}_diagonals"] = x, diagonals
        for hq in (h, BAND_SMALL[name]):
            k = 2 * hq + 1                                     # segment.py:121-130, its own lines
            kd2 = k // 2
            if k < max_kernel:
                extra = max_kernel - k
                dk = diagonals[:, extra:-extra]
            else:
                dk = diagonals.copy()
            dk = np.pad(dk, ((kd2, kd2), (0, 0)))
            arrays[f"band_{name}_raw_{hq}"] = S.convolve_diagonals(dk, S.checker(kd2, normalize=True))
    for name, (seed, n, wb, wa, ms) in PICKS.items():
        x = pick_input(seed, n)
        x64 = x.astype(np.float64)
        assert R.robust(x64, 1e-9, wb, wa, ms), f"picker input {name} is not robust: choose another seed"
        got = S.pick_globally_sorted_maxes(x64, wb, wa, ms)
        assert len(got) >= 3, (name, got)
        arrays[f"pick_{name}_x"], arrays[f"pick_{name}_out"] = x, np.asarray(got, dtype=np.int64)
        print(f"picker {name}: n {n}, waits {wb, wa}, min_strength {ms}: {len(got)} peaks")
    path = os.path.join(OUT, "segment.npz")
    np.savez_compressed(path, **arrays)
    print(f"segment.npz: {os.path.getsize(path) / 1024:.1f} KiB, {len(arrays)} arrays")


if __name__ == "__main__":
    make()
