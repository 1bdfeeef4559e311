"""Generates tests/golden/samplify.npz from the numpy / scipy restatement of the reference's Samplifyer (tests/samplify_refs.py).

    python tests/golden/make_golden_samplify.py

The reference's own class needs numba and librosa, which are not installed.  What is recorded is its algorithm as restated, on seeded
synthetic signals: every level is the bin sum of a float64 torch.stft magnitude (reflect padding, periodic Hann window - the by-parts
pinning of make_golden_envelope.py) of the length-fixed signal, divided by its maximum and stored as float32; its gradient is the
reference's float32 derivative divided by its largest magnitude; both go through scipy's interp1d(kind="quadratic") to the signal's length,
as the reference's Interpolate.np_func does, and the selection runs on those float32 curves.

A cut is `robust` when every decision on its way leads by more than the derived bounds of the values it compares
(samplify_refs.robust_flags), and `robust_f32` when a float32 transform gives the same cut.  The generator asserts the kind of every
fixture and that at least three quarters of its cuts are robust.
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from tests import samplify_refs as R  # noqa: E402

OUT = os.path.dirname(os.path.abspath(__file__))


def make():
    arrays = {}
    for name in R.FIXTURES:
        r, r32 = R.fixture(name), R.fixture(name, torch.float32)
        n = len(r["cuts"])
        same = len(r32["cuts"]) == n and np.array_equal(r32["coarse_cuts"], r["coarse_cuts"])
        r = dict(r, robust_f32=(r32["cuts"] == r["cuts"]) if same else np.zeros(n, dtype=bool), sensitivity=np.float64(r["sensitivity"]))
        assert 4 * int(r["robust"].sum()) >= 3 * n, (name, int(r["robust"].sum()), n)
        assert 4 * int((r["robust"] & r["robust_f32"]).sum()) >= 3 * n, (name, "float32 transform")
        assert np.all(np.diff(r["coarse_cuts"]) > 0) and not np.isnan(r["scores"]).any()
        for key in R.GOLDEN_KEYS:
            arrays[f"{name}_{key}"] = np.asarray(r[key])
        print(f"{name}: {n} cuts of {len(r['att'])} attacks, {int((r['sides'] == 0).sum())} on the left, {int(r['robust'].sum())} robust, "
              f"{int(r['robust_f32'].sum())} the same from a float32 transform")
    b, d = (R.fixture(k) for k in ("bursts", "dense"))
    assert len(b["cuts"]) >= 6 and (b["sides"] == 1).all() and len(b["cuts"]) < len(b["att"])
    assert len(d["cuts"]) == len(d["att"]) >= 12 and (d["sides"] == 0).any() and (d["sides"] == 1).any()
    path = os.path.join(OUT, "samplify.npz")
    np.savez_compressed(path, **arrays)
    print(f"samplify.npz: {os.path.getsize(path) / 1024:.1f} KiB, {len(arrays)} arrays")


if __name__ == "__main__":
    make()
