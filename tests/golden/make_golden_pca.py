"""Generates tests/golden/pca.npz FROM THE REFERENCE'S OWN PCA (mimikit/features/functionals.py:1114-1138: sklearn's StandardScaler, then
sklearn's PCA).

Run in the build container only (needs the reference tree, sklearn and scipy):
    python tests/golden/make_golden_pca.py
mimikit/features/functionals.py is imported unmodified through oracle/ref_shim.py.  The inputs are regenerated from their seeds
(tests/pca_refs.py: fixture_frames) and are not committed; what is committed are the reference's float64 scores of the five small
fixtures (its result on the float64 copies of the float32 frames) and, as information, the largest difference between its float32 and
its float64 run relative to the largest score.

The restatement of tests/pca_refs.py is asserted against the reference here with the bounds of that module at float64's unit: the
scores to the a-posteriori vector bound of the reference's own components (z^T scores, normalised) plus
(d + 2) v sum |z| |v|; the columns of the null regime by their size only.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from oracle import ref_shim  # noqa: E402
from tests import pca_refs as R  # noqa: E402

OUT = os.path.dirname(os.path.abspath(__file__))


def make():
    PCA = ref_shim.load_reference().functionals.PCA
    arrays = {}
    for name in R.GOLDEN:
        x, p, e, allow, null, margins = R.fixture_case(name)
        k = p["k"]
        s64 = np.asarray(PCA(n_components=k)(x.astype(np.float64)), dtype=np.float64)
        s32 = np.asarray(PCA(n_components=k)(x.copy()), dtype=np.float64)
        top = np.abs(s64).max()
        # the reference's components from its scores: z^T z v = (N - 1) lambda v, so v is z^T s normalised - outside the null regime, where
        # the restatement's own vector stands in (only the size of those scores is looked at)
        comps = (p["z"].T @ s64).T
        comps = np.where(null[:, None], p["comps"], comps / np.sqrt((comps * comps).sum(1))[:, None])
        r = R.check_components(p, comps, f"{name}: the reference's components", allow)
        bound = (np.sqrt((p["z"] ** 2).sum(1))[:, None] * np.where(r["null"], 0.0, r["vec_bound"])[None, :]
                 + (p["d"] + 2) * R.V * (np.abs(p["z"]) @ (np.abs(p["comps"]).T + np.where(r["null"], 0.0, r["vec_bound"])[None, :])))
        err = np.abs(s64 - p["scores"])
        reg = ~r["null"]
        assert (err[:, reg] <= bound[:, reg]).all(), f"{name}: the restatement is {(err[:, reg] / bound[:, reg]).max():.2f} bounds from the reference"
        size = np.sqrt((p["n"] - 1) * (np.maximum(p["evals"][:k], 0) + 2 * allow))
        assert (np.abs(s64[:, r["null"]]) <= size[r["null"]]).all() and (np.abs(p["scores"][:, r["null"]]) <= size[r["null"]]).all()
        arrays[f"{name}_scores"] = s64
        arrays[f"{name}_f32_diff"] = np.float64(np.abs(s32 - s64)[:, reg].max() / top)
        print(f"PCA {name} {x.shape}, {k} components: restatement - reference {err[:, reg].max() / top:.1e} of the largest score "
              f"(worst error / bound {(err[:, reg] / bound[:, reg]).max():.3f}), the reference's float32 run differs by "
              f"{float(arrays[f'{name}_f32_diff']):.1e}, {int(r['null'].sum())} null columns (|score| up to "
              f"{np.abs(s64[:, r['null']]).max() if r['null'].any() else 0:.1e}, bound {size[r['null']].max() if r['null'].any() else 0:.1e}), "
              f"margins {margins}")
    path = os.path.join(OUT, "pca.npz")
    np.savez_compressed(path, **arrays)
    print(f"pca.npz: {os.path.getsize(path) / 1024:.1f} KiB, {len(arrays)} arrays")


if __name__ == "__main__":
    make()
