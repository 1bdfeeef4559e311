"""Generates tests/golden/nmf.npz FROM THE REFERENCE'S OWN NMF (mimikit/features/functionals.py:1141-1170: sklearn.decomposition.NMF with
n_components, tol, max_iter and random_state).

Run in the build container only (needs the reference tree and sklearn):
    python tests/golden/make_golden_nmf.py
mimikit/features/functionals.py is imported unmodified through oracle/ref_shim.py.  The inputs are regenerated from their seeds
(tests/nmf_refs.py: fixture_frames) and are not committed.  Per fixture the file holds the reference's W, components_ and n_iter_ at
random_seed 42 on the float64 copies of the float32 frames, sklearn's transform of the unseen batch with that fit, and as information
the spread across random_seed 42, 7 and 0 and the difference of the reference's float32 run, each relative to the largest entry.

Asserted here: the three seeds agree to 1e-10 of the largest entry in W and components_, so does the restatement of tests/nmf_refs.py
(both starts), and every iteration count is equal.
"""
import os
import sys
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from oracle import ref_shim  # noqa: E402
from tests import nmf_refs as R  # noqa: E402

OUT = os.path.dirname(os.path.abspath(__file__))
SEEDS = (42, 7, 0)
AGREE = 1e-10


def fitted_reference(NMF, f, seed, x):
    """the reference's result and the sklearn estimator behind it: the functional keeps no estimator, so the same call is made on
    sklearn's class with the functional's four fields to reach components_ and n_iter_ (asserted equal to the functional's output)"""
    from sklearn.decomposition import NMF as skNMF
    func = NMF(n_components=f["k"], tol=f["tol"], max_iter=f["max_iter"], random_seed=seed)
    w = np.asarray(func(x))
    est = skNMF(n_components=func.n_components, tol=func.tol, max_iter=func.max_iter, random_state=func.random_seed)
    assert np.array_equal(est.fit_transform(x), w), "the reference's functional is not sklearn's NMF with its four fields"
    return w, est


def make():
    NMF = ref_shim.load_reference().functionals.NMF
    arrays = {}
    warnings.simplefilter("ignore")                              # (the cap fixtures warn, as they must)
    for name in R.NAMES:
        r = R.fixture_case(name)
        f, x64 = r["f"], r["x"].astype(np.float64)
        runs = [fitted_reference(NMF, f, seed, x64) for seed in SEEDS]
        w, est = runs[0]
        h, top_w, top_h = est.components_, np.abs(runs[0][0]).max(), np.abs(est.components_).max()
        seeds = max(max(np.abs(ww - w).max() / top_w, np.abs(e.components_ - h).max() / top_h) for ww, e in runs[1:])
        assert seeds <= AGREE, f"{name}: the reference's seeds differ by {seeds:.2e}"
        assert all(e.n_iter_ == est.n_iter_ for _, e in runs), f"{name}: the reference's seeds stop at {[e.n_iter_ for _, e in runs]}"
        worst = 0.0
        for route in ("gram", "svd"):
            o = R.fit64(r["x"], f["k"], f["tol"], f["max_iter"], route=route)
            worst = max(worst, np.abs(o["w"] - w).max() / top_w, np.abs(o["h"] - h).max() / top_h)
            assert o["n_iter"] == est.n_iter_, f"{name}: the restatement ({route}) stops at {o['n_iter']}, the reference at {est.n_iter_}"
        assert worst <= AGREE, f"{name}: the restatement is {worst:.2e} from the reference"
        tw = est.transform(r["y"].astype(np.float64))
        terr = np.abs(r["tw"] - tw).max() / np.abs(tw).max()
        assert terr <= AGREE, f"{name}: the restatement's transform is {terr:.2e} from the reference's"
        w32, e32 = fitted_reference(NMF, f, 42, r["x"].copy())
        f32 = np.abs(w32.astype(np.float64) - w).max() / top_w
        arrays[f"{name}_w"] = w.astype(np.float32) if name == "runs" else w
        arrays[f"{name}_components"] = h
        arrays[f"{name}_n_iter"] = np.int64(est.n_iter_)
        arrays[f"{name}_transform"] = tw
        arrays[f"{name}_seed_spread"] = np.float64(seeds)
        arrays[f"{name}_f32_diff"] = np.float64(f32)
        arrays[f"{name}_f32_n_iter"] = np.int64(e32.n_iter_)
        print(f"NMF {name} {r['x'].shape}, {f['k']} components, tol {f['tol']:g}, max_iter {f['max_iter']}: n_iter {est.n_iter_}, seeds agree to "
              f"{seeds:.1e}, restatement - reference {worst:.1e}, transform {terr:.1e}; the reference's float32 run: {e32.n_iter_} iterations, "
              f"{f32:.1e} away")
    path = os.path.join(OUT, "nmf.npz")
    np.savez_compressed(path, **arrays)
    print(f"nmf.npz: {os.path.getsize(path) / 1024:.1f} KiB, {len(arrays)} arrays")


if __name__ == "__main__":
    make()
