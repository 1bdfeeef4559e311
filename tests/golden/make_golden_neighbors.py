"""Generates tests/golden/neighbors.npz FROM THE REFERENCE'S OWN nearest_neighbor, AngularDistance, cum_entropy and hist_transform.

Run in the build container only (needs the reference tree):
    python tests/golden/make_golden_neighbors.py
mimikit/extract/from_neighbors.py and mimikit/modules/loss_functions.py are imported unmodified through oracle/ref_shim.py; the package
object ``mimikit.extract`` is a path-only one made here, because the package's own __init__ star-imports modules that need sklearn.  What
is committed are seeded float32 / int64 inputs and the reference's outputs only.

What the reference's code does, recorded as it is:
  * nearest_neighbor(X, Y) as written builds AngularDistance() with its default reduction="mean": D_xy is a scalar, and the function
    returns (the mean distance, index 0) for any input - ``nn_default_*`` keeps that as a record of the defect.  The evident meaning,
    AngularDistance(reduction="none")(X, Y) followed by torch.min(dim=-1), is what ``nn_*_dists`` / ``nn_*_index`` hold (the
    full distance matrix is not kept: the file stays below envelope.npz).
  * cum_entropy(n) with its default neg_diff=True raises IndexError (torch.diff(..., dim=1) on a 1-D tensor): asserted here, nothing to
    record.  neg_diff=False is recorded with reduce="sum" and reduce="none".
  * repeat_rate raises TypeError: asserted here, out of scope.
"""
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from oracle.ref_shim import REFERENCE_ROOT, load_reference  # noqa: E402

OUT = os.path.dirname(os.path.abspath(__file__))
torch.set_grad_enabled(False)

N, M, D = 50, 200, 33
ENTROPY_T, ENTROPY_VALUES = 40, 7


def reference_modules():
    load_reference()
    import importlib
    pkg = types.ModuleType("mimikit.extract")
    pkg.__path__ = [os.path.join(REFERENCE_ROOT, "mimikit", "extract")]
    sys.modules["mimikit.extract"] = pkg
    return importlib.import_module("mimikit.extract.from_neighbors"), importlib.import_module("mimikit.modules.loss_functions")


def make():
    FN, LF = reference_modules()
    rng = np.random.default_rng(795)
    arrays = {}
    for name, lo in (("nonneg", 0.0), ("signed", -1.0)):
        x = rng.uniform(lo, 1.0, size=(N, D)).astype(np.float32)
        y = rng.uniform(lo, 1.0, size=(M, D)).astype(np.float32)
        Dxy = LF.AngularDistance(reduction="none")(torch.from_numpy(x.copy()), torch.from_numpy(y.copy()))
        dists, nn = torch.min(Dxy, dim=-1)
        arrays[f"nn_{name}_x"], arrays[f"nn_{name}_y"] = x, y
        arrays[f"nn_{name}_dists"], arrays[f"nn_{name}_index"] = dists.numpy(), nn.numpy()
        d0, i0 = FN.nearest_neighbor(torch.from_numpy(x.copy()), torch.from_numpy(y.copy()))
        assert d0.dim() == 0 and int(i0) == 0, "the reference's nearest_neighbor no longer reduces to a scalar"
        arrays[f"nn_default_{name}_dist"], arrays[f"nn_default_{name}_index"] = d0.numpy(), i0.numpy()

    rows = {"random": rng.integers(0, ENTROPY_VALUES, size=ENTROPY_T).astype(np.int64) * 1000 + 3,
            "same": np.full(ENTROPY_T, 12345, dtype=np.int64),
            "distinct": rng.permutation(ENTROPY_T).astype(np.int64) * 7}
    for name, n in rows.items():
        t = torch.from_numpy(n.copy())
        arrays[f"ce_{name}_items"] = n
        arrays[f"ce_{name}_sum"] = FN.cum_entropy(t, reduce="sum", neg_diff=False).numpy()
        arrays[f"ce_{name}_none"] = FN.cum_entropy(t, reduce="none", neg_diff=False).numpy()
    try:
        FN.cum_entropy(torch.from_numpy(rows["random"].copy()))
        raise AssertionError("the reference's cum_entropy(neg_diff=True) no longer raises")
    except IndexError:
        pass
    try:
        FN.repeat_rate(torch.from_numpy(rows["random"].copy()).float(), 8, 4)
        raise AssertionError("the reference's repeat_rate no longer raises")
    except TypeError:
        pass

    h = (rng.integers(0, 64, size=(3, 30))).astype(np.float32)
    arrays["hist_x"] = h
    arrays["hist_2d_16"] = FN.hist_transform(torch.from_numpy(h.copy()), bins=16).numpy()
    arrays["hist_1d_16"] = FN.hist_transform(torch.from_numpy(h[0].copy()), bins=16).numpy()
    path = os.path.join(OUT, "neighbors.npz")
    np.savez(path, **arrays)
    print(f"neighbors.npz: {os.path.getsize(path) / 1024:.1f} KiB, {len(arrays)} arrays")


if __name__ == "__main__":
    make()
