"""Writes tests/golden/factor_analysis.npz: recorded results of sklearn's FactorAnalysis on the fixtures of tests/factor_analysis_refs.py.
Run by hand where sklearn and the reference tree are present (`python tests/golden/make_golden_factor_analysis.py`), not by the tests.

The inputs are regenerated from their seeds (tests/factor_analysis_refs.py: fixture_frames) and are not committed.  Per fixture:
    <name>_components, _noise_variance, _loglike, _n_iter, _scores     sklearn.decomposition.FactorAnalysis(svd_method="lapack") on the
                                                                       float64 copy of the float32 frames: the exact method
    <name>_ref_scores, _ref_n_iter                                     the reference's own mimikit.features.functionals.FactorAnalysis
                                                                       (sklearn's default, randomised method at random_seed 42), imported
                                                                       unmodified through oracle/ref_shim.py
    <name>_ref_deviation                                               r_i: the largest deviation of the reference's scores from the float64
                                                                       restatement's (fa64), up to one sign per component - the reference's
                                                                       own approximation error, not a bound on the code under test
"""
import os
import sys
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from oracle import ref_shim  # noqa: E402
from tests import factor_analysis_refs as R  # noqa: E402

OUT = os.path.dirname(os.path.abspath(__file__))


def main():
    from sklearn.decomposition import FactorAnalysis as skFA
    RefFA = ref_shim.load_reference().functionals.FactorAnalysis
    arrays = {}
    warnings.simplefilter("ignore")                              # (the max_iter fixture warns, as it must)
    for name in R.NAMES:
        f = R.FIXTURES[name]
        x = R.fixture_frames(name)
        exact = skFA(n_components=f["k"], tol=f["tol"], max_iter=f["max_iter"], svd_method="lapack")
        scores = exact.fit_transform(x.astype(np.float64))
        arrays[f"{name}_components"] = exact.components_
        arrays[f"{name}_noise_variance"] = exact.noise_variance_
        arrays[f"{name}_loglike"] = np.asarray(exact.loglike_, dtype=np.float64)
        arrays[f"{name}_n_iter"] = np.int64(exact.n_iter_)
        arrays[f"{name}_scores"] = scores
        func = RefFA(n_components=f["k"], tol=f["tol"], max_iter=f["max_iter"], random_seed=42)
        ref_scores = np.asarray(func(x.copy()))
        arrays[f"{name}_ref_scores"] = ref_scores
        probe = skFA(n_components=f["k"], tol=f["tol"], max_iter=f["max_iter"], random_state=42).fit(x.copy())
        arrays[f"{name}_ref_n_iter"] = np.int64(probe.n_iter_)
        mine = R.fixture_case(name)["scores"]
        arrays[f"{name}_ref_deviation"] = np.float64(np.abs(R.align(ref_scores, mine, by_rows=False) - mine).max())
        print(f"{name}: n_iter exact {exact.n_iter_}, reference {probe.n_iter_}, restatement {R.fixture_case(name)['n_iter']}; reference scores "
              f"{ref_scores.dtype}, deviation from the restatement {arrays[f'{name}_ref_deviation'] / np.abs(mine).max():.2e} of the largest score")
    path = os.path.join(OUT, "factor_analysis.npz")
    np.savez_compressed(path, **arrays)
    print(f"factor_analysis.npz: {os.path.getsize(path) / 1024:.1f} KiB, {len(arrays)} arrays")


if __name__ == "__main__":
    main()
