"""Generates tests/golden/kmeans.npz FROM sklearn.cluster.KMeans / kmeans_plusplus on the seeded corpora of tests/kmeans_refs.py.  CPU only.

    python -m tests.golden.make_golden_kmeans            (from the repository root; needs scikit-learn)

The file holds results only - per case the seed rows, labels_, cluster_centers_, inertia_ and n_iter_ that sklearn gave, the sklearn and
numpy versions, and a float64 checksum of the corpus, which the tests regenerate from its seed.  A case is written only where exact
agreement is a fair demand of a correct fp32 device path; the generator asserts, and refuses the case otherwise:
  - the float64 restatement (kmeans_refs.fit64 / lloyd_from64) reproduces sklearn's seed rows, labels_ and n_iter_ exactly;
  - every seeding draw lies at least 1e-9 pot from the nearest boundary of the scan, and the winning candidate's pot at least that far below
    every other candidate row's (a float64 scan or sum in another order moves either by at most N 2^-53 relative);
  - at every iteration every frame's gap between its best and second-best float64 key is at least twice the derived fp32 bound, the
    centres' own rounding included (kmeans_refs.gap_ratio >= 1);
  - the centres' shift stays 1e-6 tol away from tol wherever it is tested;
  - the case takes at least the iterations kmeans_refs.FIT_FIXTURES asks of it.
"""
import os
import sys

import numpy as np
import sklearn
from sklearn.cluster import KMeans, kmeans_plusplus

from tests import kmeans_refs as R

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "kmeans.npz")
MARGIN = 1e-9
SHIFT_MARGIN = 1e-6


def sklearn_seed_rows(x, k, seed, n_init):
    """the rows sklearn's seedings choose: KMeans.fit centres x with its float32 column mean and calls kmeans_plusplus once per run on ONE
    RandomState"""
    rs = np.random.RandomState(seed)
    xc = x - x.mean(axis=0)
    return np.array([kmeans_plusplus(xc, k, random_state=rs)[1] for _ in range(n_init)])


def conditions(name, res, least_iter=1):
    assert res["margin"] >= MARGIN, f"{name}: a draw or a pot lies {res['margin']:.2e} pot from a boundary"
    assert res["ratio"] >= 1.0, f"{name}: the smallest gap is {res['ratio']:.3f} x twice the bound"
    assert res["shift_margin"] >= SHIFT_MARGIN, f"{name}: a shift lies {res['shift_margin']:.2e} tol from tol"
    assert res["n_iter"] >= least_iter, f"{name}: {res['n_iter']} iterations, at least {least_iter} are asked for"


def main():
    out = dict(sklearn_version=np.array(sklearn.__version__), numpy_version=np.array(np.__version__))
    winners = set()
    for name, (_, _, k, seed, least_iter, max_iter) in R.FIT_FIXTURES.items():
        x = R.fit_corpus(name)
        km = KMeans(n_clusters=k, n_init=2, max_iter=max_iter, random_state=seed).fit(x.copy())
        rows = sklearn_seed_rows(x, k, seed, 2)
        res = R.fit_result(name)
        assert np.array_equal(res["seed_rows"], rows), f"{name}: the restatement seeds {res['seed_rows'].tolist()}, sklearn {rows.tolist()}"
        assert np.array_equal(res["labels"], km.labels_), f"{name}: {int((res['labels'] != km.labels_).sum())} labels differ from sklearn's"
        assert res["n_iter"] == km.n_iter_, f"{name}: n_iter {res['n_iter']}, sklearn {km.n_iter_}"
        conditions(name, res, least_iter)
        winners.add(res["winner"])
        print(f"{name} {x.shape}, K {k}: n_iter {km.n_iter_}, run {res['winner']} kept, gap ratio {res['ratio']:.2f}, draw margin {res['margin']:.2e}, "
              f"shift margin {res['shift_margin']:.2e}, inertia {km.inertia_:.6g} (float64 {res['inertia']:.9g})")
        out.update({f"{name}_seed_rows": rows, f"{name}_labels": km.labels_.astype(np.int64), f"{name}_centres": km.cluster_centers_.astype(np.float32),
                    f"{name}_inertia": np.array(km.inertia_, dtype=np.float64), f"{name}_n_iter": np.array(km.n_iter_), f"{name}_winner": np.array(res["winner"]),
                    f"{name}_checksum": np.array(R.checksum(x))})
    assert winners == {0, 1}, f"the kept runs are {winners}: one case where the first seeding wins and one where the second does are asked for"
    for name in R.LLOYD_FIXTURES:
        x, init = R.lloyd_corpus(name)
        km = KMeans(n_clusters=init.shape[0], init=init.copy(), n_init=1, max_iter=100).fit(x.copy())
        res = R.lloyd_result(name)
        first = R.lloyd_from64(x, init, max_iter=1)
        assert np.array_equal(res["labels"], km.labels_) and res["n_iter"] == km.n_iter_, f"{name}: the restatement differs from sklearn"
        assert (np.bincount(R.first_argmax(R.key64(R.centred(x, res["mu"]), R.centred(init, res["mu"]))), minlength=init.shape[0]) == 0).sum() == 1, \
            f"{name}: not exactly one empty cluster at iteration 0"
        conditions(name, dict(res, margin=np.inf))
        print(f"{name} {x.shape}, K {init.shape[0]}: n_iter {km.n_iter_}, gap ratio {res['ratio']:.2f}, sizes {np.bincount(km.labels_).tolist()}, "
              f"after one iteration {np.bincount(first['labels'], minlength=init.shape[0]).tolist()}")
        out.update({f"{name}_labels": km.labels_.astype(np.int64), f"{name}_centres": km.cluster_centers_.astype(np.float32),
                    f"{name}_inertia": np.array(km.inertia_, dtype=np.float64), f"{name}_n_iter": np.array(km.n_iter_), f"{name}_checksum": np.array(R.checksum(x))})
    np.savez_compressed(OUT, **out)
    print(f"wrote {OUT}: {os.path.getsize(OUT)} bytes")


if __name__ == "__main__":
    sys.exit(main())
