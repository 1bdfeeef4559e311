"""CPU checks of tests/kmeans_refs.py and of the KMeans interface: the float64 restatement against sklearn's recorded results of
tests/golden/kmeans.npz and the conditions under which the device must reproduce them exactly, every planted defect visible, the label
rule on float64's own answer and on planted faults, the kernel cases inside the cap of rows left to the second rule, and the completeness
of include/mmk_kmeans.h (its names against native.KMEANS_SYMBOLS, its prototypes against the ctypes signatures, a stream case per entry
point that takes a stream).  No GPU."""
import ctypes as C
import dataclasses
import os
import re

import numpy as np
import pytest
import torch

import mimikit_amd as mmk
from mimikit_amd import native
from mimikit_amd.extract import clusters as CL
from tests import kmeans_refs as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "mmk_kmeans.h")
GOLDEN = os.path.join(ROOT, "tests", "golden", "kmeans.npz")
G = np.load(GOLDEN)
MARGIN = 1e-9


# ------------------------------------------------------------------------------------------------------------------- the interface
def test_package_exports_fields_and_round_trip():
    assert mmk.KMeans is CL.KMeans and "KMeans" in CL.__all__ and callable(CL.lloyd)
    sources = __import__("mimikit_amd.build", fromlist=["SOURCES"])
    assert "kmeans.hip" in sources.SOURCES and any(h.endswith("mmk_kmeans.h") for h in sources.HEADERS)
    km = mmk.KMeans()
    fields = [f.name for f in dataclasses.fields(km) if f.name != "type"]
    assert fields == ["n_clusters", "n_init", "max_iter", "random_seed"]
    assert (km.n_clusters, km.n_init, km.max_iter, km.random_seed) == (16, 2, 100, 42)
    assert (km.labels_, km.cluster_centers_, km.inertia_, km.n_iter_) == (None, None, None, None) and isinstance(km.inv, mmk.Identity)
    other = mmk.KMeans(n_clusters=5, n_init=3, max_iter=7, random_seed=1)
    assert mmk.Config.deserialize(other.serialize()) == other
    chain = mmk.Compose(mmk.MagSpec(), mmk.PCA(16), mmk.KMeans(n_clusters=4))
    assert mmk.Config.deserialize(chain.serialize()) == chain
    text = CL.__doc__
    assert "``KMeans``, ``SpectralClustering`` and ``GCluster`` are not carried over" not in text
    assert "``SpectralClustering`` and ``GCluster`` are not carried over" in text
    for word in ("RandomState", "two small host reads", "argpartition", "N x K", "strict convergence", 'side="left"'):
        assert word in text, word


def test_cpu_tensors_numpy_and_bad_arguments_raise():
    x = torch.rand(40, 5)
    km = mmk.KMeans(n_clusters=4)
    with pytest.raises(RuntimeError, match="MI355X"):
        km.fit(x)
    with pytest.raises(RuntimeError, match="MI355X"):
        km(x)
    with pytest.raises(TypeError):
        km.fit(x.numpy())
    with pytest.raises(NotImplementedError, match="device"):
        km(x.numpy())
    with pytest.raises(NotImplementedError, match="device"):
        km.np_func(x.numpy())
    with pytest.raises(TypeError):
        km.fit(x.double())
    with pytest.raises(ValueError):
        km.fit(x[0])
    with pytest.raises(RuntimeError, match="MI355X"):
        CL.lloyd(x, x[:4])
    with pytest.raises(RuntimeError, match="MI355X"):
        native.kmeans_assign(x, None, x[:4], torch.zeros(40, dtype=torch.int32))
    with pytest.raises(RuntimeError, match="MI355X"):
        native.kmeans_label_sums(x, None, torch.zeros(40, dtype=torch.int32), 4)


# ------------------------------------------------------------------------------------------------------------------- the header
def header_prototypes():
    text = re.sub(r"/\*.*?\*/", " ", open(HEADER).read(), flags=re.S)
    return {m.group(2): (m.group(1), m.group(3)) for m in re.finditer(r"\b(int|size_t)\s+(mmk_[a-z0-9_]+)\s*\(([^;{}]*?)\)\s*;", text)}


def test_header_names_signatures_and_exports():
    protos = header_prototypes()
    assert sorted(protos) == sorted(native.KMEANS_SYMBOLS), "include/mmk_kmeans.h and native.KMEANS_SYMBOLS name different functions"
    assert not set(native.KMEANS_SYMBOLS) & set(native.EXPORTED_SYMBOLS)
    kinds = {"int64_t": C.c_int64, "int32_t": C.c_int32, "size_t": C.c_size_t, "float": C.c_float, "mmk_stream_t": C.c_void_p, "int": C.c_int32}
    lib = native.load_library()
    for name, (res, args) in protos.items():
        want_res, want_args = native._KMEANS_SIGNATURES[name]
        assert want_res is kinds[res], name
        got = [] if args.strip() == "void" else [C.c_void_p if "*" in a else kinds[a.strip().replace("const ", "").split()[0]] for a in args.split(",")]
        assert got == list(want_args), (name, got, want_args)
        assert getattr(lib, name) is not None, f"the library does not export {name}"
    main = open(os.path.join(ROOT, "include", "mmk.h")).read()
    assert "kmeans" not in main.lower(), "include/mmk.h names kmeans: the prototypes live in include/mmk_kmeans.h"
    text = open(HEADER).read()
    for macro, value in (("MMK_KMEANS_MAX_K", native.KMEANS_MAX_K), ("MMK_KMEANS_PP_MAX_TRIALS", native.KMEANS_PP_MAX_TRIALS),
                         ("MMK_KMEANS_MAX_SLABS", native.KMEANS_MAX_SLABS)):
        assert int(re.search(rf"#define {macro} (\d+)", text).group(1)) == value, macro
    assert native.KMEANS_MAX_K == 256 and native.KMEANS_PP_MAX_TRIALS == 8
    assert 2 + int(np.log(native.KMEANS_MAX_K)) <= native.KMEANS_PP_MAX_TRIALS, "the trials of the largest K fit one seeding step"


def test_every_stream_entry_point_has_a_stream_case():
    from tests import test_gpu_kmeans as T
    with_stream = sorted(name for name, (_, args) in header_prototypes().items() if "mmk_stream_t" in args)
    assert with_stream == ["mmk_kmeans_assign_f32", "mmk_kmeans_label_sums_f64", "mmk_kmeans_pp_step_f64"]
    assert sorted({c.entry for c in T.STREAM_CASES}) == with_stream
    assert "returns without waiting" in open(HEADER).read()


def test_workspace_sizes_do_not_grow_with_n():
    lib = native.load_library()
    for d, k in ((16, 16), (1025, 256), (1, 1)):
        sizes = [lib.mmk_kmeans_label_sums_workspace_bytes(n, d, k) for n in (1, 64, 65, 1 << 16, 1 << 20, 1 << 30)]
        assert all(a <= b for a, b in zip(sizes, sizes[1:])) and sizes[-1] == sizes[-2], (d, k, sizes)
        assert sizes[-1] <= native.KMEANS_MAX_SLABS * (k * (d + 1) + 1) * 8
        assert sizes[0] == (k * (d + 1) + native.KMEANS_MAX_SLABS) * 8                  # one slab
    assert lib.mmk_kmeans_label_sums_workspace_bytes(0, 4, 4) == 0 and lib.mmk_kmeans_label_sums_workspace_bytes(4, 0, 4) == 0
    assert lib.mmk_kmeans_pp_step_workspace_bytes() == (native.KMEANS_MAX_SLABS * native.KMEANS_PP_MAX_TRIALS + 1) * 8


def test_entry_points_refuse_bad_arguments_before_any_launch():
    lib = native.load_library()
    buf = (C.c_double * 64)()
    p = C.addressof(buf)
    big = 1 << 30
    for n, d, k in ((0, 4, 4), (4, 0, 4), (4, 4, 0)):
        assert lib.mmk_kmeans_assign_f32(p, 4, None, n, d, p, 4, p, k, p, None, None, None) == -1, (n, d, k)
        assert lib.mmk_kmeans_label_sums_f64(p, 4, None, n, d, p, k, p, p, None, 0, None, None, p, big, None) == -1, (n, d, k)
    assert lib.mmk_kmeans_assign_f32(p, 4, None, 4, 4, p, 4, p, native.KMEANS_MAX_K + 1, p, None, None, None) == -3
    assert "MMK_KMEANS_MAX_K" in lib.mmk_last_error().decode()
    assert lib.mmk_kmeans_assign_f32(p, 4, None, 4, 4, None, 4, p, 4, p, None, None, None) == -1                   # no centres
    assert lib.mmk_kmeans_assign_f32(p + 2, 4, None, 4, 4, p, 4, p, 4, p, None, None, None) == -1                  # x not 4-byte aligned
    assert lib.mmk_kmeans_assign_f32(p, 4, None, 4, 4, p, 4, p, 4, p, None, p + 4, None) == -1                     # changed not 8-byte aligned
    assert lib.mmk_kmeans_assign_f32(p, -1, None, 4, 4, p, 4, p, 4, p, None, None, None) == -1                     # negative stride
    assert lib.mmk_kmeans_label_sums_f64(p, 4, None, 4, 4, p, 4, p, p, None, 0, p, None, p, big, None) == -1        # row_d2 without centres
    assert lib.mmk_kmeans_label_sums_f64(p, 4, None, 4, 4, p, 4, p, p, None, 0, None, None, p, 8, None) == -4       # workspace too small
    assert lib.mmk_kmeans_label_sums_f64(p, 4, None, 4, 4, p, 4, p, p, None, 0, None, None, None, big, None) == -4  # no workspace
    assert lib.mmk_kmeans_label_sums_f64(p, 4, None, 4, 4, p, 4, p, p, None, 0, None, None, p + 4, big, None) == -4  # misaligned workspace
    assert lib.mmk_kmeans_label_sums_f64(p, 4, None, 4, 4, p, 1 << 20, p, p, None, 0, None, None, p, 1 << 40, None) == -3      # counts beyond a wave's LDS
    for n, d, t in ((0, 4, 1), (4, 0, 1), (4, 4, 0)):
        assert lib.mmk_kmeans_pp_step_f64(p, 4, None, n, d, p, t, p, p, p, p, big, None) == -1, (n, d, t)
    assert lib.mmk_kmeans_pp_step_f64(p, 4, None, 4, 4, p, native.KMEANS_PP_MAX_TRIALS + 1, p, p, p, p, big, None) == -3
    assert lib.mmk_kmeans_pp_step_f64(p, 4, None, 4, 4, p, 2, p, p, p, p, 64, None) == -4
    assert lib.mmk_kmeans_pp_step_f64(p, 4, None, 4, 4, p + 4, 2, p, p, p, p, big, None) == -1                     # cand not 8-byte aligned


# ------------------------------------------------------------------------------------------------------------------- the restatement
@pytest.mark.parametrize("name", sorted(R.FIT_FIXTURES))
def test_restatement_equals_sklearn_and_exactness_is_a_fair_demand(name):
    k, seed, least_iter, _ = R.FIT_FIXTURES[name][2:]
    x = R.fit_corpus(name)
    assert x.dtype == np.float32 and R.checksum(x) == float(G[f"{name}_checksum"]), "the corpus is not the seeded recipe the golden was made from"
    res = R.fit_result(name)
    assert np.array_equal(res["seed_rows"], G[f"{name}_seed_rows"]), "seed rows"
    assert np.array_equal(res["labels"], G[f"{name}_labels"]) and res["n_iter"] == int(G[f"{name}_n_iter"]) >= least_iter
    assert res["winner"] == int(G[f"{name}_winner"])
    err = np.abs(res["centres"].astype(np.float64) - G[f"{name}_centres"]).max()
    print(f"{name}: n_iter {res['n_iter']}, run {res['winner']} kept, gap ratio {res['ratio']:.2f}, draw margin {res['margin']:.2e}, shift margin "
          f"{res['shift_margin']:.2e}; centres differ from sklearn's float32 ones by {err:.2e}, inertia {res['inertia']:.9g} / {float(G[f'{name}_inertia']):.9g}")
    assert res["ratio"] >= 1.0 and res["margin"] >= MARGIN and res["shift_margin"] >= 1e-6
    assert err <= 1e-4 * np.abs(G[f"{name}_centres"]).max() and abs(res["inertia"] - float(G[f"{name}_inertia"])) <= 1e-4 * res["inertia"]


def test_both_seedings_win_somewhere_and_the_file_is_small():
    assert {int(G[f"{name}_winner"]) for name in R.FIT_FIXTURES} == {0, 1}
    assert os.path.getsize(GOLDEN) < 100 * 1024
    assert str(G["sklearn_version"]) and str(G["numpy_version"])
    shapes = {name: R.fit_corpus(name).shape for name in R.FIT_FIXTURES}
    assert shapes == dict(blobs=(600, 16), overlap=(2000, 16), wide=(400, 257), spectra=(1000, 129), renamed=(300, 4))
    assert int(G["overlap_n_iter"]) >= 15 and int(G["spectra_n_iter"]) >= 10
    assert float(R.fit_corpus("spectra").min()) >= 0 and float(R.fit_corpus("spectra").mean()) > 10


@pytest.mark.parametrize("name", sorted(R.LLOYD_FIXTURES))
def test_lloyd_restatement_from_an_init_with_an_empty_cluster(name):
    x, init = R.lloyd_corpus(name)
    assert R.checksum(x) == float(G[f"{name}_checksum"])
    res = R.lloyd_result(name)
    mu = res["mu"]
    first = R.first_argmax(R.key64(R.centred(x, mu), R.centred(init, mu)))
    assert (np.bincount(first, minlength=init.shape[0]) == 0).sum() == 1, "exactly one cluster is empty at iteration 0"
    assert np.array_equal(res["labels"], G[f"{name}_labels"]) and res["n_iter"] == int(G[f"{name}_n_iter"])
    assert res["ratio"] >= 1.0 and res["shift_margin"] >= 1e-6
    assert (np.bincount(res["labels"], minlength=init.shape[0]) > 0).all()
    print(f"{name}: n_iter {res['n_iter']}, gap ratio {res['ratio']:.2f}, sizes {np.bincount(res['labels']).tolist()}")


@pytest.mark.parametrize("defect", R.DEFECTS)
def test_every_defect_is_noticed(defect):
    seen = []
    for name in sorted(R.FIT_FIXTURES):
        res = R.fit_result(name, defect)
        if not (np.array_equal(res["labels"], G[f"{name}_labels"]) and np.array_equal(res["seed_rows"], G[f"{name}_seed_rows"])
                and res["n_iter"] == int(G[f"{name}_n_iter"])):
            seen.append(name)
    for name in sorted(R.LLOYD_FIXTURES):
        res = R.lloyd_result(name, defect)
        if not (np.array_equal(res["labels"], G[f"{name}_labels"]) and res["n_iter"] == int(G[f"{name}_n_iter"])):
            seen.append(name)
    x, offset, centres = R.special_case()
    key = R.key64(R.centred(x, offset), centres)
    if defect == "ties_high" and not np.array_equal(R.first_argmax(key, high=True), R.first_argmax(key)):
        seen.append("identical centres")
    # a draw that falls EXACTLY on a boundary of the scan (closest = 0, 4, 4; u pot = 4): "left" takes row 1, "right" row 2 - RandomState's
    # draws on a real corpus never do, so no fixture can show this defect
    on_edge = np.array([[0.0], [2.0], [-2.0]])
    side = "right" if defect == "searchsorted_right" else "left"
    if not np.array_equal(R.seeding64(on_edge, 0, np.array([[0.5, 0.5]]), side=side)[0], [0, 1]):
        seen.append("a draw on a boundary")
    print(f"{defect}: changes seed rows, labels or n_iter of {seen}")
    assert seen, f"the defect {defect} changes no case"


# ------------------------------------------------------------------------------------------------------------------- the kernel cases
@pytest.mark.parametrize("k", R.KS)
def test_kernel_cases_leave_few_rows_to_the_second_rule(k):
    worst = 0.0
    for n in R.NS:
        for d in R.DS:
            x, offset, centres = R.kernel_case(n, d, k)
            xp = R.centred(x, offset)
            key, bound = R.key64(xp, centres), R.key_bound(xp, centres)
            best, safe = R.safe_rows(key, bound)
            left = int((~safe).sum())
            worst = max(worst, left / n)
            assert left <= R.LEFT_CAP * n, f"n {n}, d {d}, k {k}: {left} rows are left to the second rule"
            bad, _ = R.label_rule_violations(best, key[np.arange(n), best], key, bound)
            assert not bad.any()
    print(f"k {k}: at most {worst:.4f} of a case's rows are left to the second rule (cap {R.LEFT_CAP})")


def test_label_rule_sees_planted_faults_and_the_special_inputs_are_what_they_say():
    x, offset, centres = R.special_case()
    xp = R.centred(x, offset)
    key, bound = R.key64(xp, centres), R.key_bound(xp, centres)
    best = R.first_argmax(key)
    assert not R.label_rule_violations(best, None, key, bound)[0].any()
    wrong = (best + 2) % centres.shape[0]
    assert R.label_rule_violations(wrong, None, key, bound)[0].mean() > 0.9
    assert R.label_rule_violations(np.full_like(best, -7), None, key, bound)[0].all()
    off_key = key[np.arange(200), best] + 3 * bound[np.arange(200), best]
    assert R.label_rule_violations(best, off_key, key, bound)[0].all()
    assert best[10] == R.SAME_CENTRES[0] and (best != R.SAME_CENTRES[1]).all() and (best != R.FAR_CENTRE).all()
    assert np.array_equal(x[R.COPY_ROWS[0]], x[R.COPY_ROWS[1]]) and not xp[R.ZERO_ROW].any()
    sums, counts, _ = R.label_sums64(xp, best, centres.shape[0])
    assert counts[R.FAR_CENTRE] == 0 and not sums[R.FAR_CENTRE].any() and counts.sum() == 200


def test_key_bound_holds_for_a_float32_replay_and_a_near_miss_leaves_it():
    """the kernel's roundings replayed in numpy float32 (an unfused chain: one more rounding per term, so within a factor of two)"""
    x, offset, centres = R.kernel_case(129, 129, 33)
    xp = R.centred(x, offset)
    acc = np.zeros((129, 33), dtype=np.float32)
    for c in range(129):
        acc = (acc + (xp[:, c, None] * centres[None, :, c]).astype(np.float32)).astype(np.float32)
    got = (acc + (-0.5 * (centres.astype(np.float64) ** 2).sum(-1)).astype(np.float32)[None, :]).astype(np.float32)
    key, bound = R.key64(xp, centres), R.key_bound(xp, centres)
    worst = float((np.abs(got.astype(np.float64) - key) / bound).max())
    print(f"unfused float32 replay: worst key error / bound {worst:.3f}")
    assert worst <= 2.0
    assert (np.abs(R.key64(xp, centres, halved=False) - key) > bound).mean() > 0.9, "a key with |c|^2 not halved stays inside the bound"
    assert (np.abs(R.key64(x, centres) - key) > bound).mean() > 0.9, "a key of the uncentred rows stays inside the bound"


def test_seeding_step_restatement_is_the_seeding():
    x = R.fit_corpus("blobs")
    mu, _ = R.centre_stats(x)
    xp = R.centred(x, mu).astype(np.float64)
    first, uniforms = R.draws(42, x.shape[0], 16, 2)[0]
    rows, _ = R.seeding64(xp, first, uniforms)
    closest, pot, t, _ = R.pp_step64(xp, [first], np.full(x.shape[0], np.inf))
    got = [first]
    for u in uniforms:
        cand = np.clip(np.searchsorted(np.cumsum(closest), u * pot), None, x.shape[0] - 1)
        closest, pot, t, _ = R.pp_step64(xp, cand, closest)
        got.append(int(cand[t]))
    assert got == rows.tolist() == G["blobs_seed_rows"][0].tolist()
