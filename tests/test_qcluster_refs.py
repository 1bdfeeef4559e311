"""CPU checks of tests/qcluster_refs.py: the float64 restatement of QCluster against the reference's recorded results of
tests/golden/qcluster.npz, every fixture gap against the device's derived bounds, the union-find of the edge-list cases against scipy, the
top-k index rule on float64's own answer and on planted faults, and every planted defect visible on a fixture.  No GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch
from scipy.sparse import coo_matrix
from scipy.sparse.csgraph import connected_components

import mimikit_amd as mmk
from mimikit_amd import native
from mimikit_amd.extract import clusters as CL
from tests import qcluster_refs as Q

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "mmk.h")
NAMES = ("mmk_nn_topk_workspace_bytes", "mmk_nn_topk_f32", "mmk_half_neg_sqnorm_f32", "mmk_edge_components_workspace_bytes",
         "mmk_edge_components_i64")

G = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "qcluster.npz"))
MIN_RATIO = 4.0


# ------------------------------------------------------------------------------------------------------------------- the interface
def test_package_exports():
    assert mmk.QCluster is CL.QCluster and "QCluster" in CL.__all__
    assert "qcluster.hip" in __import__("mimikit_amd.build", fromlist=["SOURCES"]).SOURCES
    q = mmk.QCluster()
    assert (q.cores_prop, q.n_neighbors, q.core_neighborhood_size, q.metric) == (.5, 8, 8, "euclidean")
    assert (q.K_, q.labels_, q.is_core_) == (None, None, None) and isinstance(q.inv, mmk.Identity)
    assert "distance exactly 0" in CL.__doc__ and "Synchronisations" in CL.__doc__ and "single core" in CL.__doc__
    with pytest.raises(NotImplementedError):
        q.np_func(np.zeros((20, 3), dtype=np.float32))
    with pytest.raises(RuntimeError):
        q.fit(torch.zeros(20, 3))
    with pytest.raises(TypeError):
        q.fit(np.zeros((20, 3), dtype=np.float32))
    with pytest.raises(NotImplementedError, match="manhattan"):
        mmk.QCluster(metric="manhattan").fit(torch.zeros(20, 3))


def test_prototypes_match_the_ctypes_signatures():
    text = open(HEADER).read()
    kinds = {"int64_t": C.c_int64, "int32_t": C.c_int32, "size_t": C.c_size_t, "float": C.c_float, "mmk_stream_t": C.c_void_p, "int": C.c_int32}
    for name in NAMES:
        found = re.search(rf"\b(int|size_t) {name}\(([^)]*)\);", text)
        assert found, name
        res, args = native._SIGNATURES[name]
        assert res is kinds[found.group(1)], name
        want = [C.c_void_p if "*" in arg else kinds[arg.strip().replace("const ", "").split()[0]] for arg in found.group(2).split(",")]
        assert want == list(args), (name, want, args)
    assert int(re.search(r"#define MMK_NN_TOPK_MAX (\d+)", text).group(1)) == native.NN_TOPK_MAX >= 16
    assert int(re.search(r"#define MMK_ABI_VERSION (\d+)", text).group(1)) == native.ABI_VERSION == 6
    lib = native.load_library()
    for rows, m, t in ((1, 1, 1), (129, 2 * Q.SPAN + 3, 9), (65536, 65536, 16)):
        assert lib.mmk_nn_topk_workspace_bytes(rows, m, t) == rows * -(-m // Q.SPAN) * t * 8       # spans x rows x T x 8, never rows x m
    assert lib.mmk_nn_topk_workspace_bytes(4, 4, native.NN_TOPK_MAX + 1) == 0
    for n in (1, 255, 256, 257, 100003):
        assert 12 * n < lib.mmk_edge_components_workspace_bytes(n) <= 12 * n + 4 * (n // 256 + 2), n


def test_entry_points_refuse_bad_sizes_before_any_launch():
    lib = native.load_library()
    buf = (C.c_double * 64)()
    p = C.addressof(buf)
    inf = float("inf")
    for rows, m, k, t in ((0, 4, 4, 1), (4, 0, 4, 1), (4, 4, 0, 1), (4, 4, 4, 0)):
        assert lib.mmk_nn_topk_f32(p, 4, p, rows, p, 4, p, p, -inf, inf, m, k, t, 0, p, p, p, 1 << 20, None) == -1, (rows, m, k, t)
    assert lib.mmk_nn_topk_f32(p, 4, p, 4, p, 4, p, p, -inf, inf, 4, 4, native.NN_TOPK_MAX + 1, 0, p, p, p, 1 << 20, None) == -3
    assert lib.mmk_nn_topk_f32(p, 4, p, 4, p, 4, p, p, 1.0, -1.0, 4, 4, 2, 0, p, p, p, 1 << 20, None) == -1      # limits the wrong way round
    assert lib.mmk_nn_topk_f32(p, 4, p, 4, p, 4, p, p, -inf, inf, 5, 4, 2, 1, p, p, p, 1 << 20, None) == -1      # self_exclude: m != rows
    assert lib.mmk_nn_topk_f32(p, 4, p, 4, p, 4, p, p, -inf, inf, 4, 4, 2, 0, p, p, p, 8, None) == -4            # workspace too small
    assert lib.mmk_half_neg_sqnorm_f32(p, 4, 0, 4, p, None) == -1
    assert lib.mmk_edge_components_i64(p, p, 0, 0, p, p, p, 4096, None) == -1
    assert lib.mmk_edge_components_i64(p, p, -1, 4, p, p, p, 4096, None) == -1
    assert lib.mmk_edge_components_i64(p, p, 0, 1 << 31, p, p, p, 1 << 40, None) == -3
    assert lib.mmk_edge_components_i64(p, p, 2, 8, p, p, p, 8, None) == -4


# ------------------------------------------------------------------------------------------------------------------- the restatement
@pytest.mark.parametrize("name", sorted(Q.FIXTURES))
def test_restatement_equals_the_reference_and_gaps_are_wide(name):
    seed, low, frames, metric, params = Q.FIXTURES[name]
    x = G[f"{name}_x"]
    assert x.dtype == np.float32 and np.array_equal(x, Q.fixture_frames(seed, low, frames)), "the fixture's input is not the seeded recipe"
    res = Q.fixture_result(name, x)
    assert np.array_equal(res["labels"], G[f"{name}_labels"]) and np.array_equal(res["is_core"], G[f"{name}_is_core"])
    assert res["K"] == int(G[f"{name}_K"]) == int(res["labels"].max()) + 1
    print(f"{name}: K_ {res['K']}, {int(res['is_core'].sum())} cores, n {res['n']}, k {res['k']}, smallest gap / bound {res['ratio']:.1f}")
    assert res["ratio"] >= MIN_RATIO, f"{name}: a gap of {res['ratio']:.2f} bounds"


def test_fixture_file_is_small_and_auto_case_takes_its_sizes_from_the_corpus():
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "qcluster.npz")
    assert os.path.getsize(path) < 100 * 1024
    res = Q.fixture_result("auto", G["auto_x"])
    assert (res["n"], res["k"]) == (12, 6) and G["auto_x"].shape[0] == 150
    assert max(max(r["n"], r["k"]) for r in (Q.fixture_result(n, G[f"{n}_x"]) for n in Q.FIXTURES)) <= Q.TOPK_MAX


@pytest.mark.parametrize("name", sorted(Q.edge_cases()))
def test_edge_components_equal_scipy(name):
    src, dst, n = Q.edge_cases()[name]
    labels, k = Q.edge_components64(src, dst, n)
    want_k, want = connected_components(coo_matrix((np.ones(src.shape[0]), (src, dst)), shape=(n, n)), directed=False)
    assert k == want_k and np.array_equal(labels, want), f"{name}: scipy numbers its components differently"
    first = np.full(k, n)
    np.minimum.at(first, labels, np.arange(n))
    assert (np.diff(first) > 0).all(), "not numbered by rising smallest member"


def test_edge_cases_are_what_they_say():
    cases = Q.edge_cases()
    assert Q.edge_components64(*cases["empty_5"])[1] == 5
    assert Q.edge_components64(*cases["self_loops_6"])[1] == 6
    assert Q.edge_components64(*cases["repeated_reversed_9"])[0].tolist() == [0, 1, 1, 2, 3, 4, 5, 6, 6]
    assert Q.edge_components64(*cases["path_4099_permuted"])[1] == 1 and Q.edge_components64(*cases["star_1000"])[1] == 1
    assert Q.edge_components64(*cases["two_cliques_one_bridge"])[1] == 3          # the two cliques as one, and nodes 45, 46
    assert 1 < Q.edge_components64(*cases["random_100003"])[1] < 100003


@pytest.mark.parametrize("metric", Q.METRICS)
def test_index_rule_takes_float64_and_sees_planted_faults(metric):
    x, key, bound = Q.self_case(50, 33, metric)
    order = Q.order64(key)
    for t in Q.TS:
        good = order[:, :t].copy()
        assert not Q.topk_rule_violations(good, key, bound, t).any()
        wrong = good.copy()
        wrong[:, 0] = np.arange(50)                                               # a row is its own nearest
        assert Q.topk_rule_violations(wrong, key, bound, t).all()
        far = good.copy()
        far[:, -1] = order[:, -1]                                                 # the farthest frame in the last slot
        assert Q.topk_rule_violations(far, key, bound, t).mean() > 0.9
    swapped = order[:, :9].copy()
    swapped[:, [2, 3]] = swapped[:, [3, 2]]
    assert Q.topk_rule_violations(swapped, key, bound, 9).mean() > 0.5
    x2, key2, bound2 = Q.self_case(3, 33, metric)                                 # two candidates: slots past them hold -1
    got = np.concatenate([Q.order64(key2)[:, :2], np.full((3, 7), -1)], -1)
    assert not Q.topk_rule_violations(got, key2, bound2, 9).any()
    got[1, 2] = 0
    assert Q.topk_rule_violations(got, key2, bound2, 9).tolist() == [False, True, False]


@pytest.mark.parametrize("metric", Q.METRICS)
def test_key_bound_holds_for_a_float32_evaluation(metric):
    """the kernel's roundings replayed in numpy float32 (a plain chain of multiply-adds, not fused: one more rounding per term, so this
    only shows the bound is of the right size, within a factor of two) - the device's own keys are held to it by the GPU test"""
    x, key, bound = Q.self_case(50, 64, metric)
    acc = np.zeros((50, 50), dtype=np.float32)
    for c in range(x.shape[1]):
        acc = (acc + (x[:, c, None] * x[None, :, c]).astype(np.float32)).astype(np.float32)
    if metric == "cosine":
        inv = (1.0 / np.sqrt((x.astype(np.float64) ** 2).sum(-1))).astype(np.float32)
        got = ((acc * inv[:, None]).astype(np.float32) * inv[None, :]).astype(np.float32)
    else:
        got = (acc + (-0.5 * (x.astype(np.float64) ** 2).sum(-1)).astype(np.float32)[None, :]).astype(np.float32)
    off = ~np.eye(50, dtype=bool)
    worst = float((np.abs(got.astype(np.float64) - key)[off] / bound[off]).max())
    print(f"{metric}: unfused float32 replay, worst error / bound {worst:.3f}")
    assert worst <= 2.0


@pytest.mark.parametrize("defect", Q.DEFECTS)
def test_every_defect_shows_on_a_fixture(defect):
    seen = []
    for name in sorted(Q.FIXTURES):
        res = Q.fixture_result(name, G[f"{name}_x"], defect)
        if not (np.array_equal(res["labels"], G[f"{name}_labels"]) and np.array_equal(res["is_core"], G[f"{name}_is_core"])):
            seen.append(name)
    print(f"{defect}: changes labels or cores of {seen}")
    assert seen, f"the defect {defect} changes no fixture"
