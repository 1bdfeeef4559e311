"""mimikit_amd.extract.clusters without a GPU: the package exports, native mirrors the header's prototypes, the entry points refuse bad
sizes before any launch, the fixture recorded from the reference (tests/golden/clusters.npz) equals the float64 restatement of
tests/hcluster_refs.py, every fixture input keeps every level's smallest gap above four times the derived bound, `components64` equals
scipy's connected_components on the graph cases, every planted defect changes a result, and the host logic refuses as documented."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import mimikit_amd as mmk
from mimikit_amd import native
from mimikit_amd.extract import clusters as CL
from tests import hcluster_refs as H
from tests import neighbors_refs as NR

HERE = os.path.dirname(os.path.abspath(__file__))
HEADER = os.path.join(os.path.dirname(HERE), "include", "mmk.h")
G = np.load(os.path.join(HERE, "golden", "clusters.npz"))
NAMES = ("mmk_nn_cosine_self_f32", "mmk_nn_components_workspace_bytes", "mmk_nn_components_i64", "mmk_segment_mean_f32")
FIXTURES = ("a", "b", "c", "d")


@pytest.fixture(scope="module")
def restated():
    return {name: H.hcluster64(G[f"h_{name}_x"]) for name in FIXTURES}


# ------------------------------------------------------------------------------------------------------------------- the interface
def test_package_exports():
    for name in ("HCluster", "ArgMax"):
        assert getattr(mmk, name) is getattr(CL, name), name
    assert "hcluster.hip" in __import__("mimikit_amd.build", fromlist=["SOURCES"]).SOURCES
    h = mmk.HCluster()
    assert (h.max_iter, h.metric, h.K_, h.labels_) == (32, "cosine", None, None)
    assert isinstance(h.inv, mmk.Identity) and isinstance(mmk.ArgMax().inv, mmk.Identity)
    text = CL.__doc__
    assert "Da[Da == 0] = inf" in text and "fixed" in text and "N x N" in text


def test_prototypes_match_the_ctypes_signatures():
    text = open(HEADER).read()
    kinds = {"int64_t": C.c_int64, "int32_t": C.c_int32, "size_t": C.c_size_t, "float": C.c_float, "mmk_stream_t": C.c_void_p, "int": C.c_int32}
    for name in NAMES:
        found = re.search(rf"\b(int|size_t) {name}\(([^)]*)\);", text)
        assert found, name
        res, args = native._SIGNATURES[name]
        assert res is kinds[found.group(1)], name
        want = []
        for arg in found.group(2).split(","):
            arg = arg.strip()
            want.append(C.c_void_p if "*" in arg else kinds[arg.replace("const ", "").split()[0]])
        assert want == list(args), (name, want, args)
    assert "NaN in the inputs is not handled" in text[text.index("mmk_nn_cosine_self_f32:"):text.index("int mmk_nn_cosine_self_f32")]
    lib = native.load_library()
    for n in (1, 2, 255, 256, 257, 100003):
        assert 20 * n < lib.mmk_nn_components_workspace_bytes(n) <= 20 * n + 4 * (n // 256 + 1), n       # O(n), never O(n^2)
    assert lib.mmk_nn_components_workspace_bytes(0) == 0


def test_entry_points_refuse_bad_sizes_before_any_launch():
    lib = native.load_library()
    buf = (C.c_double * 64)()
    p = C.addressof(buf)
    for rows, k in ((1, 4), (0, 4), (2, 0)):
        assert lib.mmk_nn_cosine_self_f32(p, 4, p, rows, k, p, p, p, 4096, None) == -1, (rows, k)
    assert lib.mmk_nn_cosine_self_f32(p, 4, p, 4, 1, p, p, p, 8, None) == -4                 # workspace too small
    assert lib.mmk_nn_components_i64(p, 0, p, p, p, 4096, None) == -1
    assert lib.mmk_nn_components_i64(p, 1 << 31, p, p, p, 1 << 40, None) == -3
    assert lib.mmk_nn_components_i64(p, 8, p, p, p, 8, None) == -4
    for n, k, segments in ((0, 1, 1), (4, 0, 1), (4, 1, 0), (4, 1, 5)):                      # 5 segments of 4 rows: one would be empty
        assert lib.mmk_segment_mean_f32(p, 1, n, k, p, p, segments, p, 1, None) == -1, (n, k, segments)


def test_cpu_tensors_and_bad_arguments_raise():
    x = torch.rand(6, 5)
    for est in (mmk.HCluster(), mmk.ArgMax()):
        with pytest.raises(RuntimeError, match="MI355X"):
            est.fit(x)
        with pytest.raises(RuntimeError, match="MI355X"):
            est(x)
        with pytest.raises(TypeError):
            est.fit(x.double())
        with pytest.raises(ValueError):
            est.fit(x[0])
        with pytest.raises(ValueError):
            est.fit(torch.rand(2, 3, 4))
        with pytest.raises(NotImplementedError, match="device"):
            est(x.numpy())
    with pytest.raises(NotImplementedError, match="cosine"):
        mmk.HCluster(metric="euclidean").fit(x)
    with pytest.raises(RuntimeError, match="MI355X"):
        native.nn_cosine_self(x)
    with pytest.raises(RuntimeError, match="MI355X"):
        native.nn_components(torch.zeros(4, dtype=torch.int64))
    with pytest.raises(TypeError):
        native.nn_components(torch.zeros(4, dtype=torch.int32))
    with pytest.raises(RuntimeError, match="MI355X"):
        native.segment_mean(x, torch.zeros(6, dtype=torch.int64), torch.zeros(2, dtype=torch.int64))


@pytest.fixture
def host_kernels(monkeypatch):
    """the three kernels replaced by their float64 restatements, so that the Python layer's loop can be followed on the host"""
    monkeypatch.setattr(native, "require_device", lambda *t: None)

    def nn_cosine_self(x, inv_norm=None):
        c = H.cosine_others64(x.numpy())
        j = NR.argmax_first(c)
        return torch.from_numpy(j), torch.from_numpy(np.take_along_axis(c, j[:, None], -1)[:, 0].astype(np.float32))

    def nn_components(nearest):
        labels, k = H.components64(nearest.numpy())
        return torch.from_numpy(labels), torch.tensor(k)

    def segment_mean(x, order, offsets):
        x64, o, f = x.numpy().astype(np.float64), order.numpy(), offsets.numpy()
        return torch.from_numpy(np.stack([x64[o[a:b]].mean(0) for a, b in zip(f[:-1], f[1:])]).astype(np.float32))
    monkeypatch.setattr(native, "nn_cosine_self", nn_cosine_self)
    monkeypatch.setattr(native, "nn_components", nn_components)
    monkeypatch.setattr(native, "segment_mean", segment_mean)


def test_the_loop_of_fit_follows_the_reference(host_kernels):
    for name in FIXTURES + ("two",):
        h = mmk.HCluster(max_iter=2 if name == "two" else 32).fit(torch.from_numpy(G[f"h_{name}_x"].copy()))
        assert h.labels_.dtype == torch.int64 and np.array_equal(h.labels_.numpy(), G[f"h_{name}_labels"]), name
        assert (-1 if h.K_ is None else h.K_) == int(G[f"h_{name}_K"]) and (h.K_ is None or type(h.K_) is int)
    x = torch.from_numpy(G["h_two_x"].copy())
    h = mmk.HCluster(max_iter=0).fit(x)
    assert h.labels_.shape == (64, 0) and h.labels_.dtype == torch.int64 and h.K_ is None
    h = mmk.HCluster().fit(x[:1])
    assert h.labels_.shape == (1, 1) and int(h.labels_[0, 0]) == 0 and h.K_ == 1
    assert torch.equal(mmk.HCluster()(x), mmk.HCluster().fit(x).labels_)
    a = mmk.ArgMax().fit(x)
    assert np.array_equal(a.labels_.numpy(), G["argmax_labels"]) and a.K_ == int(G["argmax_K"]) and a.labels_.dtype == torch.int64


# ------------------------------------------------------------------------------------------------------------------- the fixture
@pytest.mark.parametrize("name", FIXTURES)
def test_restatement_equals_the_reference(restated, name):
    got = restated[name]
    assert np.array_equal(got["labels"], G[f"h_{name}_labels"]) and got["K"] == int(G[f"h_{name}_K"])
    assert [lv["k"] for lv in got["levels"]] == {"a": [6, 1], "b": [26, 6, 1], "c": [53, 7, 1], "d": [1]}[name]


def test_restatement_equals_the_reference_without_convergence():
    got = H.hcluster64(G["h_two_x"], max_iter=2)
    assert np.array_equal(got["labels"], G["h_two_labels"]) and got["K"] is None and int(G["h_two_K"]) == -1
    assert got["labels"].shape == (64, 2) and got["labels"][:, 1].max() + 1 == 4
    assert H.hcluster64(G["h_two_x"], max_iter=0)["labels"].shape == (64, 0)
    x = G["h_two_x"]
    assert np.array_equal(np.unique(x.argmax(1), return_inverse=True)[1], G["argmax_labels"]) and int(G["argmax_K"]) == len(np.unique(x.argmax(1)))


@pytest.mark.parametrize("name", FIXTURES + ("two",))
def test_fixture_inputs_keep_every_gap_above_four_bounds(restated, name):
    got = restated[name] if name in restated else H.hcluster64(G["h_two_x"], max_iter=2)
    worst = np.inf
    for i, lv in enumerate(got["levels"]):
        if lv["x"].shape[0] < 3:             # two rows: one candidate each, no second best
            assert np.isinf(lv["gap"]).all()
            continue
        ratio = (lv["gap"] / lv["bound"]).min()
        assert ratio >= 4, f"{name}, level {i}: smallest gap / bound {ratio:.2f}"
        assert i == 0 or (lv["err"] > 0).any()
        worst = min(worst, ratio)
    print(f"{name}: smallest gap / bound {worst:.1f}")


def test_level_bound_grows_with_the_level_and_stays_small(restated):
    lv = restated["c"]["levels"]
    assert (lv[0]["err"] == 0).all() and lv[1]["err"].max() < 4 * H.U * np.abs(lv[1]["x"]).max() and lv[2]["err"].max() < 8 * H.U * np.abs(lv[2]["x"]).max()
    assert (lv[2]["err"] / np.abs(lv[2]["x"])).min() > (lv[1]["err"] / np.abs(lv[1]["x"])).min() >= H.U
    plain = H.row_bound_others(H.level_bound(lv[1]["x"]))
    assert (lv[1]["bound"] > plain).all() and (lv[1]["bound"] < plain + 32 * H.U).all()


# ------------------------------------------------------------------------------------------------------------------- components
@pytest.mark.parametrize("name", sorted(H.graph_cases()))
def test_components64_is_scipy(name):
    csgraph = pytest.importorskip("scipy.sparse.csgraph")
    sparse = pytest.importorskip("scipy.sparse")
    nearest = H.graph_cases()[name]
    n = nearest.shape[0]
    adj = sparse.csr_matrix((np.ones(n, dtype=bool), (np.arange(n), nearest)), shape=(n, n))
    k, want = csgraph.connected_components(adj, directed=True, connection="weak")
    labels, got_k = H.components64(nearest)
    assert got_k == k and np.array_equal(labels, want), name


def test_graph_cases_are_what_they_say():
    g = H.graph_cases()
    assert H.components64(g["self_loop_1"]) [1] == 1 and H.components64(g["mutual_2"])[1] == 1
    assert H.components64(g["pairs_4098"])[1] == 2049 and H.components64(g["chain_4099"])[1] == 1 and H.components64(g["cycle_4099"])[1] == 1
    assert g["chain_4099"][0] == 1 and (g["chain_4099"][1:] == np.arange(4098)).all()
    labels, k = H.components64(g["cycle3_tails"])
    assert k == 2 and labels.tolist() == [0, 0, 0, 0, 0, 0, 1, 1]
    labels, k = H.components64(g["min_off_cycle"])
    assert k == 3 and labels.tolist() == [0, 1, 1, 2, 2, 0, 0]
    assert H.components64(g["star_1000"])[1] == 1
    k = H.components64(g["random_100003"])[1]
    assert 1 < k < 100 and (g["random_100003"] == np.arange(100003)).any()          # a handful of components, self-loops among the nodes


# ------------------------------------------------------------------------------------------------------------------- near misses
def changed(name, defect, **kw):
    x = G[f"h_{name}_x"]
    return not np.array_equal(H.hcluster64(x, defect=defect, **kw)["labels"], H.hcluster64(x, **kw)["labels"])


def test_rejects_self_as_the_nearest():
    assert all(changed(name, "self_allowed", max_iter=3) for name in FIXTURES)
    x, c, bound = H.self_case(50, 33)
    own = np.arange(50)
    assert NR.index_rule_violations(own, c, bound).all()


def test_rejects_the_last_index_among_ties():
    x, c, _ = H.big_self_case()
    first, last = NR.argmax_first(c), NR.argmax_first(c, "last_tie")
    assert first[H.ZERO_ROW] == 0 and last[H.ZERO_ROW] == x.shape[0] - 1
    for a, b in H.COPIES:
        assert np.array_equal(x[a], x[b]) and first[a] == b and first[b] == a
    zeros = np.zeros((5, 4), dtype=np.float32)
    assert NR.argmax_first(H.cosine_others64(zeros)).tolist() == [1, 0, 0, 0, 0]
    assert NR.argmax_first(H.cosine_others64(zeros), "last_tie").tolist() == [4, 4, 4, 4, 3]


def test_rejects_the_mean_of_the_original_frames():
    assert changed("b", "mean_of_frames") or changed("c", "mean_of_frames")
    # ... and where the labels happen to survive, the rows of the third level do not
    for name in ("b", "c"):
        x = G[f"h_{name}_x"]
        good, bad = H.hcluster64(x)["levels"], H.hcluster64(x, defect="mean_of_frames")["levels"]
        assert np.array_equal(good[1]["x"], bad[1]["x"])
        assert good[2]["x"].shape != bad[2]["x"].shape or np.abs(good[2]["x"] - bad[2]["x"]).max() > 1e3 * good[2]["err"].max()


def test_rejects_numbering_by_the_cycle():
    g = H.graph_cases()
    for name in ("min_off_cycle", "random_100003"):
        assert not np.array_equal(H.components64(g[name], "number_by_cycle")[0], H.components64(g[name])[0]), name
    assert H.components64(g["min_off_cycle"], "number_by_cycle")[0].tolist() == [2, 0, 0, 1, 1, 2, 2]


def test_rejects_a_column_that_is_not_composed():
    # (where the second level is the last, its column is all zeros composed or not: the inputs of three levels tell)
    assert all(changed(name, "no_relabel") for name in ("b", "c"))


def test_cases_of_the_kernels_are_well_posed():
    for rows in H.SELF_ROWS:
        for k in H.SELF_KS:
            x, c, bound = H.self_case(rows, k)
            assert x.shape == (rows, k) and np.isinf(np.diag(c)).all() and not NR.index_rule_violations(NR.argmax_first(c), c, bound).any()
            if k > 1 and rows > 3:
                assert np.mean(NR.gap64(c) <= 2 * bound) <= NR.GAP_CAP, (rows, k)
    x, c, bound = H.big_self_case()
    assert x.shape == H.BIG_SELF_CASE and np.mean(NR.gap64(c) <= 2 * bound) <= NR.GAP_CAP
    for k in H.MEAN_KS:
        x, order, offsets, want, mb = H.mean_case(k)
        assert np.diff(offsets).tolist() == list(H.MEAN_SEGMENTS) and sorted(order.tolist()) == list(range(x.shape[0]))
        got32 = np.stack([x[order[a:b]].astype(np.float64).mean(0) for a, b in zip(offsets[:-1], offsets[1:])]).astype(np.float32)
        assert not NR.outside(got32, want, mb).any()
        # a float32 running sum is outside it: the bound tells an fp64 accumulator from an fp32 one
        run32 = np.stack([np.add.accumulate(x[order[a:b]], 0, dtype=np.float32)[-1] / np.float32(b - a) for a, b in zip(offsets[:-1], offsets[1:])])
        assert NR.outside(run32, want, mb)[2].mean() > 0.5
