"""mimikit_amd.extract without a GPU: the package and its exports exist, native mirrors the header's constants and prototypes, the fixture
recorded from the reference (tests/golden/neighbors.npz) agrees with the float64 restatements of tests/neighbors_refs.py inside the derived
bounds, every case keeps the share of rows below the index rule's gap under its cap in float64 alone, the bounds are not vacuous (an fp32
restatement sits inside them) and reject seven near misses, and the host logic shapes, flattens and refuses as documented."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import mimikit_amd as mmk
from mimikit_amd import native
from mimikit_amd.extract import from_neighbors as FN
from tests import neighbors_refs as R

HERE = os.path.dirname(os.path.abspath(__file__))
HEADER = os.path.join(os.path.dirname(HERE), "include", "mmk.h")
G = np.load(os.path.join(HERE, "golden", "neighbors.npz"))
NAMES = ("mmk_nn_cosine_workspace_bytes", "mmk_nn_cosine_f32", "mmk_cum_entropy_i64")


# ------------------------------------------------------------------------------------------------------------------- the interface
def test_package_exports():
    for name in ("nearest_neighbor", "cum_entropy", "hist_transform", "NeighborScorer"):
        assert getattr(mmk, name) is getattr(FN, name), name
    assert "neighbors.hip" in __import__("mimikit_amd.build", fromlist=["SOURCES"]).SOURCES


def test_constants_mirror_the_header():
    text = open(HEADER).read()
    for name, value in (("MMK_NN_SPAN", native.NN_SPAN), ("MMK_CUM_ENTROPY_MAX_T", native.CUM_ENTROPY_MAX_T)):
        found = re.search(rf"#define {name} (\d+)", text)
        assert found and int(found.group(1)) == value, name
    assert "#define MMK_ABI_VERSION 6" in text and native.ABI_VERSION == 6


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
        assert name in native.EXPORTED_SYMBOLS
    lib = native.load_library()
    span = native.NN_SPAN
    for rows, m in ((1, 1), (67, 2 * span + 3), (82688, 131072), (5, span), (5, span + 1)):
        got = lib.mmk_nn_cosine_workspace_bytes(rows, m)
        assert 0 < got <= rows * -(-m // span) * 16 + 4096, (rows, m, got)
    assert lib.mmk_nn_cosine_workspace_bytes(0, 5) == 0


def test_entry_points_refuse_bad_sizes_before_any_launch():
    lib = native.load_library()
    buf = (C.c_double * 64)()
    p = C.addressof(buf)
    for rows, m, k in ((0, 1, 1), (1, 0, 1), (1, 1, 0)):
        assert lib.mmk_nn_cosine_f32(p, 1, p, rows, p, 1, p, m, k, p, p, p, 4096, None) == -1, (rows, m, k)
    assert lib.mmk_nn_cosine_f32(p, 1, p, 1, p, 1, p, (1 << 31), 1, p, p, p, 1 << 40, None) == -3
    assert lib.mmk_nn_cosine_f32(p, 1, p, 4, p, 1, p, 4, 1, p, p, p, 8, None) == -4          # workspace too small
    assert lib.mmk_cum_entropy_i64(p, 1, 0, 1, p, None, 0, None) == -1
    assert lib.mmk_cum_entropy_i64(p, 1, 1, 0, p, None, 0, None) == -1
    assert lib.mmk_cum_entropy_i64(p, 1, 1, native.CUM_ENTROPY_MAX_T + 1, p, None, 0, None) == -3
    assert b"MMK_CUM_ENTROPY_MAX_T" in lib.mmk_last_error()


# ------------------------------------------------------------------------------------------------------------------- host logic
def test_cpu_tensors_and_bad_arguments_raise():
    x, y = torch.rand(2, 5, 9), torch.rand(30, 9)
    with pytest.raises(RuntimeError, match="MI355X"):
        mmk.nearest_neighbor(x, y)
    with pytest.raises(RuntimeError, match="MI355X"):
        mmk.cum_entropy(torch.zeros(7, dtype=torch.int64), neg_diff=False)
    with pytest.raises(NotImplementedError, match="reference"):
        mmk.cum_entropy(torch.zeros(7, dtype=torch.int64), neg_diff=True)
    with pytest.raises(TypeError):
        mmk.cum_entropy(torch.zeros(7), neg_diff=False)
    with pytest.raises(ValueError):
        mmk.cum_entropy(torch.zeros(2, 3, 4, dtype=torch.int64))
    with pytest.raises(ValueError):
        mmk.cum_entropy(torch.zeros(2, 0, dtype=torch.int64))
    with pytest.raises(NotImplementedError, match=str(native.CUM_ENTROPY_MAX_T)):
        native.cum_entropy(torch.zeros(1, native.CUM_ENTROPY_MAX_T + 1, dtype=torch.int64))
    with pytest.raises(TypeError):
        mmk.NeighborScorer(y.double())
    with pytest.raises(ValueError):
        mmk.NeighborScorer(torch.rand(0, 9))
    with pytest.raises(ValueError):
        mmk.NeighborScorer(torch.rand(9))


@pytest.fixture
def host_kernels(monkeypatch):
    """the two kernels and the norms replaced by their float64 restatements, so that the Python layer's shapes can be followed on the host"""
    monkeypatch.setattr(native, "require_device", lambda *t: None)
    monkeypatch.setattr(native, "inv_row_norm", lambda x: torch.zeros(x.shape[:-1]))

    def nn_cosine(x, corpus, inv):
        assert x.dim() == 2 and corpus.dim() == 2 and inv.shape == (corpus.shape[0],)
        c = R.cosine64(x.numpy(), corpus.numpy())
        j = R.argmax_first(c)
        return torch.from_numpy(j), torch.from_numpy(np.take_along_axis(c, j[:, None], -1)[:, 0].astype(np.float32))

    def cum_entropy(items, per_step=False):
        assert items.dim() == 2 and items.dtype == torch.int64
        e = torch.from_numpy(np.stack([R.cum_entropy64(r) for r in items.numpy()]).astype(np.float32))
        return (e.sum(-1), e) if per_step else e.sum(-1)
    monkeypatch.setattr(native, "nn_cosine", nn_cosine)
    monkeypatch.setattr(native, "cum_entropy", cum_entropy)


def test_leading_dimensions_are_flattened_and_restored(host_kernels):
    x, y = torch.from_numpy(G["nn_nonneg_x"].copy()), torch.from_numpy(G["nn_nonneg_y"].copy())
    scorer = mmk.NeighborScorer(y)
    assert (scorer.n_frames, scorer.n_bins) == y.shape and scorer.corpus_has_negatives is False
    d2, n2 = scorer(x)
    assert d2.shape == n2.shape == (50,) and n2.dtype == torch.int64 and d2.dtype == torch.float32
    d3, n3 = scorer(x.reshape(5, 10, -1))
    d4, n4 = mmk.nearest_neighbor(x.reshape(5, 2, 5, -1), y)
    assert d3.shape == n3.shape == (5, 10) and d4.shape == n4.shape == (5, 2, 5)
    assert torch.equal(n3.reshape(-1), n2) and torch.equal(n4.reshape(-1), n2) and torch.equal(d3.reshape(-1), d2) and torch.equal(d4.reshape(-1), d2)
    assert np.array_equal(n2.numpy(), G["nn_nonneg_index"])
    with pytest.raises(ValueError, match="bins"):
        scorer(x[:, :-1])
    with pytest.raises(ValueError):
        scorer(x[0])
    with pytest.raises(TypeError):
        scorer(x.double())
    # one flag for the call: a single negative element in X halves every distance
    xs = x.clone()
    xs[3, 4] = -1e-3
    ds, _ = scorer(xs)
    assert float((ds[:3] / d2[:3]).max()) < 0.51
    e = scorer.entropy(x.reshape(5, 10, -1))
    assert e.shape == (5,)
    order, scores = scorer.k_bests(x.reshape(5, 10, -1), 3)
    assert order.shape == scores.shape == (3,) and torch.equal(order, torch.argsort(e, stable=True)[:3]) and torch.equal(scores, e[order])
    with pytest.raises(ValueError):
        scorer.k_bests(x.reshape(5, 10, -1), 6)


def test_cum_entropy_shapes(host_kernels):
    n = torch.from_numpy(G["ce_random_items"].copy())
    assert mmk.cum_entropy(n).shape == () and mmk.cum_entropy(n, reduce="none").shape == (40,)
    nb = torch.stack([n, n.flip(0), n])
    assert mmk.cum_entropy(nb).shape == (3,) and mmk.cum_entropy(nb, reduce=None).shape == (3, 40)
    assert torch.equal(mmk.cum_entropy(nb)[0], mmk.cum_entropy(n))


def test_hist_transform_is_the_reference():
    x = torch.from_numpy(G["hist_x"].copy())
    assert np.array_equal(mmk.hist_transform(x, bins=16).numpy(), G["hist_2d_16"])
    assert np.array_equal(mmk.hist_transform(x[0], bins=16).numpy(), G["hist_1d_16"])
    assert mmk.hist_transform(x.reshape(3, 1, 30)).shape == (3, 1, 256)


# ------------------------------------------------------------------------------------------------------------------- the fixture
@pytest.mark.parametrize("name", ("nonneg", "signed"))
def test_fixture_agrees_with_the_float64_restatement(name):
    x, y = G[f"nn_{name}_x"], G[f"nn_{name}_y"]
    dists, index, c = R.nearest64(x, y)
    bound = R.row_bound(x, y)
    nonneg = not R.has_negatives(x, y)
    assert nonneg == (name == "nonneg")
    assert not R.index_rule_violations(G[f"nn_{name}_index"], c, bound).any()
    assert R.below_gap_share(c, bound) <= R.GAP_CAP
    R.assert_inside(G[f"nn_{name}_dists"], dists, R.dist_bound(c.max(-1), bound, nonneg), f"the reference's distances, {name}")
    # the defect on record: the function as written returns the mean over the matrix and index 0
    assert G[f"nn_default_{name}_index"].shape == () and int(G[f"nn_default_{name}_index"]) == 0
    assert abs(float(G[f"nn_default_{name}_dist"]) - R.distance64(c, nonneg).mean()) < 1e-5


@pytest.mark.parametrize("rows,m,k", R.argmax_cases())
def test_cases_keep_the_share_of_rows_below_the_gap(rows, m, k):
    for signed in (False, True) if k > 1 and m > 1 else (False,):
        x, y, c, bound = R.nn_case(rows, m, k, signed)
        assert x.shape == (rows, k) and y.shape == (m, k) and R.has_negatives(x, y) == (signed or (k == 1 and m > 1))
        assert R.below_gap_share(c, bound) <= R.GAP_CAP, (rows, m, k, signed)
        assert not R.index_rule_violations(R.argmax_first(c), c, bound).any()


def test_many_blocks_case_keeps_the_share_of_rows_below_the_gap():
    rows, m, k = R.MANY_BLOCKS_CASE
    assert rows > 16 * 128 and rows % 128 and m > 2 * R.SPAN        # more query blocks than one group of workgroups, a ragged last block
    x, y, c, bound = R.nn_case(rows, m, k, True)
    assert R.below_gap_share(c, bound) <= R.GAP_CAP
    assert not R.index_rule_violations(R.argmax_first(c), c, bound).any()


def test_planted_case_is_well_posed():
    x, y, want = R.planted_case()
    c = R.cosine64(x, y)
    span = native.NN_SPAN
    assert np.array_equal(y[span + 5], y[7]) and np.array_equal(y[2 * span + 1], y[300]) and not R.has_negatives(x, y)
    assert np.array_equal(R.argmax_first(c), want)
    assert c[0, 7] == c[0, span + 5] and c[1, 300] == c[1, 2 * span + 1] and (c[2] == 0).all() and (c[:, 11] == 0).all()
    assert (R.gap64(c)[3:] > 2 * R.row_bound(x, y)[3:]).all()


def test_float32_restatement_sits_inside_the_bounds():
    """the kernel's arithmetic in numpy float32 (a sequential sum, not its order): the bounds hold and are not loose by orders of magnitude"""
    for rows, m, k, signed in ((50, 200, 33, False), (67, 200, 1025, True), (50, 200, 64, True)):
        x, y, c, bound = R.nn_case(rows, m, k, signed)

        def inv(a):
            s = np.sqrt((a * a).sum(-1, dtype=np.float32))
            return np.divide(np.float32(1), s, out=np.zeros_like(s), where=s > 0)
        c32 = np.clip((x @ y.T) * inv(x)[:, None] * inv(y)[None, :], -1, 1)
        assert c32.dtype == np.float32
        ratio = R.assert_inside(c32, c, R.cos_bound(x, y) + 1e-300, f"fp32 cosines {rows, m, k}")
        assert ratio > 1e-4
        j = np.argmax(c32, -1)
        assert not R.index_rule_violations(j, c, bound).any()
        nonneg = not R.has_negatives(x, y)
        d32 = (np.float32(1 + nonneg) * np.arccos(np.take_along_axis(c32, j[:, None], -1)[:, 0]) / np.float32(np.pi)).astype(np.float32)
        R.assert_inside(d32, R.distance64(c.max(-1), nonneg), R.dist_bound(c.max(-1), bound, nonneg), "fp32 distances")


# ------------------------------------------------------------------------------------------------------------------- near misses
def test_rejects_the_last_index_among_ties():
    x, y, want = R.planted_case()
    got = R.nearest64(x, y, "last_tie")[1]
    assert got[0] == native.NN_SPAN + 5 and got[1] == 2 * native.NN_SPAN + 1 and not np.array_equal(got, want)


def test_rejects_the_dot_product_without_the_corpus_norms():
    x, y, c, bound = R.nn_case(50, 200, 33)
    got = R.nearest64(x, y, "no_corpus_norm")[1]
    assert R.index_rule_violations(got, c, bound).mean() > 0.2


def test_rejects_abs_on_load():
    x, y, c, bound = R.nn_case(50, 200, 33, True)
    got = R.nearest64(x, y, "abs")[1]
    assert R.index_rule_violations(got, c, bound).mean() > 0.2


def test_rejects_the_nonneg_factor_per_row():
    x, y = G["nn_signed_x"].copy(), np.abs(G["nn_signed_y"])
    x[::2] = np.abs(x[::2])                       # every other query row is non-negative, the call is not
    want, _, c = R.nearest64(x, y)
    got = R.nearest64(x, y, "nonneg_per_row")[0]
    bad = R.outside(got, want, R.dist_bound(c.max(-1), R.row_bound(x, y), False))
    assert bad[::2].all() and not bad[1::2].any()


@pytest.mark.parametrize("defect", ("c/t", "log2", "final"))
def test_rejects_the_entropy_near_misses(defect):
    items, e64 = G["ce_random_items"], R.cum_entropy64(G["ce_random_items"])
    got = R.cum_entropy64(items, defect)
    assert R.outside(got, e64, R.entropy_bound(e64)).mean() > 0.5
    assert R.outside(got, G["ce_random_none"], R.ref_entropy_bound(items, e64)).mean() > 0.5
    assert abs(got.sum() - e64.sum()) > R.total_bound(e64) + R.ref_total_bound(items, e64)


# ------------------------------------------------------------------------------------------------------------------- cumulative entropy
def identity_entropy(items):
    """the kernel's formula, float64 numpy: occurrence ranks, f(r + 1) - f(r), one running sum"""
    def f(c):
        return c * np.log(c) if c > 0 else 0.0
    seen, S, e = {}, 0.0, []
    for s, v in enumerate(np.asarray(items).tolist()):
        r = seen.get(v, 0)
        seen[v] = r + 1
        S += f(r + 1.0) - f(float(r))
        e.append(0.0 if r == s else max(np.log(s + 1.0) - S / (s + 1.0), 0.0))       # (r == s: one item so far, a histogram of one bin)
    return np.array(e)


@pytest.mark.parametrize("name", ("random", "same", "distinct"))
def test_entropy_fixture_agrees_with_the_float64_restatement(name):
    items = G[f"ce_{name}_items"]
    e64 = R.cum_entropy64(items)
    R.assert_inside(G[f"ce_{name}_none"], e64, R.ref_entropy_bound(items, e64), f"the reference's e, {name}")
    assert abs(float(G[f"ce_{name}_sum"]) - e64.sum()) <= R.ref_total_bound(items, e64)
    R.assert_inside(identity_entropy(items), e64, R.entropy_bound(e64) - R.U * e64 + 1e-300, f"the identity, {name}")
    if name == "same":
        assert (G["ce_same_none"] == 0).all() and (identity_entropy(items) == 0).all()
    if name == "distinct":
        assert np.abs(e64 - np.log(np.arange(1, 41))).max() < 1e-14


@pytest.mark.parametrize("t", R.ENTROPY_TS)
def test_entropy_cases_and_the_identity(t):
    items, e64 = R.entropy_case(t)
    assert items.shape == (3, t) and (e64 >= 0).all() and e64[:, 0].max() == 0
    for r in range(3):
        R.assert_inside(identity_entropy(items[r]), e64[r], R.entropy_bound(e64[r]) - R.U * e64[r] + 1e-300, f"the identity, T = {t}, row {r}")
