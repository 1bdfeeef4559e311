"""CPU checks of tests/nn_filter_refs.py and of the NearestNeighborFilter interface: fields, defaults, serialisation and refusals; the
completeness of include/mmk_nn_filter.h (its names against native.NN_FILTER_SYMBOLS, its prototypes against the ctypes signatures and the
library's exports, its macros against native, a stream case per entry point that takes a stream); the restatement against the recorded
sklearn / numpy results of tests/golden/nn_filter.npz and the condition under which the device must reproduce them exactly; every planted
defect visible.  No GPU."""
import ctypes as C
import dataclasses
import os
import re

import numpy as np
import pytest
import torch

import mimikit_amd as mmk
from mimikit_amd import native
from mimikit_amd.features import functionals as F
from tests import nn_filter_refs as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "mmk_nn_filter.h")
GOLDEN = os.path.join(ROOT, "tests", "golden", "nn_filter.npz")
G = np.load(GOLDEN)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


# ------------------------------------------------------------------------------------------------------------------- the interface
def test_package_exports_fields_and_round_trip():
    assert mmk.NearestNeighborFilter is F.NearestNeighborFilter and "NearestNeighborFilter" in F.__all__
    build = __import__("mimikit_amd.build", fromlist=["SOURCES"])
    assert "nn_filter.hip" in build.SOURCES and any(h.endswith("mmk_nn_filter.h") for h in build.HEADERS)
    nf = mmk.NearestNeighborFilter()
    assert [f.name for f in dataclasses.fields(nf) if f.name != "type"] == ["n_neighbors", "metric", "aggregate"]
    assert (nf.n_neighbors, nf.metric, nf.aggregate) == (16, "cosine", "median") and nf.n_neighbors == native.NN_TOPK_MAX
    assert nf.unit is None and nf.elem_type is None and isinstance(nf.inv, mmk.Identity)
    other = mmk.NearestNeighborFilter(n_neighbors=5, metric="euclidean", aggregate="max")
    assert mmk.Config.deserialize(other.serialize()) == other
    chain = mmk.Compose(mmk.MagSpec(), mmk.NearestNeighborFilter(), mmk.PCA(16), mmk.KMeans(8))
    assert mmk.Config.deserialize(chain.serialize()) == chain
    assert native.NN_AGGREGATES == ("median", "mean", "max", "min")
    text = F.NearestNeighborFilter.__doc__
    for word in ("from\n    memory".split()[1], "the k nearest", "float64", "k | k + 1", "two frames are enough"):
        assert word in text, word


def test_cpu_tensors_numpy_and_bad_arguments_raise():
    x = torch.rand(40, 5)
    nf = mmk.NearestNeighborFilter()
    with pytest.raises(RuntimeError, match="MI355X"):
        nf(x)
    with pytest.raises(RuntimeError, match="MI355X"):
        nf(x[None])
    with pytest.raises(NotImplementedError, match="device"):
        nf(x.numpy())
    with pytest.raises(NotImplementedError, match="device"):
        nf.np_func(x.numpy())
    with pytest.raises(TypeError):
        nf.torch_func(x.numpy())
    with pytest.raises(TypeError):
        nf(x.double())
    with pytest.raises(ValueError):
        nf(x[0])
    with pytest.raises(ValueError, match="two frames"):
        nf(x[:1])
    with pytest.raises(ValueError, match="two frames"):
        nf(x[None, :1])
    with pytest.raises(ValueError, match="n_neighbors"):
        mmk.NearestNeighborFilter(n_neighbors=0)(x)
    with pytest.raises(NotImplementedError, match=f"limit of the HIP path is {native.NN_TOPK_MAX}"):
        mmk.NearestNeighborFilter(n_neighbors=native.NN_TOPK_MAX + 1)(x)
    with pytest.raises(NotImplementedError, match="manhattan"):
        mmk.NearestNeighborFilter(metric="manhattan")(x)
    with pytest.raises(ValueError, match="aggregate"):
        mmk.NearestNeighborFilter(aggregate="sum")(x)
    index = torch.zeros((40, 3), dtype=torch.int64)
    with pytest.raises(RuntimeError, match="MI355X"):
        native.nn_aggregate(x, index)
    with pytest.raises(TypeError):
        native.nn_aggregate(x.numpy(), index)
    with pytest.raises(TypeError):
        native.nn_aggregate(x.double(), index)
    with pytest.raises(ValueError):
        native.nn_aggregate(x[0], index)


# ------------------------------------------------------------------------------------------------------------------- the header
def header_prototypes():
    text = re.sub(r"/\*.*?\*/", " ", open(HEADER).read(), flags=re.S)
    return {m.group(2): (m.group(1), m.group(3)) for m in re.finditer(r"\b(int|size_t)\s+(mmk_[a-z0-9_]+)\s*\(([^;{}]*?)\)\s*;", text)}


def test_header_names_signatures_exports_and_macros():
    protos = header_prototypes()
    assert sorted(protos) == sorted(native.NN_FILTER_SYMBOLS) == ["mmk_nn_aggregate_f32"]
    assert not set(native.NN_FILTER_SYMBOLS) & (set(native.EXPORTED_SYMBOLS) | set(native.KMEANS_SYMBOLS))
    kinds = {"int64_t": C.c_int64, "int32_t": C.c_int32, "size_t": C.c_size_t, "float": C.c_float, "mmk_stream_t": C.c_void_p, "int": C.c_int32}
    lib = native.load_library()
    for name, (res, args) in protos.items():
        want_res, want_args = native._NN_FILTER_SIGNATURES[name]
        assert want_res is kinds[res], name
        got = [C.c_void_p if "*" in a else kinds[a.strip().replace("const ", "").split()[0]] for a in args.split(",")]
        assert got == list(want_args), (name, got, want_args)
        fn = getattr(lib, name)
        assert fn is not None and fn.restype is want_res and list(fn.argtypes) == list(want_args), f"the library does not export {name}, or it is untyped"
    text = open(HEADER).read()
    assert '#include "mmk.h"' in text and "must not alias" in text
    for path in ("mmk.h", "mmk_kmeans.h"):
        assert "nn_aggregate" not in open(os.path.join(ROOT, "include", path)).read(), f"include/{path} names the filter's entry point"
    for code, op in enumerate(native.NN_AGGREGATES):
        assert int(re.search(rf"#define MMK_NN_AGG_{op.upper()} (\d+)", text).group(1)) == code, op
    main = open(os.path.join(ROOT, "include", "mmk.h")).read()
    assert int(re.search(r"#define MMK_NN_TOPK_MAX (\d+)", main).group(1)) == native.NN_TOPK_MAX == mmk.NearestNeighborFilter().n_neighbors
    assert int(re.search(r"#define MMK_ABI_VERSION (\d+)", main).group(1)) == native.ABI_VERSION == 6


def test_every_stream_entry_point_has_a_stream_case():
    from tests import test_gpu_nn_filter as T
    with_stream = sorted(name for name, (_, args) in header_prototypes().items() if "mmk_stream_t" in args)
    assert with_stream == ["mmk_nn_aggregate_f32"]
    assert sorted({c.entry for c in T.STREAM_CASES}) == with_stream
    assert "returns without waiting" in open(HEADER).read()


def test_entry_point_refuses_bad_arguments_before_any_launch():
    lib = native.load_library()
    buf = (C.c_double * 64)()
    p = C.addressof(buf)
    q = p + 256
    for n, d, t in ((0, 4, 4), (4, 0, 4), (4, 4, 0)):
        assert lib.mmk_nn_aggregate_f32(p, 4, n, d, p, t, 1, 0, q, 4, None, None) == -1, (n, d, t)
    assert lib.mmk_nn_aggregate_f32(p, 4, 4, 4, p, native.NN_TOPK_MAX + 1, 1, 0, q, 4, None, None) == -3
    assert "MMK_NN_TOPK_MAX" in lib.mmk_last_error().decode()
    for op in (-1, 4, 99):
        assert lib.mmk_nn_aggregate_f32(p, 4, 4, 4, p, 4, 1, op, q, 4, None, None) == -3, op
    assert "MMK_NN_AGG" in lib.mmk_last_error().decode()
    assert lib.mmk_nn_aggregate_f32(None, 4, 4, 4, p, 4, 1, 0, q, 4, None, None) == -1                 # no x
    assert lib.mmk_nn_aggregate_f32(p, 4, 4, 4, None, 4, 1, 0, q, 4, None, None) == -1                 # no index
    assert lib.mmk_nn_aggregate_f32(p, 4, 4, 4, p, 4, 1, 0, None, 4, None, None) == -1                 # no out
    assert lib.mmk_nn_aggregate_f32(p, -1, 4, 4, p, 4, 1, 0, q, 4, None, None) == -1                   # negative stride
    assert lib.mmk_nn_aggregate_f32(p, 4, 4, 4, p, 4, 1, 0, q, 3, None, None) == -1                    # output rows overlap
    assert lib.mmk_nn_aggregate_f32(p + 2, 4, 4, 4, p, 4, 1, 0, q, 4, None, None) == -1                # x not 4-byte aligned
    assert lib.mmk_nn_aggregate_f32(p, 4, 4, 4, p + 4, 4, 1, 0, q, 4, None, None) == -1                # index not 8-byte aligned
    assert lib.mmk_nn_aggregate_f32(p, 4, 4, 4, p, 4, 1, 0, q, 4, p + 2, None) == -1                   # count not 4-byte aligned
    assert lib.mmk_nn_aggregate_f32(p, 4, 4, 4, p, 4, 1, 0, p, 4, None, None) == -1                    # out aliases x
    assert "alias" in lib.mmk_last_error().decode()


# ------------------------------------------------------------------------------------------------------------------- the restatement
@pytest.mark.parametrize("name", sorted(R.FIXTURES))
def test_restatement_reproduces_the_golden_and_exactness_is_a_fair_demand(name):
    n, d, k, metric, _, empty = R.FIXTURES[name]
    x = R.fixture_frames(name)
    assert x.dtype == np.float32 and x.shape == (n, d) and float(x.astype(np.float64).sum()) == float(G[f"{name}_checksum"]), \
        "the frames are not the seeded recipe the golden was made from"
    res = R.fixture_result(name, "median")
    assert res["ratio"] >= R.MIN_RATIO, f"{name}: ratio {res['ratio']:.2f}"
    counts = G[f"{name}_counts"]
    assert np.array_equal(res["counts"], counts) and int((counts == 0).sum()) == empty
    if n - 1 <= k:
        assert (counts == n - 1).all() and res["ratio"] == np.inf
    else:
        assert (counts == k).any() and ((counts > 0) & (counts % 2 == 0)).any() and (counts % 2 == 1).any()
    for op in ("median", "max"):
        got = R.fixture_result(name, op)["out"]
        assert got.dtype == np.float32 and np.array_equal(bits(got), bits(G[f"{name}_{op}"])), f"{name} {op}: not numpy's bits"
    mean = R.fixture_result(name, "mean")
    lists = R.mutual_lists64(mean["index"])
    abs_sum = np.stack([np.abs(x[nb].astype(np.float64)).sum(0) if nb.shape[0] else np.zeros(d) for nb in lists])
    bound = mean["bound"] + R.numpy_mean_bound(abs_sum, counts[:, None])
    err = np.abs(G[f"{name}_mean"].astype(np.float64) - mean["out"])
    worst = float((err / np.maximum(bound, 1e-300)).max())
    print(f"{name}: ratio {res['ratio']:.1f}, rows per count {np.bincount(counts).tolist()}; numpy's float32 mean against the float64 mean: worst "
          f"error / (bound + gamma(c)) {worst:.3f}")
    assert (err <= bound).all()


def test_the_file_is_small_and_says_what_made_it():
    assert os.path.getsize(GOLDEN) < 256 * 1024
    assert str(G["sklearn_version"]) and str(G["numpy_version"]) and str(G["scipy_version"])
    assert sorted(k for k in G.files if k.endswith("_counts")) == sorted(f"{name}_counts" for name in R.FIXTURES)
    assert {(v[0], v[1], v[2], v[3]) for v in R.FIXTURES.values()} == {(96, 33, 16, "cosine"), (96, 33, 16, "euclidean"), (40, 12, 4, "cosine"),
                                                                      (40, 12, 4, "euclidean"), (300, 33, 8, "euclidean"), (12, 7, 16, "cosine")}
    assert sorted(np.unique(G["cos96_counts"]).tolist()) == list(range(17)), "cos96 holds every count from 0 to 16"


@pytest.mark.parametrize("defect", R.DEFECTS)
def test_every_defect_is_noticed(defect):
    seen = []
    for name in sorted(R.FIXTURES):
        for op in R.GOLDEN_OPS:
            want = G[f"{name}_{op}"]
            got = R.fixture_result(name, op, defect)
            if op == "mean":
                clean = R.fixture_result(name, op)
                tol = np.abs(want.astype(np.float64) - clean["out"]).max() * 4 + 1e-12
                changed = bool((np.abs(got["out"] - want.astype(np.float64)) > tol).any())
            else:
                changed = not np.array_equal(bits(got["out"]), bits(want))
            if changed or not np.array_equal(got["counts"], G[f"{name}_counts"]):
                seen.append(f"{name} {op}")
    print(f"{defect}: changes {len(seen)} of {len(R.FIXTURES) * len(R.GOLDEN_OPS)} golden results: {seen[:6]}")
    assert seen, f"the defect {defect} changes no golden result"
    if defect in ("lower_median", "upper_median"):
        assert all(s.endswith("median") for s in seen)
    if defect == "mean_over_slots":
        assert all(s.endswith("mean") for s in seen)


# ------------------------------------------------------------------------------------------------------------------- the kernel cases
def test_kernel_cases_are_what_they_say():
    every = set()
    for n in R.NS:
        for d in R.DS:
            for t in R.TS:
                x, index = R.kernel_case(n, d, t)
                assert x.dtype == np.float32 and x.shape == (n, d) and index.shape == (n, t) and index.dtype == np.int64
                tiny = np.abs(x[x != 0]).min()
                assert 0 < tiny < 2.0 ** -126 and ((x < 0).any() or n * d < 10), "no subnormal or no negative value"
                for mutual in (True, False):
                    every |= set(R.nn_aggregate64(x, index, "max", mutual)[1].tolist())
    assert every == set(range(R.TOPK_MAX + 1)), f"the cases reach the counts {sorted(every)}"
    x, index = R.kernel_case(129, 65, 16)
    assert ((index < 0) | (index >= 129)).any() and (index == np.arange(129)[:, None]).any() and (index == 129).any() and (index > 2 ** 40).any()
    assert len(np.unique(x[:, 40])) <= 7, "values repeat across rows: the median meets ties"
    assert index[1, 0] == index[1, 1] == 0 and R.mutual_lists64(index)[1][:2].tolist() == [0, 0], "a row named by two slots counts twice"
    a, ca, _ = R.nn_aggregate64(x, index, "median", True)
    b, cb, _ = R.nn_aggregate64(x, index, "median", False)
    assert (ca <= cb).all() and (ca < cb).any() and not np.array_equal(bits(a), bits(b))
    for defect in ("self_included", "empty_slot_as_row0", "empty_row_zero", "lower_median", "upper_median"):
        c, cc, _ = R.nn_aggregate64(x, index, "median", True, defect)
        assert not (np.array_equal(bits(a), bits(c)) and np.array_equal(ca, cc)), f"{defect} does not show on the 129 x 65 x 16 kernel case"
    m, _, mb = R.nn_aggregate64(x, index, "mean", True)
    wrong, _, _ = R.nn_aggregate64(x, index, "mean", True, "mean_over_slots")
    assert (np.abs(wrong - m) > mb).any()
    f32 = np.stack([x[nb].mean(0) if nb.shape[0] else x[i] for i, nb in enumerate(R.mutual_lists64(index))])
    assert (np.abs(f32.astype(np.float64) - m) > mb).any(), "numpy's float32 running sum stays inside the float64 mean's bound: the bound is loose"
