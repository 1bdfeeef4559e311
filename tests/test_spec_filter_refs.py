"""CPU checks of tests/spec_filter_refs.py and of the AutoConvolve / F0Filter interface: the recorded numpy / scipy results of
tests/golden/spec_filter.npz against the float64 restatements, inside the derived bounds; fields, defaults, serialisation and the refusals
raised on the host; the completeness of include/mmk_spec_filter.h (its names against native.SPEC_FILTER_SYMBOLS, its prototypes against the
ctypes signatures and the library's exports, its macros against native, a stream case per entry point); the entry points' refusals before
any launch.  No GPU."""
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
from tests import spec_filter_refs as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "mmk_spec_filter.h")
GOLDEN = os.path.join(ROOT, "tests", "golden", "spec_filter.npz")
G = np.load(GOLDEN)


# ------------------------------------------------------------------------------------------------------------------- the goldens
@pytest.mark.parametrize("name", sorted(R.F0_SHAPES))
def test_f0_restatement_lies_inside_the_bound_of_scipys_result(name):
    s = R.f0_fixture(name)
    _, n_frames, bins = R.F0_SHAPES[name]
    assert s.dtype == np.float32 and s.shape == (n_frames, bins) and float(s.astype(np.float64).sum()) == float(G[f"{name}_checksum"]), \
        "the frames are not the seeded recipe the golden was made from"
    assert not s[2].any() and s[3, :bins // 2].all() and not s[3, bins // 2:].any()
    for n_over, n_under in R.F0_RECORDED[name]:
        y_sp = G[f"y_{name}_{n_over}_{n_under}"]
        y, e_b = R.f0_parts64(s, n_over, n_under)
        worst_y = R.assert_inside(y, y_sp, e_b, f"{name} ({n_over}, {n_under}) y")
        gap = min(R.min_gap(y, e_b), R.min_gap(y_sp, e_b))
        assert gap >= R.MIN_GAP, f"{name} ({n_over}, {n_under}): smallest gap {gap:.2f} E_b"
        worst = 0.0
        for soft, normalize in R.MODES:
            out, bound = R.f0_filter64(s, n_over, n_under, soft, normalize)
            gold = R.f0_from_y(s, y_sp, soft, normalize)
            worst = max(worst, R.assert_inside(out, gold, bound, f"{name} ({n_over}, {n_under}) soft={soft} normalize={normalize}"))
            if not soft:
                assert np.array_equal(gold != 0, out != 0), "the hard masks differ"
        print(f"{name} ({n_over}, {n_under}): smallest gap {gap:.1f} E_b, scipy's y within {worst_y:.2f} E_b, outputs within {worst:.2f} of the bound")


def test_f0_definition_on_frames_worked_by_hand():
    s = np.array([[1, 2, 4, 8, 16, 32, 64]], dtype=np.float32)
    y, _ = R.f0_parts64(s, 3, 4)            # overtones h = 1, 2; undertones x = 2, 3
    sl = np.array([1 + 1, 2 + 4, 4 + 16, 8 + 64, 16, 32, 64], dtype=np.float64)
    half = np.array([1, 1.5, 2, 3, 4, 6, 8], dtype=np.float64)
    third = np.array([1, 1 + 1 / 3, 1 + 2 / 3, 2, 2 + 2 / 3, 2 + 4 / 3, 4], dtype=np.float64)
    assert np.allclose(y[0], sl - half - third, rtol=1e-15, atol=0)
    assert not R.f0_parts64(s, 1, 2)[0].any() and not R.f0_filter64(s, 1, 2, True, True)[0].any(), "n_overtone = 1 with n_undertone = 2 is all zeros"
    assert np.array_equal(R.f0_parts64(s, 0, 0)[0], R.f0_parts64(s, 1, 2)[0])
    edge = R.f0_parts64(np.array([[3, 5]], dtype=np.float32), 2, 3)[0]      # F = 2: lo + 1 is clamped to F - 1
    assert np.array_equal(edge[0], [3 - 3, 5 - 4])


@pytest.mark.parametrize("name", sorted(R.AC_SHAPES))
def test_auto_convolve_restatement_reproduces_numpys_rounded_values(name):
    s = R.ac_fixture(name)
    assert float(s.astype(np.float64).sum()) == float(G[f"{name}_checksum"])
    for k in R.AC_WINDOWS[name]:
        gold = G[f"ac_{name}_k{k}"]
        assert gold.dtype == np.float32 and gold.any() and not gold[2].any()
        n = R.ulp_rule(R.auto_convolve64(s, k).astype(np.float32), gold, f"{name} k={k}")
        assert np.array_equal(R.bits(R.auto_convolve_numpy(s, k).astype(np.float32)), R.bits(gold))
        print(f"{name} k={k}: {n} of {gold.size} float32 elements differ between the exact sum and numpy's order; {int(gold.any(axis=1).sum())} frames are not zero")


def test_auto_convolve_window_is_the_lopsided_one():
    s = np.array([[2.0], [3.0], [5.0], [7.0]], dtype=np.float32).repeat(2, axis=1)
    for k, want in ((2, [2, 6, 15, 35]), (3, [6, 30, 105, 35]), (4, [6, 30, 210, 105])):
        z = np.log(1.0 + np.array(want, dtype=np.float64))
        out = R.auto_convolve64(s, k)
        assert np.allclose(out[:, 0], z / (2 * z + 1e-8) * s[:, 0].astype(np.float64), rtol=1e-15), k
        assert np.allclose(R.auto_convolve_numpy(s, k), out, rtol=1e-14), k
    with pytest.raises(ValueError):
        R.auto_convolve_numpy(s, 1)              # the reference's own slice [:, :-0] is empty


def test_the_file_is_small_and_says_what_made_it():
    assert os.path.getsize(GOLDEN) < 1024 * 1024
    assert str(G["numpy_version"]) and str(G["scipy_version"])
    assert sorted(k for k in G.files if k.startswith("y_")) == sorted(f"y_{n}_{a}_{b}" for n, ps in R.F0_RECORDED.items() for a, b in ps)
    assert sorted(k for k in G.files if k.startswith("ac_")) == sorted(f"ac_{n}_k{k}" for n, ks in R.AC_WINDOWS.items() for k in ks)
    assert {v[1:] for v in R.F0_SHAPES.values()} == {(9, 1025), (33, 513), (6, 65), (5, 1026)} and set(R.F0_PARAMS) == {(4, 4), (8, 6), (2, 9), (16, 16)}
    assert {p for ps in R.F0_RECORDED.values() for p in ps} == set(R.F0_PARAMS)
    text = open(os.path.join(ROOT, "tests", "golden", "make_golden_spec_filter.py")).read()
    assert "librosa" in text and "import librosa" not in text and "mimikit." not in text.replace("mimikit_amd", "")


def test_b_div_x_by_multiplication_is_exact_where_the_kernel_uses_it():
    """csrc/spec_filter.hip: lo = (b * ceil(2^18 / x)) >> 18 for b <= 4096, 2 <= x <= 15, inside 32 bits"""
    b = np.arange(R.MAX_BINS, dtype=np.int64)
    for x in range(2, R.MAX_UNDERTONE):
        m = ((1 << 18) + x - 1) // x
        assert (b * m).max() < 2 ** 31 and np.array_equal((b * m) >> 18, b // x), x


# ------------------------------------------------------------------------------------------------------------------- the interface
def test_package_exports_fields_and_round_trip():
    assert mmk.AutoConvolve is F.AutoConvolve and mmk.F0Filter is F.F0Filter and {"AutoConvolve", "F0Filter"} <= set(F.__all__)
    build = __import__("mimikit_amd.build", fromlist=["SOURCES"])
    assert "spec_filter.hip" in build.SOURCES and any(h.endswith("mmk_spec_filter.h") for h in build.HEADERS)
    ac, f0 = mmk.AutoConvolve(), mmk.F0Filter()
    assert [f.name for f in dataclasses.fields(ac) if f.name != "type"] == ["window_size"] and ac.window_size == 3
    assert [f.name for f in dataclasses.fields(f0) if f.name != "type"] == ["n_overtone", "n_undertone", "soft", "normalize"]
    assert (f0.n_overtone, f0.n_undertone, f0.soft, f0.normalize) == (4, 4, True, True)
    for fn in (ac, f0):
        assert fn.unit is None and fn.elem_type is None and isinstance(fn.inv, mmk.Identity)
    other = mmk.F0Filter(n_overtone=8, n_undertone=6, soft=False, normalize=False)
    assert mmk.Config.deserialize(other.serialize()) == other
    assert mmk.Config.deserialize(mmk.AutoConvolve(5).serialize()) == mmk.AutoConvolve(5)
    chain = mmk.Compose(mmk.MagSpec(), mmk.F0Filter(), mmk.PCA(16), mmk.KMeans(8))
    assert mmk.Config.deserialize(chain.serialize()) == chain
    for cls, words in ((F.AutoConvolve, ("from memory", "float64", "log1p", "never crosses a clip", "returns float64")),
                       (F.F0Filter, ("from memory", "float64", "returns float64", "2-D input only", "in float32 before", "upper end"))):
        doc = " ".join(cls.__doc__.split())
        for word in words:
            assert word in doc, (cls.__name__, word)


def test_refusals_raised_on_the_host():
    x = torch.rand(40, 9)
    for fn, call in ((mmk.AutoConvolve(), native.auto_convolve), (mmk.F0Filter(), native.f0_filter)):
        with pytest.raises(RuntimeError, match="MI355X"):
            fn(x)
        with pytest.raises(RuntimeError, match="MI355X"):
            fn(x[None])
        with pytest.raises(NotImplementedError, match="device"):
            fn(x.numpy())
        with pytest.raises(NotImplementedError, match="device"):
            fn.np_func(x.numpy())
        with pytest.raises(TypeError):
            fn.torch_func(x.numpy())
        with pytest.raises(TypeError):
            fn(x.double())
        with pytest.raises(ValueError):
            fn(x[0])
        with pytest.raises(ValueError):
            fn(x[None, None])
        with pytest.raises(ValueError, match="2 bins"):
            fn(x[:, :1])
        with pytest.raises(ValueError):
            fn(x[:0])
        with pytest.raises(NotImplementedError, match=str(native.SPEC_FILTER_MAX_BINS)):
            call(torch.zeros(2, native.SPEC_FILTER_MAX_BINS + 1))
    for k in (1, 0, -3):
        with pytest.raises(ValueError, match="window_size"):
            mmk.AutoConvolve(k)(x)
    with pytest.raises(NotImplementedError, match=str(native.AUTO_CONVOLVE_MAX_WINDOW)):
        mmk.AutoConvolve(native.AUTO_CONVOLVE_MAX_WINDOW + 1)(x)
    with pytest.raises(NotImplementedError, match="F0_FILTER_MAX_OVERTONE"):
        mmk.F0Filter(n_overtone=native.F0_FILTER_MAX_OVERTONE + 1)(x)
    with pytest.raises(NotImplementedError, match="F0_FILTER_MAX_UNDERTONE"):
        mmk.F0Filter(n_undertone=native.F0_FILTER_MAX_UNDERTONE + 1)(x)
    with pytest.raises(ValueError, match="negative"):
        mmk.F0Filter(n_overtone=-1)(x)


# ------------------------------------------------------------------------------------------------------------------- the header
def header_prototypes():
    text = re.sub(r"/\*.*?\*/", " ", open(HEADER).read(), flags=re.S)
    return {m.group(2): (m.group(1), m.group(3)) for m in re.finditer(r"\b(int|size_t)\s+(mmk_[a-z0-9_]+)\s*\(([^;{}]*?)\)\s*;", text)}


def test_header_names_signatures_exports_and_macros():
    protos = header_prototypes()
    assert sorted(protos) == sorted(native.SPEC_FILTER_SYMBOLS) == ["mmk_auto_convolve_f32", "mmk_f0_filter_f32"]
    others = set(native.EXPORTED_SYMBOLS) | set(native.KMEANS_SYMBOLS) | set(native.NN_FILTER_SYMBOLS) | set(native.NMF_SYMBOLS) | set(native.SAMPLIFY_SYMBOLS)
    assert not set(native.SPEC_FILTER_SYMBOLS) & others
    kinds = {"int64_t": C.c_int64, "int32_t": C.c_int32, "size_t": C.c_size_t, "float": C.c_float, "mmk_stream_t": C.c_void_p, "int": C.c_int32}
    lib = native.load_library()
    for name, (res, args) in protos.items():
        want_res, want_args = native._SPEC_FILTER_SIGNATURES[name]
        assert want_res is kinds[res], name
        got = [C.c_void_p if "*" in a else kinds[a.strip().replace("const ", "").split()[0]] for a in args.split(",")]
        assert got == list(want_args), (name, got, want_args)
        fn = getattr(lib, name)
        assert fn is not None and fn.restype is want_res and list(fn.argtypes) == list(want_args), f"the library does not export {name}, or it is untyped"
        names = [a.replace("*", " ").split()[-1] for a in args.split(",")]
        assert names[:6] == ["s", "s_batch_stride", "s_row_stride", "batch", "frames", "bins"] and names[-4:] == ["out", "out_batch_stride", "out_row_stride", "stream"]
    text = open(HEADER).read()
    assert '#include "mmk.h"' in text and "must not overlap" in text and "64 bits" in text
    assert "MMK_ERR_INVALID:" in text and "MMK_ERR_UNSUPPORTED:" in text
    main = open(os.path.join(ROOT, "include", "mmk.h")).read()
    for word in ("auto_convolve", "f0_filter", "spec_filter"):
        assert word not in main, f"include/mmk.h names {word}"
    assert int(re.search(r"#define MMK_ABI_VERSION (\d+)", main).group(1)) == native.ABI_VERSION == 6
    for macro, value in (("MMK_SPEC_FILTER_MAX_BINS", native.SPEC_FILTER_MAX_BINS), ("MMK_SPEC_FILTER_TILE_FRAMES", native.SPEC_FILTER_TILE_FRAMES),
                         ("MMK_AUTO_CONVOLVE_MAX_WINDOW", native.AUTO_CONVOLVE_MAX_WINDOW), ("MMK_F0_FILTER_MAX_OVERTONE", native.F0_FILTER_MAX_OVERTONE),
                         ("MMK_F0_FILTER_MAX_UNDERTONE", native.F0_FILTER_MAX_UNDERTONE)):
        assert int(re.search(rf"#define {macro} (\d+)", text).group(1)) == value, macro
    assert (native.SPEC_FILTER_MAX_BINS, native.SPEC_FILTER_TILE_FRAMES, native.AUTO_CONVOLVE_MAX_WINDOW, native.F0_FILTER_MAX_OVERTONE,
            native.F0_FILTER_MAX_UNDERTONE) == (R.MAX_BINS, R.TILE_FRAMES, R.MAX_WINDOW, R.MAX_OVERTONE, R.MAX_UNDERTONE)
    assert native.SPEC_FILTER_MAX_BINS >= 2049 and min(native.AUTO_CONVOLVE_MAX_WINDOW, native.F0_FILTER_MAX_OVERTONE, native.F0_FILTER_MAX_UNDERTONE) >= 16


def test_every_stream_entry_point_has_a_stream_case():
    from tests import test_gpu_spec_filter as T
    with_stream = sorted(name for name, (_, args) in header_prototypes().items() if "mmk_stream_t" in args)
    assert with_stream == sorted(native.SPEC_FILTER_SYMBOLS)
    assert sorted({c.entry for c in T.STREAM_CASES}) == with_stream and sorted({c.case.entry for c in T.FAR_CASES}) == with_stream
    assert "returns without waiting" in open(HEADER).read()


def refusals(lib, p, q):
    """(entry point's name, call, code, a word of the text) for every refusal of the header; p, q: two aligned addresses"""
    ac = lambda s=p, sb=40, sr=8, batch=2, frames=5, bins=8, k=3, out=q, ob=40, orow=8: \
        lib.mmk_auto_convolve_f32(s, sb, sr, batch, frames, bins, k, out, ob, orow, None)
    f0 = lambda s=p, sb=40, sr=8, batch=2, frames=5, bins=8, no=4, nu=4, out=q, ob=40, orow=8: \
        lib.mmk_f0_filter_f32(s, sb, sr, batch, frames, bins, no, nu, 1, 1, out, ob, orow, None)
    rows = []
    for name, fn in (("auto_convolve", ac), ("f0_filter", f0)):
        rows += [(name, lambda fn=fn: fn(s=None), -1, "bad arguments"), (name, lambda fn=fn: fn(out=None), -1, "bad arguments"),
                 (name, lambda fn=fn: fn(batch=0), -1, "batch=0"), (name, lambda fn=fn: fn(frames=0), -1, "bad arguments"),
                 (name, lambda fn=fn: fn(bins=1, sr=1, orow=1, sb=5, ob=5), -1, "bins=1"), (name, lambda fn=fn: fn(bins=0), -1, "bad arguments"),
                 (name, lambda fn=fn: fn(sr=-1), -1, "row strides"), (name, lambda fn=fn: fn(orow=7), -1, "row strides"),
                 (name, lambda fn=fn: fn(sb=-1), -1, "batch strides"), (name, lambda fn=fn: fn(ob=7), -1, "batch strides"),
                 (name, lambda fn=fn: fn(s=p + 2), -1, "4-byte aligned"), (name, lambda fn=fn: fn(out=q + 2), -1, "4-byte aligned"),
                 (name, lambda fn=fn: fn(out=p), -1, "overlap"),
                 (name, lambda fn=fn: fn(bins=native.SPEC_FILTER_MAX_BINS + 1, sr=5000, orow=5000, sb=25000, ob=25000), -3, "MMK_SPEC_FILTER_MAX_BINS"),
                 (name, lambda fn=fn: fn(batch=2 ** 31 - 1, frames=2 ** 31 - 1), -3, "one launch")]
    rows += [("auto_convolve", lambda k=k: ac(k=k), -1, "window") for k in (1, 0, -2)]
    rows += [("auto_convolve", lambda: ac(k=native.AUTO_CONVOLVE_MAX_WINDOW + 1), -3, "MMK_AUTO_CONVOLVE_MAX_WINDOW"),
             ("f0_filter", lambda: f0(no=-1), -1, "negative"), ("f0_filter", lambda: f0(nu=-1), -1, "negative"),
             ("f0_filter", lambda: f0(no=native.F0_FILTER_MAX_OVERTONE + 1), -3, "MMK_F0_FILTER_MAX_OVERTONE"),
             ("f0_filter", lambda: f0(nu=native.F0_FILTER_MAX_UNDERTONE + 1), -3, "MMK_F0_FILTER_MAX_UNDERTONE")]
    return rows


def test_entry_points_refuse_bad_arguments_before_any_launch():
    lib = native.load_library()
    buf = (C.c_double * 256)()
    p = C.addressof(buf)
    for name, call, code, word in refusals(lib, p, p + 1024):
        assert call() == code, (name, word)
        text = lib.mmk_last_error().decode()
        assert name in text and word in text, (name, word, text)
