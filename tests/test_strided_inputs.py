"""tests/strided_inputs.py without a GPU: the table against the headers and the test files, the helper's view, surround, mask() and
untouched() on host tensors, HUGE against every finite value, and the integer decoys."""
import ast
import itertools
import re
from pathlib import Path

import numpy as np
import pytest
import torch

from tests import far_cases as F
from tests import strided_inputs as SI
from tests.strided_inputs import DECOY, HUGE, NAN, ZERO, Strided

HERE = Path(__file__).resolve().parent


# ---------------------------------------------------------------------------------------------------------------------- the table
def test_table_and_headers_agree_in_both_directions():
    header, table = set(F.header_stride_params()), set(SI.SURROUND_PARAMS)
    assert not header - table, f"stride parameters without an entry: {sorted(header - table)}"
    assert not table - header, f"entries that no header declares: {sorted(table - header)}"
    assert set(SI.SURROUND_PARAMS) == set(F.FAR_PARAMS)
    for p, (kind, text) in SI.SURROUND_PARAMS.items():
        assert (kind == "RULE" and "::" in text) or (kind == "REASON" and text in SI.REASONS), (p, kind, text)


def reaches_the_rule(text, func):
    """does the module-level function `func` of the source `text` call, directly or through other functions of the module, a helper that is
    decorated with surround_rule and places an input with Strided.of, itself or in a function it calls"""
    defs = {n.name: n for n in ast.parse(text).body if isinstance(n, ast.FunctionDef)}
    names = lambda node: {n.id for n in ast.walk(node) if isinstance(n, ast.Name)} | {n.attr for n in ast.walk(node) if isinstance(n, ast.Attribute)}
    under = {name for name, d in defs.items() if any("surround_rule" in names(dec) for dec in d.decorator_list)}
    calls = {name: names(d) for name, d in defs.items()}

    def reach(start):
        seen, todo = set(), [start]
        while todo:
            name = todo.pop()
            if name in defs and name not in seen:
                seen.add(name)
                todo += sorted(calls[name] & set(defs))
        return seen
    return any({"Strided", "of"} <= calls[f] for helper in reach(func) & under for f in reach(helper))


def test_every_test_named_exists_and_reaches_a_helper_under_the_rule():
    for p, test in SI.UNDER_RULE.items():
        name, func = test.split("::")
        text = (HERE / name).read_text()
        assert re.search(rf"^def {func}\(", text, re.M), (p, test)
        assert reaches_the_rule(text, func), f"{p}: {test} calls no helper that is decorated with surround_rule and places an input"
    text = "def helper(x):\n    return Strided.of(x, 1, 'cpu')\n\n\ndef test_a():\n    helper(0)\n"
    assert not reaches_the_rule(text, "test_a") and reaches_the_rule(text.replace("def helper", "@surround_rule(ZERO)\ndef helper"), "test_a")
    for entry in SI.CONTIGUOUS_ONLY:
        assert not any(p.startswith(entry + ".") for p in SI.SURROUND_PARAMS), entry
    for name in SI.PLAN_TESTS:
        file, func = name.split("::")
        assert re.search(rf"^def {func}\(", (HERE / file).read_text(), re.M), name


def test_no_family_file_keeps_a_placement_class_of_its_own():
    for path in sorted(HERE.glob("test_gpu_*.py")):
        assert not re.search(r"^class (Rows|Clips)\b", path.read_text(), re.M), path.name


# ---------------------------------------------------------------------------------------------------------------------- the helper
LAYOUTS = [(shape, offset, pad, gap) for shape in ((1, 1), (3, 4), (2, 5), (2, 3, 4), (1, 2, 1))
           for offset in (0, 1, 2, 3) for pad in (0, 3, 4) for gap in (0, 6)]


def array(shape, dtype=np.float32):
    return (np.arange(1, 1 + int(np.prod(shape))).reshape(shape) * 0.5).astype(dtype)


def place(shape, offset, pad, gap, surround, dtype=np.float32, **kw):
    rows, k = shape[-2:]
    bs = dict(batch_stride=(rows - 1) * (k + pad) + k + gap) if len(shape) == 3 else {}
    return Strided.of(array(shape, dtype), offset, "cpu", row_stride=k + pad, surround=surround, **bs, **kw)


@pytest.mark.parametrize("surround", (ZERO, NAN, HUGE))
@pytest.mark.parametrize("dtype", (np.float32, np.float64))
def test_view_surround_mask_and_untouched(surround, dtype):
    for shape, offset, pad, gap in LAYOUTS:
        what = (shape, offset, pad, gap)
        s = place(shape, offset, pad, gap, surround, dtype)
        x = array(shape, dtype)
        assert np.array_equal(s.view.numpy(), x) and s.view.data_ptr() == s.ptr == s.buf.data_ptr() + offset * s.buf.element_size(), what
        assert tuple(s.view.stride()) == s.strides and s.strides[-2] == shape[-1] + pad, what
        mask = s.mask().numpy()
        assert mask.sum() == x.size and np.array_equal(s.buf.numpy()[mask], x.ravel()), what
        assert mask.size == offset + shape[0] * s.strides[0] + SI.TAIL and not mask[:offset].any() and not mask[-SI.TAIL:].any(), what
        outside, at = s.buf.numpy()[~mask], np.nonzero(~mask)[0]
        if surround == ZERO:
            assert not outside.any() and not np.signbit(outside).any(), what
        elif surround == NAN:
            bits = outside.view(np.uint32 if dtype == np.float32 else np.uint64)
            assert (bits == (SI.NAN_BITS if dtype == np.float32 else 0x7FF8000000000000)).all(), what
            assert np.array_equal(bits, torch.full((outside.size,), float("nan"), dtype=s.buf.dtype).numpy().view(bits.dtype)), what
        else:
            assert np.array_equal(outside, np.where(at % 2 == 0, 1, -1) * np.finfo(dtype).max), what
        # untouched(): true as placed; false after one element changes, inside or outside the view, by as little as its last bit
        # (another NaN payload, a subnormal for a zero); true again when the bits are back
        assert s.untouched(), what
        ints = SI._ints(s.buf)
        for j in {0, offset, mask.size - 1, int(np.nonzero(mask)[0][-1])}:
            kept = int(ints[j])
            ints[j] = kept ^ 1                        # the last bit
            assert not s.untouched(), (what, j)
            ints[j] = kept
            assert s.untouched(), (what, j)


def test_an_output_has_no_before_and_is_never_untouched():
    out = Strided((2, 3), 1, "cpu", float("nan"))
    assert not out.untouched() and bool(torch.isnan(out.buf).all()) and out.mask().sum() == 6


def test_the_defaults_are_the_families_layout():
    s = Strided.of(array((2, 3, 4)), 1, "cpu")
    assert (SI.PAD, SI.GAP, SI.TAIL) == (7, 11, 5) and s.strides == (3 * 11 + 11, 11, 1) and s.buf.numel() == 1 + 2 * 44 + 5
    assert (s.stride, s.clip, s.rows, s.k) == (11, 44, 3, 4) and s.surround == ZERO
    r = Strided.of(array((3, 4)), 2, "cpu")
    assert r.strides == (11, 1) and r.buf.numel() == 2 + 3 * 11 + 5


@pytest.mark.parametrize("dtype", (np.float32, np.float64))
def test_huge_wins_every_comparison_on_either_side(dtype):
    fin = np.finfo(dtype)
    values = np.array([0.0, -0.0, fin.tiny, -fin.tiny, 1.0, -1.0, 3.25, 1e30, -1e30, np.nextafter(fin.max, 0), -np.nextafter(fin.max, 0)], dtype)
    surround = SI.pattern(HUGE, 8, dtype)
    assert np.isfinite(surround).all() and (surround[::2] > values[:, None]).all() and (surround[1::2] < values[:, None]).all()
    assert surround[::2].min() >= values.max() and surround[1::2].max() <= values.min()
    # next to any window of in-view values a positive and a negative neighbour lie within two elements: max, min and median all move
    for window in itertools.combinations(values[4:9], 3):
        w = np.array(window, dtype)
        for extra in (surround[:1], surround[1:2], surround[:2]):
            both = np.concatenate([w, extra])
            assert both.max() != w.max() or both.min() != w.min()
        assert np.median(np.concatenate([w, surround[:1], surround[2:3]])) != np.median(w) or len(set(window)) < 3
    with np.errstate(over="ignore"):
        assert np.isinf(surround[0] + surround[2]) and np.isinf(np.float32(1) * surround[1] + surround[3])


# ---------------------------------------------------------------------------------------------------------------------- the decoys
DECOY_CASES = [  # (what, the in-view array, the valid range [lo, hi), offset, row stride or None)
    ("kmeans labels, k 3", np.array([[0, 2, 1, 1, 0, 2, 2]], np.int32), (0, 3), 4, 7),
    ("kmeans labels, k 1", np.zeros((1, 5), np.int32), (0, 1), 4, 5),
    ("kmeans labels, k 2", np.array([[0, 1, 1, 0]], np.int32), (0, 2), 4, 4),
    ("nn_aggregate lists, n 5", np.array([[1, 0], [0, 0], [4, 3], [2, 2], [-1, 1]], np.int64), (0, 5), 4, 2),
    ("pp_step candidates, n 129", np.array([[128, 0, 77]], np.int64), (0, 129), 4, 3),
    ("segment_mean order, n 6", np.array([[5, 0, 3, 1, 4, 2]], np.int64), (0, 6), 4, 6),
    ("cum_entropy items, strided rows", np.array([[3, 1003, 3], [-5, 0, -5]], np.int64), (-5, 1005), 1, None),
    ("classes, q_levels 256", np.array([[255, 0, 128], [7, 7, 7]], np.int64), (0, 256), 3, None),
]


@pytest.mark.parametrize("what,x,valid,offset,row_stride", DECOY_CASES, ids=[c[0] for c in DECOY_CASES])
def test_integer_decoys_are_in_range_and_differ_from_their_neighbours(what, x, valid, offset, row_stride):
    lo, hi = valid
    zero = Strided.of(x, offset, "cpu", row_stride=row_stride, decoy=valid, surround=ZERO)
    assert not zero.buf.numpy()[~zero.mask().numpy()].any() and zero.surround == ZERO
    for surround in (DECOY, NAN, HUGE):
        s = Strided.of(x, offset, "cpu", row_stride=row_stride, decoy=valid, surround=surround)
        buf, mask = s.buf.numpy(), s.mask().numpy()
        assert s.surround == DECOY and np.array_equal(s.view.numpy(), x) and s.buf.dtype == torch.from_numpy(x).dtype and s.untouched()
        assert ((buf[~mask] >= lo) & (buf[~mask] < hi)).all(), f"{what}: a decoy outside [{lo}, {hi})"
        assert (~mask).sum() >= offset + SI.TAIL
        if hi - lo > 2:
            for j in np.nonzero(~mask)[0]:
                for n in (j - 1, j + 1):
                    if 0 <= n < mask.size and mask[n]:
                        assert buf[j] != buf[n], f"{what}: the decoy at {j} equals the in-view value beside it"
        if hi - lo > 1:
            assert len(set(buf[~mask].tolist())) > 1, f"{what}: one decoy value only"


def test_monotone_decoys_for_offsets():
    offsets = np.array([[0, 2, 5, 5, 9]], np.int64)
    s = Strided.of(offsets, 4, "cpu", row_stride=5, decoy=SI.MONOTONE, surround=DECOY)
    buf = s.buf.numpy()
    assert (np.diff(buf) >= 0).all() and buf.min() == 0 and buf.max() == 9 and np.array_equal(s.view.numpy(), offsets)
    assert buf[:4].tolist() == [0] * 4 and buf[9:].tolist() == [9] * SI.TAIL


# ---------------------------------------------------------------------------------------------------------------------- the rule
def test_the_rule_passes_a_call_that_stays_inside_and_catches_one_that_does_not():
    x = array((3, 4))

    @SI.surround_rule(*SI.FLOAT_SURROUNDS)
    def inside(x_np):
        s = Strided.of(x_np, 1, "cpu")
        return s.view.sum(-1), dict(n=3, best=float(s.view.max()))

    @SI.surround_rule(*SI.FLOAT_SURROUNDS)
    def one_past_the_row_times_zero(x_np):
        s = Strided.of(x_np, 1, "cpu")
        wide = s.buf.as_strided((3, 5), (s.stride, 1), s.offset)
        return (wide * torch.tensor([1., 1., 1., 1., 0.])).sum(-1)

    @SI.surround_rule(*SI.FLOAT_SURROUNDS)
    def max_with_the_element_in_front(x_np):
        s = Strided.of(x_np, 1, "cpu")
        return torch.maximum(s.view[:, 0], s.buf[s.offset - 1])          # (a comparison: NaN in `other` propagates in torch, so test HUGE alone)

    @SI.surround_rule(*SI.FLOAT_SURROUNDS)
    def writes_its_surround(x_np):
        s = Strided.of(x_np, 1, "cpu")
        s.buf[0] = 5.0
        return s.view.sum()

    @SI.surround_rule(*SI.FLOAT_SURROUNDS)
    def places_nothing(x_np):
        return 0

    assert torch.equal(inside(x)[0], torch.from_numpy(x).sum(-1))
    with pytest.raises(AssertionError, match="under nan: .*a read outside a view"):
        one_past_the_row_times_zero(x)
    with pytest.raises(AssertionError, match="a read outside a view"):
        max_with_the_element_in_front(x)
    with pytest.raises(AssertionError, match="was written"):
        writes_its_surround(x)
    with pytest.raises(AssertionError, match="places no input"):
        places_nothing(x)
    assert SI._RUN is None


def test_bits_of_tells_a_negative_zero_and_a_nan_payload():
    a, b = torch.tensor([0.0, float("nan")]), torch.tensor([-0.0, float("nan")])
    assert SI.bits_of(a) != SI.bits_of(b) and SI.bits_of(a) == SI.bits_of(a.clone())
    assert SI.bits_of((a, None, 3, dict(k=a.numpy()))) == SI.bits_of([a.clone(), None, 3, dict(k=a.numpy().copy())])
    assert "1 elements differ, first at flat index 0" in SI.differing(SI.bits_of((a,)), SI.bits_of((b,)))
