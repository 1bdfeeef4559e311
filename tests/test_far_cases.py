"""The table and the layouts of tests/far_cases.py against the headers and against themselves: no GPU needed.

A new `int64_t ..._stride` parameter fails the completeness test until the table says which far case drives it or why none does; a
layout whose far row falls short of its mark, whose operands meet, whose twin is in another alignment class or whose narrowed offsets
would land on the case's own rows (so that a wrong read returned data and a wrong write were overwritten) fails here, before any
kernel runs."""
import pytest
import torch

from mimikit_amd import native
from tests import far_cases as F
from tests import stream_cases as S


@pytest.fixture(scope="module")
def L():
    return native.lib()


def test_every_stride_parameter_is_under_exactly_one_of_far_and_not_far():
    declared = F.header_stride_params()
    assert len(declared) == len(set(declared)) and len(declared) > 100, len(declared)
    assert not set(F.FAR) & set(F.NOT_FAR), sorted(set(F.FAR) & set(F.NOT_FAR))
    missing = sorted(set(declared) - set(F.FAR_PARAMS))
    unknown = sorted(set(F.FAR_PARAMS) - set(declared))
    assert not missing, f"a stride or leading dimension of the headers under neither FAR nor NOT_FAR: {missing}"
    assert not unknown, f"in the table, but no int64_t stride parameter of the headers: {unknown}"
    for p, (rule, what) in F.FAR_PARAMS.items():
        if rule == "FAR":
            assert what in F.FAR_BY_ID or what == F.PLAN_TEST, (p, what)
        else:
            assert len(what.split()) >= 6 and what == what.strip(), (p, what)         # a reason, in a sentence
    for name in ("mmk_resample_f32.x_row_stride", "mmk_gemm_f32.a_batch", "mmk_tr_attention_f32.kv_cs", "mmk_categorical_sample_f32_i64.out_stride",
                 "mmk_gemm_bias_act_f32.group_stride", "mmk_srnn_warmup_multi.idx_row_stride", "mmk_wavenet_generate.cond_row_stride",
                 "mmk_pack_weight_f32.ldw", "mmk_wavenet_last_logits.ld", "mmk_tr_last_logits.out_ld", "mmk_spline2_coef_f64.coef_row_stride", "mmk_s2s_step_classes.x_elem_stride"):
        assert name in declared, name
    assert not any(p.endswith((".n", ".rows", ".t0", ".n_steps", ".numel", ".index", ".partial_floats")) for p in declared)


def test_one_name_more_is_noticed():
    """the parser and the comparison above, on a header with one more stride parameter than the table"""
    texts = F.header_texts()
    proto = "int mmk_lfilter1_f32(const float* x, int64_t x_row_stride,"
    assert proto in texts["mmk.h"]
    texts["mmk.h"] = texts["mmk.h"].replace(proto, "int mmk_lfilter1_f32(const float* x, /* new */ int64_t x_clip_stride, int64_t x_row_stride,", 1)
    assert set(F.header_stride_params(texts)) - set(F.FAR_PARAMS) == {"mmk_lfilter1_f32.x_clip_stride"}
    texts = F.header_texts()
    texts["mmk_nn_filter.h"] = texts["mmk_nn_filter.h"].replace("int64_t out_row_stride", "int64_t out_row_stride, const int64_t* w_ld", 1)
    assert set(F.header_stride_params(texts)) - set(F.FAR_PARAMS) == {"mmk_nn_aggregate_f32.w_ld"}


def test_every_far_case_covers_its_strided_operands_and_the_class_it_refuses_is_recorded():
    for c in F.FAR_CASES:
        assert c.params and all(p in F.header_stride_params() for p in c.params), c.id
        assert c.odd in ("runs", "refused")
    assert sorted(c.id for c in F.FAR_CASES if c.odd == "refused") == ["mmk_gemm_bias_act_f32", "mmk_gemm_bias_act_f32[row map]", "mmk_gemm_f32",
                                                                             "mmk_skinny_linear_f32"]
    for n_fft in S.SPECTRAL_N_FFT:                                            # the three kernel families
        for stem in F._STFT_STEMS:
            assert f"{stem}[{n_fft}]" in F.FAR_BY_ID


def _layout_conditions(c, lay):
    """-> list of what is wrong with one layout (empty: nothing)"""
    bad = []
    what = f"{c.id} {lay.id}"
    mark = F.MARKS[lay.mark]
    ivs = sorted(iv for p in lay.far for iv in p.intervals())
    for (a, b), (a2, b2) in zip(ivs, ivs[1:]):
        if a2 < b:
            bad.append(f"{what}: operands overlap at word {a2}")
    if ivs[0][0] < F.LEAD or ivs[-1][1] > F.CANVAS:
        bad.append(f"{what}: a row outside the field")
    tivs = sorted(iv for p in lay.twin for iv in p.intervals())
    if any(a2 < b for (a, b), (a2, b2) in zip(tivs, tivs[1:])) or tivs[0][0] < S.PAD or tivs[-1][1] > lay.twin_words - S.PAD:
        bad.append(f"{what}: the twin's rows overlap or leave its buffer")
    seen = {"bytes->uint32": False, "bytes->int32": False}
    for p, t in zip(lay.far, lay.twin):
        last_bytes = p.last_row_words() * F.WORD
        if lay.mark == "far":
            if last_bytes < 2 ** 32 or (p.ew == 1 and (p.far_count - 1) * p.far_stride < 2 ** 31):
                bad.append(f"{what} {p.name}: the last row begins {last_bytes} bytes from the base: short of the mark")
        elif not 2 ** 31 <= last_bytes < 2 ** 32:
            bad.append(f"{what} {p.name}: the last row begins {last_bytes} bytes from the base: not between 2^31 and 2^32")
        if p.last_row_words() < mark:
            bad.append(f"{what} {p.name}: short of the layout's mark")
        if (p.name, p.ew, p.levels, p.B, p.R, p.K, p.far_axis) != (t.name, t.ew, t.levels, t.B, t.R, t.K, t.far_axis):
            bad.append(f"{what} {p.name}: the twin has another shape")
        if (p.off * F.WORD) % 256 != (t.off * F.WORD) % 256 or p.s0 % 64 != t.s0 % 64 or p.s1 % 64 != t.s1 % 64:
            bad.append(f"{what} {p.name}: the twin is in another alignment class")
        if lay.cls == 0 and ((p.off * F.WORD) % 16 or p.s0 % 4 or p.s1 % 4):
            bad.append(f"{what} {p.name}: class 0 is 16-byte aligned with strides that are multiples of 4")
        if lay.cls == 1 and ((p.off * F.WORD) % 256 != p.ew * F.WORD or p.s1 % 2 == 0 or (p.levels == 2 and p.s0 % 2 == 0)):
            bad.append(f"{what} {p.name}: class 1 is one element in with odd strides")
        if t.far_stride * t.ew >= 2 ** 16:
            bad.append(f"{what} {p.name}: the twin is not near")
        for i in range(p.far_count):
            e = i * p.far_stride
            b = e * p.ew * F.WORD
            for name, w in (("bytes->uint32", b % 2 ** 32), ("bytes->int32", (b + 2 ** 31) % 2 ** 32 - 2 ** 31)):
                if w == b:
                    continue
                seen[name] = seen[name] or i == p.far_count - 1
                lo = p.off + w // F.WORD
                hi = lo + p.slot_words
                if lo < 0 or hi > F.CANVAS or any(a < hi and lo < b2 for a, b2 in ivs):
                    bad.append(f"{what} {p.name}: slot {i} under {name} lands on words [{lo}, {hi}): outside the canvas or on the case's own rows")
            if e % 2 ** 32 != e:
                bad.append(f"{what} {p.name}: an element offset beyond 2^32: the docstring's limit no longer holds, check elements->uint32 too")
    if not seen["bytes->int32"] or (lay.mark == "far" and not seen["bytes->uint32"]):
        bad.append(f"{what}: a narrowing of the last row's byte offset gives the true offset: the layout cannot see it ({seen})")
    return bad


@pytest.mark.parametrize("case", F.FAR_CASES, ids=[c.id for c in F.FAR_CASES])
def test_every_layout_reaches_its_mark_and_a_narrowed_offset_lands_on_fill(case, L):
    layouts = case.layouts(L)
    ids = [lay.id for lay in layouts]
    assert len(ids) == len(set(ids))
    two_level = any(levels == 2 for levels in case.ops.values())
    for axis in case.axes or (("rows", "batch") if two_level and any(p.B > 1 for p in layouts[0].far) else ("rows",)):
        for mark in ("far", "mid"):
            for cls in (0, 1):
                assert f"{axis}-{mark}-c{cls}" in ids, (case.id, axis, mark, cls)
    for lay in layouts:
        assert [p.name for p in lay.far] == list(case.ops)
        if lay.axis == "batch":
            assert all(p.far_axis == 0 for p in lay.far if p.levels == 2), (case.id, lay.id)        # each of the two strides is far in a layout
        else:
            assert all(p.far_axis == 1 for p in lay.far), (case.id, lay.id)
        bad = _layout_conditions(case, lay)
        assert not bad, bad[:5]
        assert not F.problems(lay.far, F.CANVAS)


def test_a_far_row_pulled_below_its_mark_is_noticed(L):
    """the conditions above, on layouts with one defect each"""
    case = F.FAR_BY_ID["mmk_cosine_cost_f32"]
    for lay in case.layouts(L):
        p = lay.far[0]
        axis = p.far_axis
        keep = (p.s0, p.s1, p.off)
        short = p.far_stride - (p.last_row_words() - F.MARKS[lay.mark]) // ((p.far_count - 1) * p.ew) - 64          # same class, just below
        p.s0, p.s1 = (short, p.s1) if axis == 0 else (p.s0, short)
        assert any("short of" in b or "not between" in b for b in _layout_conditions(case, lay)), lay.id
        p.s0, p.s1, p.off = keep
        p.off = lay.far[1].off                                                 # on top of another operand
        assert any("overlap" in b for b in _layout_conditions(case, lay)), lay.id
        p.s0, p.s1, p.off = keep
        lay.twin[0].off += 1                                                   # the twin one word further in
        assert any("alignment class" in b for b in _layout_conditions(case, lay)), lay.id
        lay.twin[0].off -= 1
        assert not _layout_conditions(case, lay)
    # without the skew a 32-bit byte offset of the last row of two lands on row 0 itself: a wrong read would return data
    lay = F.FAR_BY_ID["mmk_stft_mag_f32[1024]"].layouts(L)[0]
    assert (lay.axis, lay.mark, lay.cls, lay.far[0].far_count) == ("rows", "far", 0, 2)
    lay.far[0].s1 = 2 ** 31
    assert any("lands on" in b for b in _layout_conditions(F.FAR_BY_ID["mmk_stft_mag_f32[1024]"], lay))


@pytest.mark.parametrize("pc", F.PLAN_CASES, ids=[pc.id for pc in F.PLAN_CASES])
def test_every_plan_layout_meets_the_same_conditions(pc):
    ref = S.plan_ref(pc)
    assert ref.clips >= 2, pc.id
    tensors = F.plan_tensors(pc)
    assert "data" in tensors and (pc.network != "wavenet" or pc.ref != "chain-cond" or "cond0" in tensors)
    layouts = F.plan_layouts(pc)
    assert len(layouts) == (8 if 2 in F.plan_ops(pc).values() else 4)            # batch and frame / time strides: each far in a layout
    assert F.plan_ops(F.PLAN_CASES[-1]) == F.PLAN_OPS["tr frames"] and F.plan_ops(F.PLAN_CASES[-2]) == F.PLAN_OPS["tr"]
    for lay in layouts:
        assert [p.name for p in lay.far] == list(tensors)
        bad = _layout_conditions(pc, lay)
        assert not bad, bad[:5]
    assert F.plan_steps(F.PLAN_CASES[1]) >= 2 * S.GRAPH_STEPS > F.plan_steps(F.PLAN_CASES[0])      # a block above the graph threshold and one below
    assert {pc.network for pc in F.PLAN_CASES} == {"wavenet", "srnn", "s2s", "tr"}
    for network in ("wavenet", "srnn", "tr"):
        assert any(c.sampled for c in F.PLAN_CASES if c.network == network) and any(not c.sampled for c in F.PLAN_CASES if c.network == network)


def _fill_like(t):
    if t.dtype.is_floating_point:
        return torch.full_like(t, float("nan"))
    bits = F.NAN_BITS if t.element_size() == 4 else (F.NAN_BITS << 32 | F.NAN_BITS)
    return torch.full_like(t, bits)


@pytest.mark.parametrize("case", [c for c in F.FAR_CASES if c.bound or c.case.ref], ids=lambda c: c.id)
def test_the_reference_sees_the_strided_inputs(case):
    """a reference that ignored a strided input would pass a kernel that read fill instead of it"""
    real = case.build(0)
    strided = [k for k in case.ops if k in real]
    assert strided, case.id
    for k in strided:
        fill = {**real, k: _fill_like(real[k])}
        if case.bound:
            want, got = case.bound(real), case.bound(fill)
            assert any(not torch.equal(want[o][0], got[o][0]) for o in want), (case.id, k)
        else:
            # a stream case's reference takes one clip: the stacked inputs clip by clip
            clips = [{n: v[c:c + 1] if n in case.stack else v for n, v in pair.items()} for pair in (real, fill) for c in range(2)] if case.stack else [real, fill]
            refs = [torch.as_tensor(case.case.ref(i)) for i in clips]
            half = len(refs) // 2
            for a, b in zip(refs[:half], refs[half:]):
                assert a.shape == b.shape and not torch.equal(a, b), (case.id, k)


def test_the_s2s_spans_sit_on_either_side_of_the_limit():
    batch, hop, in_dim = 2, 8, 33
    for fs in (in_dim, in_dim + 7):
        spans = {w: F.s2s_span_bytes(batch, hop, in_dim, F.s2s_batch_stride(w, batch, hop, in_dim, fs), fs) for w in ("below", "above", "beyond")}
        assert F.S2S_SPAN_LIMIT - 16 * batch <= spans["below"] < F.S2S_SPAN_LIMIT <= spans["above"] < F.S2S_SPAN_LIMIT + 64 * batch, spans
        assert spans["beyond"] > 2 ** 32 and spans["beyond"] + 2 ** 20 < F.FIELD * F.WORD, spans
        assert all(F.s2s_batch_stride(w, batch, hop, in_dim, fs) % 4 == 0 for w in spans)
