"""The table of tests/stream_cases.py against include/mmk.h, and its inputs against themselves: no GPU needed.

A new entry point with an mmk_stream_t parameter fails the completeness test until the table says whether it returns without waiting
for the stream; an entry point the table lists under WAITS fails the agreement test until the header's streams paragraph names it; and
a case whose stale input is the real one (or gives the reference the same outputs) would let every late-input test pass whatever the
kernel's stream."""
import pytest
import torch

from mimikit_amd import native
from tests import stream_cases as S


def test_every_stream_entry_point_is_under_exactly_one_rule():
    declared = S.header_stream_functions()
    assert len(declared) == len(set(declared)) and len(declared) > 70, len(declared)
    assert set(declared) <= set(native.EXPORTED_SYMBOLS)
    missing = sorted(set(declared) - set(S.ENTRY_POINTS))
    unknown = sorted(set(S.ENTRY_POINTS) - set(declared))
    assert not missing, f"in include/mmk.h with an mmk_stream_t parameter, but under none of ASYNC / WAITS / NOT_RUN: {missing}"
    assert not unknown, f"in the table, but not a function of include/mmk.h that takes an mmk_stream_t: {unknown}"
    lists = S.ASYNC + S.WAITS + S.NOT_RUN
    assert sorted(lists) == declared                                          # exactly one list each
    assert S.NOT_RUN == ("mmk_wavenet_profile_steps",)                        # the only one the issue allows beside the fault injectors


def test_one_name_less_is_noticed():
    """the parser and the comparison above, on a header with one more prototype than the table"""
    text = S.header_text().replace("#ifdef __cplusplus\n}", "int mmk_new_thing_f32(const float* x, /* a comment */ int64_t n,\n    mmk_stream_t stream);\n#ifdef __cplusplus\n}", 1)
    declared = S.header_stream_functions(text)
    assert set(declared) - set(S.ENTRY_POINTS) == {"mmk_new_thing_f32"}
    assert "mmk_abi_version" not in declared and "mmk_stft_n_frames" not in declared and "mmk_wavenet_plan_bind" not in declared


def test_the_header_names_every_waiting_entry_point():
    paragraph = S.header_streams_paragraph()
    for name in S.WAITS:
        assert name in paragraph, f"{name} waits for its stream ({S.ENTRY_POINTS[name].where}) but the header's streams paragraph does not name it"
    for name, e in S.ENTRY_POINTS.items():
        if e.unless:                                                          # the conditional waits are stated there too
            stem = name[:-len("_multi")] if name.endswith("_multi") else name
            assert stem in paragraph or ("spectral" in e.unless and "mmk_stft*_f32" in paragraph), name
    assert "never synchronises" not in paragraph


def test_every_stateless_entry_point_has_a_case():
    by_entry = {c.entry for c in S.CASES}
    for name, e in S.ENTRY_POINTS.items():
        assert (name in by_entry) == (e.how == S._CASE), name
    ids = [c.id for c in S.CASES]
    assert len(ids) == len(set(ids))
    for i in S.TWO_STREAM_CASES + S.NULL_STREAM_CASES:
        assert i in S.BY_ID
    for n_fft in S.SPECTRAL_N_FFT:                                            # the three kernel families, each entry point on each
        for stem in ("mmk_stft_mag_f32", "mmk_stft_f32", "mmk_stft_energy_f32", "mmk_stft_mel_f32", "mmk_istft_f32"):
            assert f"{stem}[{n_fft}]" in S.BY_ID


def test_the_smallest_shapes_are_the_ones_the_kernels_can_go_wrong_at():
    assert S.LFILTER_N == native.LFILTER1_CHUNK + 1                           # two chunks: the scan's second launch has something to carry
    assert (S.NOVELTY_T, S.NOVELTY_D, S.NOVELTY_HALVES) == (native.NOVELTY_TILE + 1, 33, (1, 6, native.NOVELTY_MAX_HALF))
    assert S.HPSS_SHAPE == (1, native.HPSS_TILE_FRAMES + 1, native.HPSS_TILE_BINS + 1)
    assert S.GEMM_K_SPLIT > 1 and S.SHORT_BLOCK < 2 * S.GRAPH_STEPS
    graph = [pc for pc in S.PLAN_CASES if pc.graph]
    assert len(graph) == 1 and graph[0].n == 2 * S.GRAPH_STEPS + 3


def test_every_plan_case_stands_on_a_case_of_the_refs_modules():
    for pc in S.PLAN_CASES + S.ERROR_WORD_CASES:
        assert S.plan_ref(pc) is not None, pc.id
    assert len({pc.id for pc in S.PLAN_CASES}) == len(S.PLAN_CASES)
    for network in ("wavenet", "srnn", "tr"):
        assert any(pc.sampled for pc in S.PLAN_CASES if pc.network == network), network


@pytest.mark.parametrize("case", S.CASES, ids=[c.id for c in S.CASES])
def test_the_stale_input_is_another_valid_input(case):
    """vacuity guard: the stale draw differs from the real one, has its shapes, dtypes and finite values, and - where the family's refs
    module restates the operation in float64 - gives that restatement other outputs"""
    real, stale = case.build(0), case.stale(0)
    assert real.keys() == stale.keys()
    assert any(not torch.equal(real[k], stale[k]) for k in real), f"{case.id}: the stale input is the real one"
    for k in real:
        assert real[k].shape == stale[k].shape and real[k].dtype == stale[k].dtype, (case.id, k)
        if stale[k].dtype.is_floating_point:
            assert bool(torch.isfinite(stale[k]).all()), (case.id, k)
        elif k in S.INT_BELOW:                                                # indices and classes stay valid ones
            assert 0 <= int(stale[k].min()) and int(stale[k].max()) < S.INT_BELOW[k], (case.id, k)
        else:
            assert k == "words", (case.id, k)                                 # (any 32-bit word is a word to fingerprint)
    again = case.build(0)
    assert all(torch.equal(real[k], again[k]) for k in real), f"{case.id}: build is not a function of its seed"
    if case.ref is not None:
        a, b = torch.as_tensor(case.ref(real)), torch.as_tensor(case.ref(stale))
        assert a.shape == b.shape and not torch.equal(a, b), f"{case.id}: the float64 restatement gives the stale input the real outputs"
