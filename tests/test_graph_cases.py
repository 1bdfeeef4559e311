"""The tables of tests/graph_cases.py against the seven headers under include/, against tests/stream_cases.py and against
mimikit_amd.features.functionals: no GPU needed.

A new prototype with an mmk_stream_t parameter, in any header, fails the completeness test until the table says whether a call can be
captured into a graph; an entry point that stream_cases (or the header) has waiting cannot be listed CAPTURED; a CAPTURED one without a
Case would never be replayed; and a new public Functional fails until FUNCTIONALS says how it is captured, or why not."""
import pytest
import torch

from mimikit_amd import native
from tests import graph_cases as G
from tests import stream_cases as S


def test_every_stream_entry_point_of_the_seven_headers_is_under_exactly_one_rule():
    declared = G.header_stream_functions()
    assert len(declared) == len(set(declared)) and len(declared) > 85, len(declared)
    assert set(S.header_stream_functions()) < set(declared)                   # mmk.h's, and the six family headers' on top
    missing = sorted(set(declared) - set(G.CAPTURE))
    unknown = sorted(set(G.CAPTURE) - set(declared))
    assert not missing, f"in a header under include/ with an mmk_stream_t parameter, but under neither CAPTURED nor NOT_CAPTURED: {missing}"
    assert not unknown, f"in the table, but not a function of a header under include/ that takes an mmk_stream_t: {unknown}"
    assert sorted(G.CAPTURED + G.NOT_CAPTURED) == declared                    # exactly one list each
    lib_names = set(native.EXPORTED_SYMBOLS) | set(native._SAMPLIFY_SIGNATURES) | set(native.SPEC_FILTER_SYMBOLS)
    assert set(S.header_stream_functions()) <= lib_names


def test_a_new_prototype_in_any_header_is_noticed():
    """the parser and the comparison above on doctored headers: one more prototype with a stream, in mmk.h and in a family's header"""
    texts = G.header_texts()
    for header in ("mmk.h", "mmk_samplify.h", "mmk_nmf.h"):
        doctored = dict(texts)
        assert "#ifdef __cplusplus\n}" in texts[header], header
        doctored[header] = texts[header].replace("#ifdef __cplusplus\n}", "int mmk_new_thing_f32(const float* x, /* a comment */ int64_t n,\n"
                                                 "    mmk_stream_t stream);\n#ifdef __cplusplus\n}", 1)
        declared = G.header_stream_functions(doctored)
        assert set(declared) - set(G.CAPTURE) == {"mmk_new_thing_f32"}, header
    doctored = dict(texts)                                                    # ... and a stream parameter added to a function that had none
    assert "size_t mmk_periods_workspace_bytes(int64_t n_samples);" in texts["mmk_samplify.h"]
    doctored["mmk_samplify.h"] = texts["mmk_samplify.h"].replace("size_t mmk_periods_workspace_bytes(int64_t n_samples);",
                                                                 "size_t mmk_periods_workspace_bytes(int64_t n_samples, mmk_stream_t stream);")
    assert set(G.header_stream_functions(doctored)) - set(G.CAPTURE) == {"mmk_periods_workspace_bytes"}
    plain = G.header_stream_functions()
    assert "mmk_abi_version" not in plain and "mmk_periods_workspace_bytes" not in plain and "mmk_fa_fit_workspace_bytes" not in plain


def test_the_table_contradicts_no_entry_of_stream_cases():
    stateless = {c.entry for c in S.CASES}
    for name, e in S.ENTRY_POINTS.items():
        rule = G.CAPTURE[name].rule
        if e.rule == "WAITS":
            assert rule == "NOT_CAPTURED", f"{name} waits for its stream ({e.where}) and is listed {rule}"
            assert e.where in G.CAPTURE[name].reason, name                    # the very line stream_cases quotes
        elif e.rule == "ASYNC" and name in stateless:
            assert rule == "CAPTURED", f"{name} is a stateless entry point that returns without waiting and is listed {rule}"
            assert bool(G.CAPTURE[name].unless) == bool(e.unless), f"{name}: the conditional wait is a precondition of the capture too"
        else:                                                                 # the plans' calls and the measurement aid
            assert rule == "NOT_CAPTURED", name
    # the families' own cases: the ones their files assert `busy` for are CAPTURED, the ones that wait are not
    waiting = {"mmk_nmf_start_f64", "mmk_nmf_solve_f64", "mmk_fa_fit_f64"}
    for case in G.all_cases():
        if case.entry not in S.ENTRY_POINTS:
            assert (G.CAPTURE[case.entry].rule == "NOT_CAPTURED") == (case.entry in waiting), case.id


def test_every_captured_name_has_a_case_and_every_other_a_reason():
    cases = G.captured_cases()
    by_entry = {c.entry for c in cases}
    for name in G.CAPTURED:
        assert name in by_entry, f"{name} is listed CAPTURED and no Case calls it"
    for name in G.NOT_CAPTURED:
        assert G.CAPTURE[name].reason and len(G.CAPTURE[name].reason) > 30, name
    ids = [c.id for c in G.all_cases()]
    assert len(ids) == len(set(ids)), "two cases share an id"
    assert all(G.CAPTURE[c.entry].rule == "NOT_CAPTURED" for c in G.all_cases() if c not in cases)
    for cid, companions in G.COMPANIONS.items():                              # what a case calls on the way is captured with it
        assert cid in ids
        for name in companions:
            assert G.CAPTURE[name].rule == "CAPTURED", (cid, name)
    # each Case keeps one definition: the families' are the objects of their own files
    from tests import test_gpu_kmeans, test_gpu_samplify
    assert all(any(c is d for d in G.all_cases()) for c in test_gpu_kmeans.STREAM_CASES + test_gpu_samplify.STREAM_CASES)


def test_the_header_states_the_capture_rule_and_names_the_table():
    paragraph = S.header_streams_paragraph()
    assert "tests/graph_cases.py" in paragraph and "tests/stream_cases.py" in paragraph
    listed = G.header_waiting_names(paragraph)
    assert len(listed) >= 17, listed
    for name in listed:
        assert G.CAPTURE[name].rule == "NOT_CAPTURED", f"the header lists {name} as waiting and the table has it CAPTURED"
    for name in S.WAITS:
        assert name in listed, name
    text = " ".join(paragraph.replace("*", " ").split())
    assert "cannot be captured into a graph" in text
    assert "plan" in text and "begin a capture of their own" in text, "the paragraph states why the plans' calls are not captured from outside"
    samplify = " ".join(G.header_texts()["mmk_samplify.h"].replace("*", " ").split())
    assert "each can be captured into a graph" in samplify                    # the promise tests/test_gpu_graphs.py holds the six to
    for name in ("mmk_spline2_coef_f64", "mmk_spline2_eval_f32", "mmk_periods_count_i64", "mmk_periods_fill_i64", "mmk_samplify_scores_f32",
                 "mmk_samplify_cuts_i64"):
        assert G.CAPTURE[name].rule == "CAPTURED", name
    for header, name in (("mmk_nmf.h", "mmk_nmf_start_f64"), ("mmk_nmf.h", "mmk_nmf_solve_f64"), ("mmk_factor_analysis.h", "mmk_fa_fit_f64")):
        own = " ".join(G.header_texts()[header].replace("*", " ").split())
        assert "captured into a graph" in own and G.CAPTURE[name].rule == "NOT_CAPTURED", name


@pytest.mark.parametrize("case", G.HALF_SWEEP_CASES, ids=[c.id for c in G.HALF_SWEEP_CASES])
def test_the_half_sweep_cases_have_another_valid_stale_input(case):
    """test_stream_cases.py's vacuity guard for the two cases that live here: the stale draw is another non-negative state of the same
    shapes, and the float64 restatement gives it other outputs"""
    real, stale, again = case.build(0), case.stale(0), case.build(0)
    assert real.keys() == stale.keys() and all(torch.equal(real[k], again[k]) for k in real)
    for k in real:
        assert real[k].shape == stale[k].shape and real[k].dtype == stale[k].dtype and not torch.equal(real[k], stale[k]), (case.id, k)
        assert bool(torch.isfinite(stale[k]).all()) and float(stale[k].min()) >= 0.0, (case.id, k)
    a, b = case.ref(real), case.ref(stale)
    assert a.shape == b.shape and not torch.equal(a, b)
    assert bool((real["w0"] == 0).any()) or bool((real["ht0"] == 0).any()), "the given state has exact zeros in it (nmf_refs.sweep_inputs)"


def test_the_chains_take_captured_entry_points_at_a_tile_edge():
    assert [c.id for c in G.CHAINS] == ["nnn", "novelty", "lloyd-step"]
    for chain in G.CHAINS:
        assert all(G.CAPTURE[e].rule == "CAPTURED" for e in chain.entries), chain.id
        first, second = chain.build(0), chain.build(1)
        assert first.keys() == second.keys()
        assert any(first[k].shape == second[k].shape and not (first[k] == second[k]).all() for k in first), chain.id
        assert all(first[k].shape == second[k].shape and first[k].dtype == second[k].dtype for k in first), chain.id
    from tests import kmeans_refs, nnn_refs, segment_refs
    x = G.CHAINS[0].build(0)
    assert x["x"].shape[1] in nnn_refs.NS and x["y"].shape[0] in nnn_refs.MS_COST and x["x"].shape[2] in nnn_refs.KS
    assert x["x"].shape[1] % native.NNN_ROW_PAD and x["y"].shape[0] == 65
    assert G.CHAINS[1].build(0)["x"].shape == (1, segment_refs.TILE + 1, 33)
    k = G.CHAINS[2].build(0)
    assert k["x"].shape[0] in kmeans_refs.NS and k["x"].shape[1] in kmeans_refs.DS and k["centres"].shape[0] in kmeans_refs.KS


def test_functionals_lists_exactly_the_public_functionals_and_the_named_functions():
    public = G.public_functionals()
    assert len(public) >= 29 and "Compose" in public and "Functional" in public
    missing = sorted(set(public) - set(G.FUNCTIONALS))
    assert not missing, f"public Functional classes of mimikit_amd.features.functionals under neither rule: {missing}"
    extra = sorted(set(G.FUNCTIONALS) - set(public))
    assert extra == sorted(["MelSpec.from_signal", "MFCC.from_signal", "PCA.transform", "mmk.discontinuity_scores", "extract.nearest_neighbor",
                            "extract.NeighborScorer.neighbors", "extract.cum_entropy"]), extra
    assert sorted(G.FUNCTIONALS_CAPTURED + G.FUNCTIONALS_NOT_CAPTURED) == sorted(G.FUNCTIONALS)
    for name in G.FUNCTIONALS_NOT_CAPTURED:
        rule, reason = G.FUNCTIONALS[name]
        assert rule == "NOT_CAPTURED" and "`" in reason and len(reason) > 30, f"{name}: the reason quotes the line"
    # what fits, reads a count or opens a file is not captured (the issue's rule); the rest is
    assert set(G.FUNCTIONALS_NOT_CAPTURED) == {"Functional", "FileToSignal", "PCA", "NMF", "FactorAnalysis", "extract.nearest_neighbor"}


def test_a_new_public_functional_is_noticed(monkeypatch):
    from mimikit_amd.features import functionals as F

    class Brand(F.Identity):
        pass
    monkeypatch.setattr(F, "Brand", Brand, raising=False)
    monkeypatch.setattr(F, "__all__", list(F.__all__) + ["Brand"])
    assert set(G.public_functionals()) - set(G.FUNCTIONALS) == {"Brand"}


@pytest.mark.parametrize("name", G.FUNCTIONALS_CAPTURED)
def test_the_second_draw_of_a_functional_case_is_another_input(name):
    fc = G.FUNCTIONALS[name]
    first, second, again = fc.draw(0), fc.draw(1), fc.draw(0)
    assert torch.equal(first, again), "draw is not a function of its seed"
    assert first.shape == second.shape and first.dtype == second.dtype and not torch.equal(first, second)
    assert first.dtype in (torch.float32, torch.int64) and (not first.dtype.is_floating_point or bool(torch.isfinite(second).all()))
