"""tests/caller_refs.py on the host: the timeline against numbers worked out by hand, the committed overrun and boundary cases against the
searches that found them, the conditions the device tests rely on (on the references alone), and the defects told apart by integers."""
import numpy as np
import pytest
import torch

from tests import caller_refs as cr
from tests.caller_refs import Ev, Slot


def _slots(C, base_sr, max_seconds, events):
    return cr.timeline(C, base_sr, max_seconds, events).slots


def test_timeline_against_hand_written_numbers():
    # 22050 -> 16000 reduces to 441 -> 320: 2205 samples -> 1600; 0.02 s = 320 steps -> 441 samples; 0.01 s = 160 -> 220.5 -> 221
    assert cr.ceil_ratio(2205, 16000, 22050) == 1600 and cr.ceil_ratio(320, 22050, 16000) == 441 and cr.ceil_ratio(160, 22050, 16000) == 221
    assert cr.ceil_ratio(2204, 16000, 22050) == 1600 and cr.ceil_ratio(2206, 16000, 22050) == 1601
    s = _slots(2205, 22050, 0.14, [Ev("class", 16000, 0.02), Ev("class", 16000, 0.01), Ev("class", 16000, 1.0)])
    assert s[0] == Slot(2205, True, 0, 1600, 1600, 320, 1600, 320, 441, 2205, 441, 2646)
    assert s[1] == Slot(2646, True, 441, 1600, 1600, 160, 1600, 160, 221, 2646, 221, 2867)
    assert s[2] == Slot(2867, False, 662, 0, 0, 0, 0, 0, 3087 - 2867, 2867, 3087 - 2867, 3087) and len(s) == 3
    # the same rate on both sides: nothing is resampled
    s = _slots(1600, 16000, 0.14, [Ev("class", 16000, 0.02)])
    assert s[0] == Slot(1600, True, 0, 1600, 1600, 320, 1600, 320, 320, 1600, 320, 1920)
    assert cr.timeline(1600, 16000, 0.14, [Ev("class", 16000, 0.02)]).exhausted          # one event does not fill 2240 samples


def test_streams_of_the_device_tests_by_hand():
    a = cr.STREAMS["a"].timeline()
    assert a.total == 5512 and not a.exhausted
    assert [(s.cursor, s.fits, s.P, s.n_steps, s.kept, s.piece_net, s.piece_base, s.written) for s in a.slots] == [
        (2205, True, 1600, 320, 1600, 320, 441, 441),
        (2646, True, 1600, 160, 1600, 160, 221, 221),
        (2867, True, 101, 16, 1600, 256, 353, 353),            # 1600 // 16 + 1 frames; 240 // 16 + 1 steps; 256 * 441 / 320 = 352.8
        (3220, True, 26, 13, 0, 768, 1059, 1059),              # 1600 // 64 + 1 frames; 800 // 64 + 1 frames out, 12 hops; 768 * 441 / 320 = 1058.4
        (4279, False, 0, 0, 0, 0, 1233, 1233)]
    # the NNN event's window [1015, 3220) spans the prompt's tail and all of events 0, 1 and 2; the Seq2Seq event's [662, 2867) two pieces
    assert a.slots[3].window == 3220 - 2205 == 1015 < a.slots[0].cursor and a.slots[2].window == 662 < a.slots[0].cursor
    b = cr.STREAMS["b"].timeline()
    assert b.total == 3307 and [(s.cursor, s.fits, s.written) for s in b.slots] == [(2205, True, 441), (2646, True, 221), (2867, False, 440)]
    c = cr.STREAMS["c"].timeline()
    # 0.01 s: 160 // 16 + 1 = 11 steps, 176 samples, 176 * 441 / 320 = 242.55 -> 243; int(0.1105 * 22050) = 2436 leaves 231
    assert c.total == 2436 and c.slots == (Slot(2205, True, 0, 1600, 101, 11, 1600, 176, 243, 2205, 231, 2448),)
    d = cr.STREAMS["d"].timeline()
    assert d.total == 2646 and [(s.cursor, s.fits, s.written) for s in d.slots] == [(2205, True, 221), (2426, False, 220)]
    e = cr.STREAMS["e"].timeline()
    assert e.total == 2240 and [(s.cursor, s.fits, s.T_net, s.piece_base) for s in e.slots] == [(1600, True, 1600, 320), (1920, True, 1600, 160), (2080, False, 0, 160)]
    for name, stream in cr.STREAMS.items():
        tl = stream.timeline()
        assert int(cr.silence_mask(tl).sum()) == tl.total - tl.C - sum(s.written for s in tl.slots if s.fits), name


def test_committed_overrun_and_boundary_cases_are_what_the_searches_find():
    assert cr.find_overrun() == cr.OVERRUN
    seconds, max_seconds = cr.OVERRUN
    s = _slots(cr.PROMPT, cr.BASE_SR, max_seconds, [Ev("framed", cr.NET_SR, seconds, cr.S2S_FFT, cr.S2S_HOP)])[0]
    assert s.fits and cr.PROMPT / cr.BASE_SR + seconds < max_seconds and s.piece_base > s.written == int(max_seconds * cr.BASE_SR) - cr.PROMPT > 0
    assert s.next_cursor > int(max_seconds * cr.BASE_SR)
    assert cr.find_boundary() == cr.BOUNDARY
    seconds, max_seconds = cr.BOUNDARY
    first, second = _slots(cr.PROMPT, cr.BASE_SR, max_seconds, [Ev("class", cr.NET_SR, seconds)] * 2)
    assert first.fits and not second.fits
    assert second.cursor / cr.BASE_SR + seconds == max_seconds                      # exactly: `>` instead of `>=` would run it
    assert second.written >= 1


def test_defects_are_told_apart_by_integers():
    shown = {d: [] for d in cr.DEFECTS}
    for name, stream in cr.STREAMS.items():
        tl = stream.timeline()
        for d in cr.DEFECTS:
            if cr.shows_in_clip(tl, d):
                shown[d].append(name)
        assert tuple(d for d in cr.DEFECTS if cr.shows_in_clip(tl, d)) == tuple(d for d in cr.DEFECTS if d in stream.defects), name
        assert all(cr.applies(tl, d) for d in stream.defects), name
    assert all(shown[d] for d in cr.DEFECTS if d != "cursor_written"), shown
    # the cursor advanced by what was written: one integer of the overrun stream, behind its last event - and no other stream's
    assert [n for n, s in cr.STREAMS.items() if cr.applies(s.timeline(), "cursor_written")] == ["c"]
    true, other = cr.STREAMS["c"].timeline().slots, cr.STREAMS["c"].timeline("cursor_written").slots
    assert other == (true[0]._replace(next_cursor=true[0].cursor + true[0].written),)


@pytest.mark.parametrize("name", ["a", "b", "c", "d"])
def test_few_float64_samples_of_the_first_window_lie_near_a_mulaw_edge(name):
    """the rule of caller_refs.mulaw_rule may excuse a code whose float64 sample lies within the resample bound of an edge: on the float64
    resampling of the prompt that is a fraction of a percent of the samples, so the rule cannot excuse a stage"""
    from mimikit_amd.features.functionals import resample_filter_bank
    from tests import f64_bounds as fb
    from tests.mulaw_refs import float64_codes
    orig, new, width, table = resample_filter_bank(cr.BASE_SR, cr.NET_SR)
    want64, bound = fb.resample_ref(cr.stream_prompt(name).double(), table.double(), orig, new, width)
    wrong, share = cr.mulaw_rule(float64_codes(want64, 256, 1.0), want64, bound, 256, 1.0)
    print(f"[callers f64] stream {name}: {share:.4%} of {want64.numel()} float64 samples within the resample bound of a mu-law edge")
    assert not bool(wrong.any()) and share <= cr.EDGE_SHARE_CAP


def test_float64_edges_are_where_the_float64_code_changes():
    from tests.mulaw_refs import float64_codes
    e = cr.float64_edges(256, 1.0)
    assert e.shape == (255,) and (np.diff(e) > 0).all()
    below, above = torch.from_numpy(e - 1e-9), torch.from_numpy(e + 1e-9)
    assert torch.equal(float64_codes(above, 256, 1.0), torch.arange(1, 256)) and torch.equal(float64_codes(below, 256, 1.0), torch.arange(0, 255))


def test_greedy_first_event_has_the_margin_check_picks_needs():
    """stream a's first event on the references alone: the fp32 oracle's own greedy run of the SampleRNN on the float64 codes of the
    resampled prompt passes net_refs.check_picks against its float64 envelope"""
    from mimikit_amd.features.functionals import resample_filter_bank
    from tests import f64_bounds as fb, net_refs as R
    from tests.mulaw_refs import float64_codes
    orig, new, width, table = resample_filter_bank(cr.BASE_SR, cr.NET_SR)
    want64, _ = fb.resample_ref(cr.stream_prompt("a").double(), table.double(), orig, new, width)
    codes = float64_codes(want64, 256, 1.0)
    slot = cr.STREAMS["a"].timeline().slots[0]
    case = cr.event_case("srnn")
    case.n, case.P, case.clips = slot.n_steps, slot.P, codes.shape[0]
    hist = R.free_run(case, codes)
    env = R.envelope(hist, case)
    tol_max, _ = R.tolerance(env.E[:, [case.n - 1]])
    R.check_picks(hist[:, case.P:], env.R64, tol_max, "stream a, event 0")


def test_nnn_prompt_fits_the_alignment_kernel():
    from mimikit_amd import native
    assert cr.STREAMS["a"].timeline().slots[3].P == 26 <= native.NNN_MAX_ROWS
