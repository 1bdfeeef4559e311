"""A restatement of EnsembleGenerator's timeline, a re-walk of a finished clip and the per-stage checks of that re-walk, shared by
tests/test_caller_refs.py (CPU: the arithmetic alone) and tests/test_gpu_callers_f64.py (the device).  Nothing here imports the callers
under test (models/ensemble_generator.py, loops/generate_chunks.py, loops/generate.py) or their helpers convert / get_n_steps / fixed_length.

THE TIMELINE, from the reference's rules (mimikit/models/ensemble_generator.py:82-163, loops/generate.py get_n_steps, features/item_spec.py
convert), in plain integers, for framed features with center=True (Frame.padding set):

  total      = int(max_seconds * base_sr)
  an event at cursor t is run iff  t / base_sr + seconds < max_seconds  (floating point, as the reference writes it); otherwise it is
               still consumed, the rest of the clip stays silent and the run ends
  T_net      = ceil(C sr / base_sr), the ratio reduced by its gcd (torchaudio's resample)
  class net  : P = T_net,            n_steps = int(sr seconds),            kept = P,           piece = n_steps
  framed net : P = T_net // hop + 1, n_steps = int(sr seconds) // hop + 1, kept = (P - 1) hop, piece = n_steps hop
               (the inverse, Griffin-Lim, returns (frames - 1) hop samples of P + n_steps frames)
  NNN        : P as a framed net, n_frames = int(sr seconds) // hop + 1, nothing kept, piece = (n_frames - 1) hop
  base piece = ceil(piece base_sr / sr);  written = min(room, base piece);  the cursor advances by the whole base piece

Where the reference disagrees with the package (DESIGN.md records both):
  * a piece longer than the room left raises a shape error there (`output[:, t:t+n] = step_output`); the package clips it.  Only a framed
    event can get there: its piece is up to one hop longer than `seconds`, which is all the fit rule looks at;
  * the reference cannot run an NNN event at all (run_event reads net.config); the NNN row is the package's wiring;
  * with center=False (what IOSpec.magspec_io builds) P = (T_net - (n_fft - hop)) // hop and kept = P hop + n_fft - hop; not restated here.

DEFECTS are near misses of that arithmetic, one at a time, by name (DEFECTS below).  `cursor_written` moves one integer only - the cursor
after an overrunning event, and the run ends there either way - so no clip can show it: the CPU test tells it apart by that integer, the
device test records that the re-walk under it still reproduces the clip.

THE RE-WALK takes every event's window out of the FINAL clip (pieces are written once and never changed) and runs the public pieces in the
event's order: Resample, the input transforms one functional at a time, before_generate / generate_block / after_generate on a
blank-extended tensor, the target's inverse one functional at a time, Resample back, the cut.  It draws from torch's device generator in
the order the event does (the uniforms of a sampled block, then Griffin-Lim's initial phases) and records both draws.

THE STAGE CHECKS adapt what the kernels' own tests use; none has a tolerance of its own.
"""
import math
from types import SimpleNamespace as NS
from typing import NamedTuple, Optional, Tuple

import numpy as np
import torch
import torch.nn.functional as F

DEFECTS = ("kept", "window_early", "window_start", "write_late", "no_plus_one", "fit_gt", "cursor_written")
EDGE_SHARE_CAP = 0.01            # the share of a mu-law stage's samples the edge rule may excuse: a cap, not a tolerance
GLA_REL_L2 = 2e-3                # tests/test_gpu_features.py::test_griffin_lim_32_iterations, test_gpu_networks.py::test_seq2seq_loop_ends_in_griffin_lim


class Ev(NamedTuple):
    kind: str                    # "class" | "framed" | "nnn"
    sr: int
    seconds: float
    n_fft: Optional[int] = None
    hop: Optional[int] = None


class Slot(NamedTuple):
    cursor: int
    fits: bool
    window: int                  # where the event's input starts in the clip
    T_net: int
    P: int
    n_steps: int
    kept: int
    piece_net: int
    piece_base: int
    at: int                      # where the piece is written
    written: int
    next_cursor: int


class Timeline(NamedTuple):
    C: int
    base_sr: int
    max_seconds: float
    events: Tuple[Ev, ...]
    total: int
    slots: Tuple[Slot, ...]      # one per event the stream was asked for
    exhausted: bool              # the events ran out before the clip was full (the caller's next() raises StopIteration)


def ceil_ratio(n: int, num: int, den: int) -> int:
    g = math.gcd(num, den)
    return -(-n * (num // g) // (den // g))


def timeline(C: int, base_sr: int, max_seconds: float, events, defect: Optional[str] = None) -> Timeline:
    assert defect is None or defect in DEFECTS, defect
    events = tuple(Ev(*e) for e in events)
    total = int(max_seconds * base_sr)
    slots, cursor = [], C
    for ev in events:
        if cursor >= total:
            break
        start = cursor / base_sr + ev.seconds
        fits = not (start > max_seconds if defect == "fit_gt" else start >= max_seconds)
        if not fits:
            slots.append(Slot(cursor, False, cursor - C, 0, 0, 0, 0, 0, total - cursor, cursor, total - cursor, total))
            cursor = total
            continue
        T_net = ceil_ratio(C, ev.sr, base_sr)
        if ev.kind == "class":
            P, n_steps, unit = T_net, int(ev.sr * ev.seconds), 1
            kept, full = P, P + n_steps
        else:
            assert ev.kind in ("framed", "nnn"), ev.kind
            P, unit = T_net // ev.hop + 1, ev.hop
            n_steps = int(ev.sr * ev.seconds) // ev.hop + (0 if defect == "no_plus_one" else 1)
            kept, full = ((P - 1) * ev.hop, (P + n_steps - 1) * ev.hop) if ev.kind == "framed" else (0, (n_steps - 1) * ev.hop)
        if defect == "kept" and ev.kind != "nnn":
            kept += unit
        piece_net = full - kept
        piece_base = ceil_ratio(piece_net, base_sr, ev.sr)
        window = {"window_early": cursor - C - 1, "window_start": 0}.get(defect, cursor - C)
        at = cursor + (defect == "write_late")
        written = max(0, min(total - at, piece_base))
        nxt = cursor + (written if defect == "cursor_written" else piece_base)
        slots.append(Slot(cursor, True, window, T_net, P, n_steps, kept, piece_net, piece_base, at, written, nxt))
        cursor = nxt
    return Timeline(C, base_sr, max_seconds, events, total, tuple(slots), cursor < total)


def applies(tl: Timeline, defect: str) -> bool:
    """the defect changes at least one integer of this stream's timeline"""
    return timeline(tl.C, tl.base_sr, tl.max_seconds, tl.events, defect).slots != tl.slots


def shows_in_clip(tl: Timeline, defect: str) -> bool:
    """... and one that decides what is written where (the cursor behind the last event decides nothing)"""
    other = timeline(tl.C, tl.base_sr, tl.max_seconds, tl.events, defect).slots
    strip = lambda slots: [s._replace(next_cursor=0) for s in slots[-1:]]
    return other[:-1] != tl.slots[:-1] or strip(other) != strip(tl.slots)


def silence_mask(tl: Timeline) -> torch.Tensor:
    """(total,) bool: True where the timeline says nothing is ever written"""
    m = torch.ones(tl.total, dtype=torch.bool)
    m[:tl.C] = False
    for s in tl.slots:
        if s.fits:
            m[s.at:s.at + s.written] = False
    return m


# ---- the host searches whose results tests/test_caller_refs.py commits ------------------------------------------------------------------------------
def find_overrun(C=2205, base_sr=22050, sr=16000, n_fft=64, hop=16):
    """the first (seconds, max_seconds) of a small grid at which ONE framed event passes the fit rule and its piece exceeds the room"""
    for k in range(2, 9):
        seconds = k * 0.005
        for j in range(1, 40):
            max_seconds = round(C / base_sr + seconds + j * 0.0005, 4)
            s = timeline(C, base_sr, max_seconds, [Ev("framed", sr, seconds, n_fft, hop)]).slots[0]
            if s.fits and s.piece_base > s.written:
                return seconds, max_seconds
    return None


def find_boundary(C=2205, base_sr=22050, sr=16000):
    """the first seconds of a small grid at which, after one class event of that length, a second one starts with
    t / base_sr + seconds == max_seconds exactly in floating point - and would have had room to write"""
    for k in range(2, 9):
        seconds = k * 0.005
        t = C + ceil_ratio(int(sr * seconds), base_sr, sr)
        max_seconds = t / base_sr + seconds
        if int(max_seconds * base_sr) - t >= 1 and t / base_sr + seconds == max_seconds:
            return seconds, max_seconds
    return None


# ---- the re-walk --------------------------------------------------------------------------------------------------------------------------------------
class Player(NamedTuple):
    """an event as the re-walk needs it: its row of the timeline's input, the network (or NearestNextNeighbor) on the device, the temperature"""
    ev: Ev
    net: object
    temperature: Optional[float] = None


def _chain(f):
    """the functionals of a transform, one at a time"""
    return list(f.functionals) if hasattr(f, "functionals") else [f]


def _redraw(draw):
    """run `draw()` and return (its result, the device generator's state before it): the caller draws the same numbers again from there"""
    state = torch.cuda.get_rng_state()
    return draw(), state


def _again(state, shape, dtype, device):
    """what torch.rand drew from `state`, leaving the generator where it is now"""
    now = torch.cuda.get_rng_state()
    torch.cuda.set_rng_state(state)
    out = torch.rand(shape, dtype=dtype, device=device)
    torch.cuda.set_rng_state(now)
    return out


def _apply(stages, fn, x):
    name = type(fn).__name__
    if name == "GLA":
        y, state = _redraw(lambda: fn(x))
        stages.append(NS(name=name, fn=fn, x=x, y=y, init=_again(state, x.shape, torch.complex64, x.device)))
    else:
        y = fn(x)
        stages.append(NS(name=name, fn=fn, x=x, y=y))
    return y


def _event(player: Player, slot: Slot, window: torch.Tensor, base_sr: int):
    import mimikit_amd as mmk
    ev, net = player.ev, player.net
    stages = []
    at_net = _apply(stages, mmk.Resample(base_sr, ev.sr), window)
    assert at_net.shape[1] == slot.T_net, (at_net.shape, slot)
    rec = NS(ev=ev, slot=slot, stages=stages, window=window, temperature=player.temperature, uniforms=None, logits=None)
    if ev.kind == "nnn":
        prompt = _apply(stages, net.feature, at_net)
        assert prompt.shape[1] == slot.P, (prompt.shape, slot)
        rec.starts = net.predict_start_frames(prompt)
        frames = net.generate_block(prompt, slot.n_steps)
        rec.prompt, rec.history = prompt, frames
        audio = frames
        for fn in _chain(net.feature.inv):
            audio = _apply(stages, fn, audio)
    else:
        spec = net.config.io_spec
        prompts = []
        for f in spec.inputs:
            z = at_net
            for fn in _chain(f.transform):
                z = _apply(stages, fn, z)
            prompts.append(z)
        P, B = prompts[0].shape[1], prompts[0].shape[0]
        assert P == slot.P, (P, slot)
        data = tuple(torch.cat([p, p.new_zeros(B, slot.n_steps, *p.shape[2:])], 1) for p in prompts)
        net.before_generate(tuple(prompts), None)
        params = {} if player.temperature is None else {"temperature": player.temperature}
        ok, state = _redraw(lambda: net.generate_block(data, P, slot.n_steps, **params))
        assert ok, "the network declined generate_block"
        if player.temperature is not None:
            rec.uniforms = _again(state, (B, slot.n_steps), torch.float32, data[0].device)
        if ev.kind == "class":
            rec.logits = net._plan.last_logits(B)
        net.after_generate(data, None)
        rec.prompt, rec.history = prompts[0], data[0]
        audio = data[0]
        for fn in _chain(spec.targets[0].transform.inv):
            audio = _apply(stages, fn, audio)
    assert audio.shape[1] == slot.kept + slot.piece_net, (audio.shape, slot)
    rec.piece = _apply(stages, mmk.Resample(ev.sr, base_sr), audio[:, slot.kept:])
    assert rec.piece.shape[1] == slot.piece_base, (rec.piece.shape, slot)
    return rec


def rewalk(clip: torch.Tensor, prompt_len: int, players, tl: Timeline, seed: int, defect: Optional[str] = None):
    """-> (the clip as the re-walk writes it, one record per slot: None for an event that does not fit).  `tl`: the true timeline; with a
    defect the re-walk follows the defective timeline's integers instead.  Networks on the device, in eval mode."""
    assert prompt_len == tl.C and clip.shape[1] == tl.total
    t = tl if defect is None else timeline(tl.C, tl.base_sr, tl.max_seconds, tl.events, defect)
    out = torch.zeros_like(clip)
    out[:, :tl.C] = clip[:, :tl.C]
    records = []
    torch.manual_seed(seed)
    with torch.no_grad():
        for player, slot in zip(players, t.slots):
            if not slot.fits:
                records.append(None)
                continue
            window = clip[:, max(slot.window, 0):slot.window + tl.C]
            if slot.window < 0:
                window = F.pad(window, (-slot.window, 0))            # (in front of the clip: silence)
            rec = _event(player, slot, window, tl.base_sr)
            out[:, slot.at:slot.at + slot.written] = rec.piece[:, :slot.written]
            records.append(rec)
    return out, records


# ---- the stage checks -----------------------------------------------------------------------------------------------------------------------------------
def float64_edges(q: int, c: float) -> np.ndarray:
    """where the float64 formula's code changes: code >= k from ((y + 1) / 2 mu + 0.5) = k on, k = 1 .. q - 1, inverted in float64"""
    mu = q - 1.0
    y = 2.0 * (np.arange(1, q, dtype=np.float64) - 0.5) / mu - 1.0
    return np.sign(y) * np.expm1(np.abs(y) * np.log1p(mu * c)) / (mu * c)


def mulaw_rule(codes: torch.Tensor, want64: torch.Tensor, bound: torch.Tensor, q: int, c: float):
    """the per-element rule: a code equals the float64 formula's code of the float64 sample, or that sample lies within `bound` (the bound of
    the stage that made it) of a bin edge - plus two places of the fp32 number line there, the neighbourhood in which the fp32 contract
    itself differs from float64 (tests/mulaw_refs.py).  -> (wrong (bool), ambiguous share)"""
    from tests.mulaw_refs import float64_codes
    edges = float64_edges(q, c)
    w = want64.double().numpy()
    i = np.clip(np.searchsorted(edges, w), 1, len(edges) - 1)
    near = np.where(np.abs(w - edges[i]) < np.abs(w - edges[i - 1]), edges[i], edges[i - 1])
    slack = bound.double().numpy() + 2.0 * np.spacing(np.abs(near).astype(np.float32)).astype(np.float64)
    ambiguous = np.abs(w - near) <= slack
    same = (codes.cpu() == float64_codes(want64, q, c)).numpy()
    off_by_more = np.abs(codes.cpu().numpy() - float64_codes(want64, q, c).numpy()) > 1
    return torch.from_numpy((~same & ~ambiguous) | off_by_more), float(ambiguous.mean())


def _line(what, ratio, note=""):
    print(f"[callers f64] {what}: worst error / bound = {ratio:.3f}{note}")


def _source64(stage):
    """(the float64 value of the stage's output from its own fp32 input, the stage's bound) for the stages a mu-law coder may follow"""
    from mimikit_amd.features.functionals import resample_filter_bank
    from tests import f64_bounds as fb, filter_refs as fr
    x = stage.x.detach().cpu()
    if stage.name == "Resample":
        if int(stage.fn.orig_sr) == int(stage.fn.target_sr):
            return x.double(), torch.zeros(x.shape, dtype=torch.float64)
        orig, new, width, table = resample_filter_bank(int(stage.fn.orig_sr), int(stage.fn.target_sr))
        return fb.resample_ref(x.double(), table.double(), orig, new, width)
    co = {"Emphasis": fr.emphasis_coeffs, "Deemphasis": fr.deemphasis_coeffs}[stage.name](stage.fn.emphasis)
    x64 = x.double().numpy()
    return torch.from_numpy(fr.lfilter1_ref(x64, *co)), torch.from_numpy(fr.lfilter1_bound(x64, *co))


def check_stage(stage, before, what):
    """one stage of a record against the check its kernel's own test uses -> (kind, worst error / bound or None, ambiguous share or None)"""
    from mimikit_amd.features.functionals import mulaw_table, resample_filter_bank
    from oracle import torch_ref as O
    from tests import f64_bounds as fb, filter_refs as fr, spectral_cases as sc
    x, y = stage.x.detach().cpu(), stage.y.detach().cpu()
    if stage.name == "Resample":
        o_sr, n_sr = int(stage.fn.orig_sr), int(stage.fn.target_sr)
        if o_sr == n_sr:
            assert torch.equal(x, y), f"{what}: a resample between equal rates changed the samples"
            return "Resample", 0.0, None
        orig, new, width, table = resample_filter_bank(o_sr, n_sr)
        c = NS(id=f"{what} {o_sr}-{n_sr}-T{x.shape[1]}", T=x.shape[1])
        return "Resample", sc.resample_check(c, x, table, orig, new, width, y), None
    if stage.name == "MuLawCompress":
        q, c = stage.fn.q_levels, float(stage.fn.compression)
        assert torch.equal(y, O.mulaw_compress(x, q, c)), f"{what}: codes differ from the fp32 contract on the stage's own input"
        want64, bound = _source64(before)
        wrong, share = mulaw_rule(y, want64, bound, q, c)
        assert not bool(wrong.any()), f"{what}: {int(wrong.sum())} codes are neither the float64 code nor within the bound of an edge"
        assert share <= EDGE_SHARE_CAP, f"{what}: {share:.2%} of the samples lie within the bound of an edge (cap {EDGE_SHARE_CAP:.0%})"
        return "MuLawCompress", None, share
    if stage.name == "MuLawExpand":
        # a code outside [0, q) can only stand in the prompt: a window louder than 1 after Emphasis makes MuLawCompress return one (the
        # reference's formula does too, and its nn.Embedding then raises; the device's warm-up writes a NaN row for it).  No table entry
        # and no reference exists for such a code: they are counted, and the part that is kept - what the network generated - has none
        q = stage.fn.q_levels
        inside = (x >= 0) & (x < q)
        if not bool(inside.all()):
            print(f"[callers f64] {what}: {int((~inside).sum())} of {x.numel()} codes lie outside [0, {q}) (largest {int(x.max())}): not compared")
        assert torch.equal(y[inside], mulaw_table(q, float(stage.fn.compression))[x[inside]]), f"{what}: expanded values differ from mulaw_table"
        return "MuLawExpand", 0.0, None
    if stage.name in ("Emphasis", "Deemphasis"):
        co = {"Emphasis": fr.emphasis_coeffs, "Deemphasis": fr.deemphasis_coeffs}[stage.name](stage.fn.emphasis)
        x64 = x.double().numpy()
        want, bound = fr.lfilter1_ref(x64, *co), fr.lfilter1_bound(x64, *co)
        out = fr.outside(y.numpy(), want, bound)
        assert not out.any(), f"{what}: {int(out.sum())} samples outside lfilter1_bound"
        miss = fr.lfilter1_ref(x64, *co, defect="b1" if stage.name == "Emphasis" else "carry", at=x64.shape[-1] // 2)
        assert fr.outside(miss, want, bound).any(), f"{what}: a near miss stays inside lfilter1_bound"
        return stage.name, float((np.abs(y.numpy().astype(np.float64) - want) / np.maximum(bound, 1e-300)).max()), None
    if stage.name == "MagSpec":
        fn = stage.fn
        assert fn.center and fn.pad_mode == "constant"
        keep = O.stft_fixed_length(x.shape[1], fn.n_fft, fn.hop_length, True)
        c = NS(id=f"{what} {fn.n_fft}-{fn.hop_length}-n{keep}", n_fft=fn.n_fft, hop=fn.hop_length, coord="mag", center=True, reflect=False)
        return "MagSpec", sc.stft_check(c, x[:, x.shape[1] - keep:], y), None
    if stage.name == "GLA":
        fn, init = stage.fn, stage.init.cpu()
        want = O.griffin_lim(x, fn.n_fft, fn.hop_length, 32, 0.99, init)
        assert y.shape == want.shape, (what, y.shape, want.shape)

        def err(v):
            return float((O.stft_coord(v, fn.n_fft, fn.hop_length, "mag", center=True, pad_mode="reflect") - x).norm() / x.norm())
        e_got, e_want = err(y), err(want)
        rel = float((y - want).norm() / want.norm())
        print(f"[callers f64] {what}: Griffin-Lim of {tuple(x.shape)} frames, relative L2 {rel:.3e} (bar {GLA_REL_L2:g}); spectral inconsistency "
              f"{e_got:.5f} against the oracle's {e_want:.5f}")
        assert abs(e_got - e_want) <= 0.05 * e_want + 1e-4, f"{what}: spectral inconsistency {e_got} against the oracle's {e_want}"
        assert rel <= GLA_REL_L2, f"{what}: relative L2 {rel:.3e} > {GLA_REL_L2:g}"
        return "GLA", rel / GLA_REL_L2, None
    raise AssertionError(f"{what}: no check for a {stage.name} stage")


def event_envelope(case, history, P, n):
    """net_refs' envelope of the n steps generated behind a prompt of P positions -> (Envelope, the history the oracle was given, the prompt's
    length in it): a SampleRNN's state depends on the whole prompt; a WaveNet's steps reach rf back (net_refs' prompt is rf + 3) and a
    Seq2Seq's one step of the network, so their histories are cut to that"""
    from oracle import torch_ref as O
    from tests import net_refs as R
    hist = history.detach().cpu()
    lead = {"srnn": P, "s2s": case.hop}.get(case.kind) or O.wavenet_rf(case.arch["kernels"], case.arch["dilations"]) + 3
    assert P >= lead
    hist = hist[:, P - lead:]
    case.n, case.P, case.clips = n, lead, hist.shape[0]
    return R.envelope(hist, case), hist, lead


def check_network(rec, case, what):
    """the generated steps of a record against net_refs' envelope on the record's own history: the last step's logits (all the plan hands
    back) and every pick of a class network, every frame of a framed one -> worst error / max(E)"""
    from tests import helpers as H, net_refs as R
    n = rec.slot.n_steps
    env, hist, P = event_envelope(case, rec.history, rec.slot.P, n)
    if case.kind == "s2s":
        R64, E, dev = env.R64[:, :n], env.E[:, :n], hist[:, P:]
    else:
        R64, E, dev = env.R64[:, [n - 1]], env.E[:, [n - 1]], rec.logits.detach().cpu()[:, None]
    assert dev.shape == R64.shape, (what, dev.shape, R64.shape)
    tol_max, tol_rms = R.tolerance(E)
    r_max, r_rms = R.ratios(dev, R64, E)
    print(f"[callers f64] {what}: {dev.numel()} outputs of scale {float(R64.abs().max()):.3g}; max|dev - R64| / max(E) = {r_max:.2f}, rms(dev - R64) / rms(E) = "
          f"{r_rms:.2f} (the margin allows {R.FACTOR:g}); max(E) {float(E.max()):.3e}")
    R.check_outputs(dev, R64, tol_max, tol_rms, what)
    if case.kind != "s2s":
        picks = hist[:, P:]
        assert bool(((picks >= 0) & (picks < env.R64.shape[-1] - 1)).all()), f"{what}: a generated class lies outside the head's classes"
        if rec.temperature is None:
            R.check_picks(picks, env.R64, tol_max, what)
        else:
            ok, exact = H.sampled_picks_ok(env.R32, rec.temperature, rec.uniforms.cpu(), picks)
            print(f"[callers f64] {what}: {int(exact.sum())} of {exact.numel()} sampled picks inside their CDF interval with no slack")
            assert bool(ok.all()), f"{what}: {int((~ok).sum())} picks outside the CDF interval of their uniform"
    return r_max / R.FACTOR


def check_alignment(rec, nnn, what):
    """an NNN record: the device's end column is the float64 argmin, or its float64 cost lies within twice the bound of the minimum; the
    block is the corpus frames from there on, clamped at the corpus' end"""
    from tests import nnn_refs as N
    X, Y = rec.prompt.detach().cpu().numpy(), nnn.snd.detach().cpu().numpy()
    assert X.shape[1] <= N.MAX_ROWS
    last64 = N.dtw_last_row(N.cosine_distances(X, Y))
    e = N.cost_bound(X, Y).max(axis=(1, 2))
    bound = N.dtw_bound(last64, X.shape[1], e)
    end = rec.starts.cpu().numpy() - 1
    best = N.end_column(last64)
    rows = np.arange(X.shape[0])
    gap = last64[rows, end] - last64[rows, best]
    room = bound[rows, end] + bound[rows, best]
    assert ((end == best) | (gap <= room)).all(), f"{what}: end columns {end} against the float64 argmin {best}: gaps {gap}, twice the bound {room}"
    index = torch.from_numpy(end + 1)[:, None] + torch.arange(rec.slot.n_steps)
    assert torch.equal(rec.history.cpu(), nnn.snd.cpu()[index.clamp(max=Y.shape[0] - 1)]), f"{what}: the block is not the corpus from the start frames on"
    ratio = float((gap / np.maximum(room, 1e-300)).max())
    _line(f"{what} NNN alignment ({int((end == best).sum())} of {len(end)} end columns are the float64 argmin)", ratio)
    return ratio


def check_record(rec, case, what, nnn=None):
    """every stage of one record -> {stage label: worst error / bound}; the mu-law stages' ambiguous shares under '<label> share'"""
    out = {}
    before = None
    for k, stage in enumerate(rec.stages):
        label = f"{what} stage {k} {stage.name}"
        kind, ratio, share = check_stage(stage, before, label)
        if ratio is not None and kind != "GLA":
            _line(label, ratio)
        if share is not None:
            print(f"[callers f64] {label}: {share:.4%} of {stage.y.numel()} samples within the bound of a mu-law edge (cap {EDGE_SHARE_CAP:.0%})")
            out[label + " share"] = share
        out[label] = ratio
        before = stage
    if rec.ev.kind == "nnn":
        out[f"{what} alignment"] = check_alignment(rec, nnn, what)
    else:
        out[f"{what} network"] = check_network(rec, case, f"{what} network")
    return out


# ---- the networks, prompts and streams of the device tests ------------------------------------------------------------------------------------------
NET_SR, BASE_SR, PROMPT = 16000, 22050, 2205             # a prompt of 0.1 s at the base rate
S2S_FFT, S2S_HOP, S2S_STEP = 64, 16, 4
NNN_FFT, NNN_HOP = 256, 64
OVERRUN = (0.01, 0.1105)                                 # find_overrun(): (seconds, max_seconds)
BOUNDARY = (0.01, 0.12002267573696145)                   # find_boundary(): (seconds of both events, max_seconds)


def make_srnn():
    """hidden 32 at 16 kHz, by net_refs' factory"""
    from tests import net_refs as R
    return R._srnn("gru", 32, (16, 4, 1), 401, mlp_dim=32)


def make_wavenet():
    """helpers.wavenet_a's geometry on filter_refs.emphasis_io(0.9): Emphasis in front of the coder, Expand then Deemphasis behind it"""
    import mimikit_amd as mmk
    from oracle.weights import load_recipe
    from tests.filter_refs import emphasis_io
    net = mmk.WaveNet.from_config(mmk.WaveNet.Config(io_spec=emphasis_io(0.9), blocks=(3, 2), dims_dilated=(16,), residuals_dim=16, skips_dim=16)).eval()
    sd = load_recipe(net, seed=402, gain=2.0)
    return net, sd, dict(kernels=[2] * 5, dilations=[1, 2, 4, 1, 2], has_skips=True, residuals=True)


def make_wavenet_plain():
    """the same geometry on plain mu-law, by net_refs' factory"""
    from tests import net_refs as R
    return R._wavenet(16, (3, 2), 32, 404)


def make_s2s():
    """a framed network: MagSpec 64 / 16 with center=True on both sides (IOSpec.magspec_io builds center=False), model_dim 32, hop 4"""
    import mimikit_amd as mmk
    from oracle.weights import load_recipe
    io = mmk.IOSpec.magspec_io(mmk.IOSpec.MagSpecIOConfig(sr=NET_SR, n_fft=S2S_FFT, hop_length=S2S_HOP))
    for f in (*io.inputs, *io.targets):
        f.transform = mmk.MagSpec(S2S_FFT, S2S_HOP, center=True, window="hann")
    net = mmk.Seq2SeqLSTMNetwork.from_config(mmk.Seq2SeqLSTMNetwork.Config(io_spec=io, model_dim=32, hop=S2S_STEP)).eval()
    sd = load_recipe(net, seed=403, gain=1.5)
    return net, sd, dict(downsampling="edge_sum", upsampling="linear_resample", enc_residuals=False, dec_residuals=False)


MAKERS = {"srnn": make_srnn, "wavenet": make_wavenet, "wavenet_plain": make_wavenet_plain, "s2s": make_s2s}


def nnn_corpus(sr=NET_SR, seconds=0.5):
    """the rising tone of tests/test_gpu_nnn.py: every frame differs from its neighbours"""
    t = torch.arange(int(sr * seconds), dtype=torch.float32) / sr
    f = 300 + 2500 * t / seconds
    return 0.5 * torch.sin(2 * torch.pi * torch.cumsum(f, 0) / sr)


def event_case(key):
    """a net_refs.Case for one of the event networks, whose prompt length and step count are the record's (set by check_network)"""
    from tests import net_refs as R

    class EventCase(R.Case):
        n = None
        P = None
    kind = {"srnn": "srnn", "wavenet": "wavenet", "wavenet_plain": "wavenet", "s2s": "s2s"}[key]
    return EventCase(f"event-{key}", kind, MAKERS[key], 0, (), {}, None, hop=S2S_STEP if key == "s2s" else None)


def ev_of(key, seconds, sr=NET_SR):
    return {"srnn": Ev("class", sr, seconds), "wavenet": Ev("class", sr, seconds), "wavenet_plain": Ev("class", sr, seconds), "s2s": Ev("framed", sr, seconds, S2S_FFT, S2S_HOP),
            "nnn": Ev("nnn", sr, seconds, NNN_FFT, NNN_HOP)}[key]


class Stream(NamedTuple):
    batch: int
    C: int
    base_sr: int
    max_seconds: float
    events: tuple                # (network key, seconds, temperature)
    defects: tuple               # the defects whose re-walk must NOT reproduce the clip

    def timeline(self, defect=None):
        return timeline(self.C, self.base_sr, self.max_seconds, [ev_of(k, s) for k, s, _ in self.events], defect)


NEVER = ("srnn", 1.0, None)      # an event that never fits: it is consumed and ends the run
_COMMON = ("kept", "window_early", "write_late")
STREAMS = {
    "a": Stream(2, PROMPT, BASE_SR, 0.25, (("srnn", 0.02, None), ("wavenet", 0.01, None), ("s2s", 0.015, None), ("nnn", 0.05, None), NEVER),
                _COMMON + ("window_start", "no_plus_one")),
    "b": Stream(3, PROMPT, BASE_SR, 0.15, (("srnn", 0.02, 0.7), ("wavenet_plain", 0.01, None), NEVER), _COMMON + ("window_start",)),
    "c": Stream(2, PROMPT, BASE_SR, OVERRUN[1], (("s2s", OVERRUN[0], None), NEVER), _COMMON + ("no_plus_one",)),
    "d": Stream(2, PROMPT, BASE_SR, BOUNDARY[1], (("srnn", BOUNDARY[0], None), ("srnn", BOUNDARY[0], None), NEVER), _COMMON + ("fit_gt",)),
    "e": Stream(3, 1600, NET_SR, 0.14, (("srnn", 0.02, None), ("wavenet", 0.01, None), NEVER), _COMMON + ("window_start",)),
}


def stream_prompt(name):
    s = STREAMS[name]
    g = torch.Generator().manual_seed(600 + ord(name))
    return (torch.rand(s.batch, s.C, generator=g) * 2 - 1) * 0.5
