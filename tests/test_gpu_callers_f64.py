"""EnsembleGenerator and generate_chunks against a restated timeline (tests/caller_refs.py).

Two checks per stream of events.  The GLUE is exact: an independent re-walk of the finished clip - every event's window cut out of the
clip at the timeline's cursor, the public pieces run in the event's order, the device generator re-seeded and drawn from in the same order
- reproduces every written region bit for bit, Griffin-Lim audio included; what the timeline calls silence is exactly 0; the stream was
advanced exactly as often as the timeline says; and the re-walk under each near miss of the arithmetic that applies to the stream does NOT
reproduce the clip.  The STAGES are bounded: every stage of the defect-free re-walk is put through the check its kernel's own test uses, on
the stage's own device input (spectral_cases.resample_check / stft_check, the mu-law contract and the per-element edge rule, mulaw_table,
filter_refs.lfilter1_bound, net_refs' envelope, the two Griffin-Lim bars, nnn_refs' bound on the alignment).

Streams (tests/caller_refs.py: STREAMS): a  SampleRNN -> WaveNet with emphasis -> framed Seq2Seq -> NNN -> an event that does not fit;
b  a sampled SampleRNN event (temperature 0.7), then a greedy WaveNet on plain mu-law (behind an Emphasis(0.9) the sampled event's
loud audio leaves [-1, 1] under 11 of 12 seeds tried, the coder returns classes past 255 and the event raises - the case of
test_window_that_leaves_the_coders_range_raises);  c  a framed event that passes the fit rule and overruns the clip;
d  an event exactly on the fit rule's boundary;  e  base_sr == sr.

Records of the first run on an MI355X (worst error / bound per stage; records, not tolerances):
  Resample 22050 <-> 16000     0.055 .. 0.096 over the 22 resample stages of streams a - d (0 between equal rates: the input itself)
  Emphasis(0.9)                0.236 (a), 0.241 (e);   Deemphasis(0.9)  0.032 (a), 0.033 (e)
  MuLawCompress                the fp32 contract bit for bit on every stage; samples within the bound of an edge: 0 % (a, e),
                               0.0417 % of 4800 (b, both events), 0.0312 % of 3200 (d); cap 1 %
  MuLawExpand                  mulaw_table bit for bit on every stage
  MagSpec 64 / 16              0.102 (a), 0.079 (c);   MagSpec 256 / 64 (NNN prompt, 26 frames)  0.121
  Griffin-Lim, 32 iterations   relative L2 4.07e-05 on (2, 117, 33) frames (a, Seq2Seq), 2.88e-05 on (2, 112, 33) (c), 1.16e-04 on (2, 13, 129)
                               (a, NNN); bar 2e-3.  Spectral inconsistency equal to the oracle's to five digits (0.13081, 0.12935, 0.20151)
  networks, max|dev - R64| / max(E) (the margin allows 4):  SampleRNN 1.05 (a), 1.14 (b, sampled), 0.58 (d), 1.36 (e);
                               WaveNet 1.07 (a), 0.86 (b, plain mu-law), 0.89 (e);  Seq2Seq 0.78 (a), 0.71 (c)
  sampled picks                960 of 960 (b) and 3 x 144 of 144 (generate_chunks at temperatures 0.5, 1.0, 1.5) inside their CDF interval with no
                               slack; against another chunk's uniforms 3 of 144, against another chunk's temperature 19 of 144
  NNN alignment                2 of 2 end columns are the float64 argmin
  generate_chunks, Seq2Seq     0.43, 0.32, 0.36 over the three chunks of 9 frames
  defects that break bit equality:  a  kept, window_early, window_start, write_late, no_plus_one;  b, e  kept, window_early, window_start,
                               write_late;  c  kept, window_early, write_late, no_plus_one;  d  kept, window_early, write_late, fit_gt.
                               cursor_written applies to c alone and cannot show in a clip (tests/caller_refs.py)
  state after the callers      on the parent commit: grad mode off, the network in eval mode and on the device after EnsembleGenerator.run()
"""
import functools

import pytest
import torch

import mimikit_amd as mmk
from mimikit_amd.models.nnn import NearestNextNeighbor
from tests import caller_refs as cr
from tests import helpers as H
from tests import net_refs as R

pytestmark = pytest.mark.gpu
SEED = 4321


@pytest.fixture(autouse=True)
def _grad_mode_as_found():
    """the loop's teardown turns grad mode on, as the reference's does: the tests of this module leave the mode they found"""
    before = torch.is_grad_enabled()
    yield
    torch.set_grad_enabled(before)


@functools.lru_cache(maxsize=None)
def _nets(device):
    nets = {key: make()[0].to(device).eval() for key, make in cr.MAKERS.items()}
    nets["nnn"] = NearestNextNeighbor(mmk.MagSpec(cr.NNN_FFT, cr.NNN_HOP), cr.nnn_corpus(), sr=cr.NET_SR, device=device)
    return nets


class Counted:
    """an event stream that counts how often it was asked"""

    def __init__(self, items):
        self.items, self.asked = iter(items), 0

    def __iter__(self):
        return self

    def __next__(self):
        self.asked += 1
        return next(self.items)


def _play(name, device, seed):
    s, nets = cr.STREAMS[name], _nets(device)
    stream = Counted([dict(generator=nets[key], seconds=seconds, temperature=temperature) for key, seconds, temperature in s.events])
    eg = mmk.EnsembleGenerator(cr.stream_prompt(name), max_seconds=s.max_seconds, base_sr=s.base_sr, stream=stream, device=device)
    torch.manual_seed(seed)
    clip = eg.run()
    players = [cr.Player(cr.ev_of(key, seconds), nets[key], temperature) for key, seconds, temperature in s.events]
    return clip, s.timeline(), players, stream, eg


@functools.lru_cache(maxsize=None)
def _run(name, device):
    """one stream through EnsembleGenerator, once per session: (clip, timeline, players, the counted stream, the generator object)"""
    return _play(name, device, SEED)


@functools.lru_cache(maxsize=None)
def _rewalked(name, device):
    clip, tl, players, _, _ = _run(name, device)
    return cr.rewalk(clip, tl.C, players, tl, SEED)


@pytest.mark.parametrize("name", list(cr.STREAMS))
def test_rewalk_reproduces_the_clip_bit_for_bit(device, name):
    clip, tl, players, stream, eg = _run(name, device)
    s = cr.STREAMS[name]
    assert clip.shape == (s.batch, tl.total)
    assert torch.equal(clip[:, :tl.C].cpu(), cr.stream_prompt(name)), "the prompt was touched"
    silent = cr.silence_mask(tl)
    assert bool(silent.any()) == (name != "c")            # (the overrunning piece fills the clip)
    assert not bool(clip.cpu()[:, silent].any()), "something was written where the timeline has silence"
    out, records = _rewalked(name, device)
    for k, slot in enumerate(tl.slots):
        if slot.fits:
            region = slice(slot.at, slot.at + slot.written)
            assert float(clip[:, region].abs().max()) > 0, f"stream {name}: event {k} wrote nothing"
            assert torch.equal(out[:, region], clip[:, region]), f"stream {name}: event {k}'s region {region} differs from the re-walk's"
    assert torch.equal(out, clip)
    # events consumed: as many as the timeline says (one that does not fit included), none once the cursor has reached the end
    assert not tl.exhausted and stream.asked == len(tl.slots) == len(records)
    assert [r is not None for r in records] == [slot.fits for slot in tl.slots]
    assert eg.generate_step(tl.total, clip[:, -tl.C:]) is None and eg.generate_step(tl.total + 5, clip[:, -tl.C:]) is None
    assert stream.asked == len(tl.slots), "an event was drawn past the end of the clip"


@pytest.mark.parametrize("name", list(cr.STREAMS))
def test_rewalk_with_a_defect_does_not_reproduce_the_clip(device, name):
    clip, tl, players, _, _ = _run(name, device)
    s = cr.STREAMS[name]
    applied = []
    for defect in cr.DEFECTS:
        if not cr.applies(tl, defect):
            continue
        out, _ = cr.rewalk(clip, tl.C, players, tl, SEED, defect)
        if cr.shows_in_clip(tl, defect):
            applied.append(defect)
            assert not torch.equal(out, clip), f"stream {name}: the re-walk with the defect '{defect}' still reproduces the clip"
        else:
            # the cursor behind an overrunning event: an integer no clip can show (tests/caller_refs.py) - recorded, not required
            assert defect == "cursor_written" and name == "c" and torch.equal(out, clip)
    assert tuple(applied) == tuple(d for d in cr.DEFECTS if d in s.defects), (name, applied)
    print(f"[callers f64] stream {name}: defects that break bit equality: {', '.join(applied)}")


@pytest.mark.parametrize("name", list(cr.STREAMS))
def test_every_stage_of_the_rewalk_stays_inside_its_bound(device, name):
    _, tl, players, _, _ = _run(name, device)
    _, records = _rewalked(name, device)
    s = cr.STREAMS[name]
    failures = []
    for k, (rec, (key, _, _)) in enumerate(zip(records, s.events)):
        if rec is None:
            continue
        try:
            got = cr.check_record(rec, None if key == "nnn" else cr.event_case(key), f"stream {name} event {k} ({key})", _nets(device)["nnn"])
        except AssertionError as err:              # (every event's figures are printed before the first failure is raised)
            failures.append(err)
            continue
        for label, value in got.items():
            if label.endswith(" share"):
                assert value <= cr.EDGE_SHARE_CAP, label
    if failures:
        raise failures[0]


def test_exhausted_stream_raises_stop_iteration(device):
    eg = mmk.EnsembleGenerator(cr.stream_prompt("c"), max_seconds=0.15, base_sr=cr.BASE_SR, stream=iter([]), device=device)
    with pytest.raises(StopIteration):
        eg.run()


def test_window_that_leaves_the_coders_range_raises(device):
    """a 3 kHz square wave of amplitude 0.95: behind the WaveNet's Emphasis(0.9) every edge reaches about 1.8, and the mu-law formula
    returns classes past 255 there.  The reference's nn.Embedding raises IndexError on them; the step kernels would go on from NaN rows"""
    t = torch.arange(cr.PROMPT, dtype=torch.float64) / cr.BASE_SR
    loud = (0.95 * torch.sign(torch.sin(2 * torch.pi * 3000 * t))).float().expand(2, -1).contiguous()
    at_net = mmk.Emphasis(0.9)(mmk.Resample(cr.BASE_SR, cr.NET_SR)(loud.to(device)))
    assert float(at_net.abs().max()) > 1.5 and int(mmk.MuLawCompress()(at_net).max()) > 255
    stream = Counted([dict(generator=_nets(device)["wavenet"], seconds=0.01)])
    eg = mmk.EnsembleGenerator(loud, max_seconds=0.15, base_sr=cr.BASE_SR, stream=stream, device=device)
    with pytest.raises(IndexError, match="out of range"):
        eg.run()
    assert stream.asked == 1


# ---------------------------------------------------------------------------------------------------------------- generate_chunks
def _picks_ok(key, prompt, chunk, what, temperature=None, uniforms=None):
    """one chunk's picks (or frames) against net_refs' envelope on its own history: the prompt it was given and what it generated"""
    case = cr.event_case(key)
    n = chunk.shape[1]
    env, hist, P = cr.event_envelope(case, torch.cat([prompt, chunk], 1), prompt.shape[1], n)
    if key == "s2s":
        tol_max, tol_rms = R.tolerance(env.E[:, :n])
        r_max, _ = R.ratios(hist[:, P:], env.R64[:, :n], env.E[:, :n])
        print(f"[callers f64] {what}: {n} frames, max|dev - R64| / max(E) = {r_max:.2f} (the margin allows {R.FACTOR:g})")
        R.check_outputs(hist[:, P:], env.R64[:, :n], tol_max, tol_rms, what)
    elif temperature is None:
        R.check_picks(hist[:, P:], env.R64, R.tolerance(env.E[:, [n - 1]])[0], what)
    else:
        ok, exact = H.sampled_picks_ok(env.R32, temperature, uniforms.cpu(), hist[:, P:])
        print(f"[callers f64] {what}: {int(exact.sum())} of {exact.numel()} sampled picks inside their CDF interval with no slack")
        assert bool(ok.all()), f"{what}: {int((~ok).sum())} picks outside the CDF interval of their uniform at temperature {temperature}"


def _prompts_seen(net, monkeypatch):
    """the prompts the loop hands to before_generate (its own calls carry the batch's index, the network's internal ones None)"""
    seen, before = [], net.before_generate

    def spy(prompts, batch_index):
        if batch_index is not None:
            seen.append(prompts[0].clone())
        return before(prompts, batch_index)
    monkeypatch.setattr(net, "before_generate", spy, raising=False)
    return seen


def test_generate_chunks_wavenet_warms_up_on_the_previous_tail(device, monkeypatch):
    net = _nets(device)["wavenet"]
    n_prompt, n = net.rf + 5, 40
    seed = torch.randint(0, 256, (2, n_prompt), generator=torch.Generator().manual_seed(14)).to(device)
    seen = _prompts_seen(net, monkeypatch)
    cfg = mmk.GenerateLoopV2.Config(output_duration_sec=n / cr.NET_SR, display_waveform=False, yield_inversed_outputs=False)
    chunks = list(mmk.generate_chunks(cfg, net, seed, 3))
    assert len(chunks) == len(seen) == 3 and all(c.shape == (2, n) and c.dtype == torch.int64 for c in chunks)
    assert torch.equal(seen[0], seed)
    for i, chunk in enumerate(chunks):
        _picks_ok("wavenet", seen[i], chunk, f"generate_chunks wavenet chunk {i}")
        if i + 1 < len(chunks):
            assert torch.equal(seen[i + 1], torch.cat([seen[i], chunk], 1)[:, -n_prompt:]), f"chunk {i + 1} was not prompted with chunk {i}'s tail"


def test_generate_chunks_framed_network(device, monkeypatch):
    net = _nets(device)["s2s"]
    bins, n_prompt = cr.S2S_FFT // 2 + 1, 2 * cr.S2S_STEP
    seed = torch.rand(3, n_prompt, bins, generator=torch.Generator().manual_seed(15)).to(device)
    seen = _prompts_seen(net, monkeypatch)
    cfg = mmk.GenerateLoopV2.Config(output_duration_sec=0.008, display_waveform=False, yield_inversed_outputs=False)
    n = int(cr.NET_SR * 0.008) // cr.S2S_HOP + 1                      # 9 frames: two whole steps of the network and one cut short
    chunks = list(mmk.generate_chunks(cfg, net, seed, 3))
    assert n == 9 and len(chunks) == len(seen) == 3 and all(c.shape == (3, n, bins) for c in chunks)
    for i, chunk in enumerate(chunks):
        _picks_ok("s2s", seen[i], chunk, f"generate_chunks seq2seq chunk {i}")
        if i + 1 < len(chunks):
            assert torch.equal(seen[i + 1], torch.cat([seen[i], chunk], 1)[:, -n_prompt:])


def test_generate_chunks_update_parameters(device, monkeypatch):
    net = _nets(device)["srnn"]
    temps, n, n_prompt = (0.5, 1.0, 1.5), 48, 32
    seed = torch.randint(0, 256, (3, n_prompt), generator=torch.Generator().manual_seed(16)).to(device)
    seen, calls = _prompts_seen(net, monkeypatch), []

    def update(parameters, i):
        calls.append((dict(parameters), i))
        return {"temperature": temps[min(i + 1, len(temps) - 1)]}
    cfg = mmk.GenerateLoopV2.Config(output_duration_sec=n / cr.NET_SR, parameters={"temperature": temps[0]}, display_waveform=False,
                                    yield_inversed_outputs=False)
    torch.manual_seed(SEED)
    chunks = list(mmk.generate_chunks(cfg, net, seed, 3, update_parameters=update))
    assert calls == [({"temperature": t}, i) for i, t in enumerate(temps)]
    torch.manual_seed(SEED)
    uniforms = [torch.rand((3, n), device=device) for _ in temps]          # drawn in order, one block per chunk
    assert len(chunks) == 3
    for i, chunk in enumerate(chunks):
        _picks_ok("srnn", seen[i], chunk, f"generate_chunks sampled chunk {i} at temperature {temps[i]}", temps[i], uniforms[i])
    # the uniforms of another chunk, or another chunk's temperature, do not explain the picks: the check can tell the chunks apart
    with pytest.raises(AssertionError):
        _picks_ok("srnn", seen[1], chunks[1], "chunk 1 against chunk 0's uniforms", temps[1], uniforms[0])
    with pytest.raises(AssertionError):
        _picks_ok("srnn", seen[2], chunks[2], "chunk 2 against chunk 0's temperature", temps[0], uniforms[2])


# ---------------------------------------------------------------------------------------------------------------- state after the callers
def test_callers_put_grad_mode_training_mode_and_device_back(device):
    """a reader that stops at the loop's first yield skips the teardown behind the loop (the reference leaks the same state): both callers
    close the generator, and GenerateLoopV2.run() restores what it found in a `finally`"""
    net = cr.make_srnn()[0].train()                   # on the host, in training mode
    before = torch.is_grad_enabled()
    torch.set_grad_enabled(True)
    try:
        home = net.device
        stream = iter([dict(generator=net, seconds=0.01), dict(generator=net, seconds=1.0)])
        clip = mmk.EnsembleGenerator(cr.stream_prompt("d"), max_seconds=0.13, base_sr=cr.BASE_SR, stream=stream, device=device).run()
        state = (torch.is_grad_enabled(), net.training, net.device)
        assert float(clip[:, cr.PROMPT:cr.PROMPT + 221].abs().max()) > 0
        assert state == (True, True, home), f"after EnsembleGenerator.run(): grad enabled, training, device = {state}"
        torch.set_grad_enabled(True)
        net.train()
        seed = torch.randint(0, 256, (2, 32), generator=torch.Generator().manual_seed(17)).to(device)
        cfg = mmk.GenerateLoopV2.Config(output_duration_sec=32 / cr.NET_SR, display_waveform=False, yield_inversed_outputs=False)
        chunks = list(mmk.generate_chunks(cfg, net, seed, 2))
        state = (torch.is_grad_enabled(), net.training, net.device)
        assert len(chunks) == 2
        assert state == (True, True, home), f"after a drained generate_chunks: grad enabled, training, device = {state}"
    finally:
        torch.set_grad_enabled(before)
