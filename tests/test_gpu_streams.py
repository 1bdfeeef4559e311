"""Every entry point that takes an mmk_stream_t, on a side stream behind a busy one (tests/stream_cases.py has the table, the cases and
the method).  The float64 suites establish that the default-stream result is right and that two calls give the same bits; on the default
stream a launch that forgot its stream argument, a memset on stream 0, a blocking copy and a table read before it is ready all give the
right bits too.  Here the input is written LATE - a device-to-device copy on the side stream behind a delay - so that whatever the library
enqueues elsewhere computes from a stale (valid, different) input, and every comparison is bitwise against the default-stream run.

  1. every ASYNC stateless entry point (C ABI, outputs inside NaN / sentinel surrounds, zero-filled workspaces): the default stream
     twice (same bits), the stale input once (other bits), then late_input on a side stream: the default-stream bits, nothing
     written around the outputs, and the stream still busy when the call returns - the header's rule, and the proof that the delay was
     still pending when the launches were enqueued;
  2. the WAITS stateless entry points the same way without the busy assertion: the late write tests only what they enqueue before
     their first wait;
  3. the plans through native's plan classes, one case per step kernel: committed and run on the default stream, then warm-up,
     generate (and the single-step calls) and last_logits behind the delay with the prompt written late; greedy, sampled, and a
     graph-replayed block of the launch path;
  4. the plans' error word on a side stream: injected, reported once, clean the second time, and a generation right behind it;
  5. two side streams, the same stateless function on both behind their own delays: scratch shared inside the library would show;
  6. the first spectral call of a fresh process on a side stream (the lazily built twiddle and window tables), another stream right after;
  7. the method can fail: the same late-input call GIVEN the null stream computes from the stale input and is seen.

No test provokes a fault or a time-out: stale inputs and workspaces are valid values, no two plans run side by side, and the only spin is
torch.cuda._sleep on one wave.

WAITS (tests/stream_cases.py: ENTRY_POINTS has the quoted lines): mmk_edge_components_i64 (csrc/hcluster.hip:286), mmk_pca_eig_f64
(csrc/pca.hip:730), mmk_srnn_reset (csrc/srnn_plan.hip:402), mmk_wavenet_commit (csrc/wavenet_plan.hip:549, :767, :842), mmk_srnn_commit
(csrc/srnn_plan.hip:455), mmk_tr_commit (csrc/transformer_plan.hip:197), mmk_s2s_commit (allowed to; enqueues everything today),
mmk_{wavenet,srnn,s2s}_sync_status and mmk_{wavenet,srnn,s2s}_inject_sync_error.  Conditional: a graph captured anew
(csrc/wavenet_plan.hip:1256, csrc/srnn_plan.hip:862, csrc/transformer_plan.hip:375) and the first spectral call of a process
(csrc/istft.hip:106).

Found by reading, fixed before the first run: mmk_srnn_sync_status and mmk_wavenet_sync_status read the error word with a blocking
hipMemcpy and (SampleRNN) cleared it with a hipMemset on the null stream, which is not ordered against a non-blocking side stream; both
now use the Async forms on `stream`.  mmk_wavenet_sync_status never cleared its word, so a second call reported the same time-out again;
it now clears it where it reports it, as the other two plans do.

RECORDS of the first run on an MI355X (records, not thresholds; the delay is a parameter and `busy` the condition):
  torch.cuda._sleep: 2382839 cycles per ms (5000000 cycles timed between two events), the delay of 50 ms = 119 141 950 cycles.
  A null-stream fill overtook 7 of 8 side streams held by a delay (xxxx.xxx): the eighth shares the null stream's hardware queue.  The
  first run of this file took its side streams as torch handed them out, and mmk_stft_mag_f32[1024] GIVEN the null stream came back
  with the real input's bits on such a stream: the method saw nothing there.  Since then every test runs behind a stream that the
  probe has seen overtaken (stream_cases.side_stream), and both null-stream cases are detected (12291 of 12291 and 9234 of 9234
  outputs differ).
  Host time of the call in ms and the stream's state on return, per case:
  mmk_fingerprint_u32                 0.050  busy    mmk_fingerprint_buffers_u32         0.034  busy
  mmk_mulaw_compress_f32_i64          0.017  busy    mmk_mulaw_expand_i64_f32            0.039  busy
  mmk_resample_f32                    0.027  busy    mmk_lfilter1_f32                    0.017  busy
  mmk_row_normalize_f32               0.019  busy    mmk_inv_row_norm_f32                0.013  busy
  mmk_cosine_cost_f32                 0.016  busy    mmk_dtw_subseq_f32                  0.012  busy
  mmk_nn_cosine_f32                   0.018  busy    mmk_cum_entropy_i64                 0.014  busy
  mmk_nn_cosine_self_f32              0.022  busy    mmk_nn_components_i64               0.054  busy
  mmk_segment_mean_f32                0.017  busy    mmk_nn_topk_f32                     0.017  busy
  mmk_half_neg_sqnorm_f32             0.029  busy    mmk_novelty_f32                     0.015  busy
  mmk_novelty_finish_f32              0.020  busy    mmk_pick_peaks_f32                  0.017  busy
  mmk_pca_colstats_f64                0.027  busy    mmk_pca_cov_f64                     0.019  busy
  mmk_pca_project_f32                 0.014  busy    mmk_stft_mag_f32[1024]              0.015  busy
  mmk_stft_mag_f32[2048]              0.013  busy    mmk_stft_mag_f32[256]               0.017  busy
  mmk_stft_f32[1024]                  0.016  busy    mmk_stft_f32[2048]                  0.017  busy
  mmk_stft_f32[256]                   0.017  busy    mmk_stft_energy_f32[1024]           0.017  busy
  mmk_stft_energy_f32[2048]           0.016  busy    mmk_stft_energy_f32[256]            0.017  busy
  mmk_interp1d_f32                    0.014  busy    mmk_derivative_f32                  0.018  busy
  mmk_hpss_f32                        0.014  busy    mmk_melbank_f32                     0.047  busy
  mmk_stft_mel_f32[1024]              0.049  busy    mmk_stft_mel_f32[2048]              0.046  busy
  mmk_stft_mel_f32[256]               0.048  busy    mmk_istft_f32[1024]                 0.025  busy
  mmk_istft_f32[2048]                 0.046  busy    mmk_istft_f32[256]                  0.016  busy
  mmk_gla_f32                         0.032  busy    mmk_pack_weight_f32                 0.016  busy
  mmk_linear_f32                      0.011  busy    mmk_gemm_f32                        0.012  busy
  mmk_gemm_bias_act_f32               0.016  busy    mmk_skinny_linear_f32               0.011  busy
  mmk_tr_attention_f32                0.012  busy    mmk_tr_add_ln_f32                   0.011  busy
  mmk_categorical_sample_f32_i64      0.015  busy    mmk_edge_components_i64            49.857  busy
  mmk_pca_eig_f64                    49.897  busy
  (the two WAITS cases return after the delay, 49.9 ms, and are busy again with what they enqueue after their last wait)
  Plans, busy after warm-up / generate / step / last_logits in every case (steps of the block in brackets):
  wavenet-launches (9), wavenet-persist (9), wavenet-chain (9), wavenet-lpipe-4_3-13 (9), wavenet-spipe-5 (9), wavenet-spipe-pair-24
  (9), wavenet-bpipe-20 (9), wavenet-frames-g4 (9), srnn-launches (9), srnn-bottom-one_clip (9), srnn-bottom-four_clips-321 (9), srnn-
  resident-gru (44), s2s-resident-128-2-3 (4), s2s-per_frame (16), s2s-launches (16), s2s-classes (8), tr-one_layer_rf9 (9), wavenet-
  chain-sampled (9), srnn-bottom-one_clip-sampled (9), tr-one_layer_rf9-sampled (9), wavenet-launches-graph (19)
  Nothing was found by the runs: every ASYNC case came back busy with the default-stream bits on the first run, every plan too, and
  the error word behaved on the side stream (the library under test already had the fix above; the null-stream hipMemset was not run).
"""
import subprocess
import sys

import pytest
import torch

from mimikit_amd import native
from tests import stream_cases as S

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)


@pytest.fixture(autouse=True)
def _nothing_more_after_a_gpu_fault():
    """a fault on the device (an illegal access, an abort of the queue) surfaces at the next synchronisation: end the session there
    instead of starting the remaining tests on a device in that state"""
    yield
    if torch.cuda.is_available():
        try:
            torch.cuda.synchronize()
        except RuntimeError as err:
            pytest.exit(f"the device reported a fault ({err}): nothing more is started on it", returncode=3)


# ---------------------------------------------------------------------------------------------------------------- stateless entry points
def _describe(a, b):
    return {k: f"{int((a[k] != b[k]).sum())} of {a[k].numel()} differ" for k in a if not S.same_bits(a[k], b[k])}


def _default_runs(bound, what):
    """the real input twice (the same bits; code loading) and the stale input once (other bits, or the case proves nothing)"""
    want = bound.run_default("real")
    again = bound.run_default("real")
    assert not S.differs(want, again), (what, "two default-stream calls disagree", _describe(want, again))
    bound.check_surround(what + " on the default stream")
    stale = bound.run_default("stale")
    assert S.differs(want, stale), (what, "the stale input gives the real input's bits: the case proves nothing")
    return want


@pytest.mark.parametrize("case", S.ASYNC_CASES, ids=[c.id for c in S.ASYNC_CASES])
def test_async_entry_point_behind_a_busy_stream(device, case):
    bound = S.Bound(case, device)
    want = _default_runs(bound, case.id)
    side = S.side_stream(device)
    got, busy, host = S.late_input(bound, side)
    print(f"[streams] {case.id}: host time of the call {host * 1e3:.3f} ms, busy on return: {busy}; delay {case.delay_ms:g} ms at "
          f"{S.cycles_per_ms():.0f} cycles / ms")
    assert not S.differs(want, got), (case.id, "behind a late input on a side stream the outputs differ from the default-stream run", _describe(want, got))
    bound.check_surround(case.id + " on the side stream")
    assert busy, (case.id, f"the call waited for its stream (or took {host * 1e3:.1f} ms on the host): the delay was over when it returned")


@pytest.mark.parametrize("case", S.WAITS_CASES, ids=[c.id for c in S.WAITS_CASES])
def test_waiting_entry_point_behind_a_busy_stream(device, case):
    """these wait for the stream by design (stream_cases.ENTRY_POINTS: where and why), so there is no busy assertion, and the late write
    tests only what the entry point enqueues before its first wait"""
    bound = S.Bound(case, device)
    want = _default_runs(bound, case.id)
    got, busy, host = S.late_input(bound, S.side_stream(device))
    print(f"[streams] {case.id} (waits): host time of the call {host * 1e3:.3f} ms, busy on return: {busy}")
    assert not S.differs(want, got), (case.id, _describe(want, got))
    bound.check_surround(case.id + " on the side stream")


@pytest.mark.parametrize("cid", S.TWO_STREAM_CASES)
def test_two_side_streams_at_once(device, cid):
    """the same call on streams A and B back to back with different inputs, each behind its own delay, neither stream synchronised until
    both calls have returned: each result is its own default-stream bits (scratch shared inside the library would mix them)"""
    case = S.BY_ID[cid]
    a, b = S.Bound(case, device, seed=0), S.Bound(case, device, seed=100)
    want_a, want_b = _default_runs(a, cid + " A"), _default_runs(b, cid + " B")
    assert S.differs(want_a, want_b)
    sa, sb = S.side_streams(device, 2)
    a.fill("stale")
    b.fill("stale")
    torch.cuda.synchronize()
    for bound, stream in ((a, sa), (b, sb)):
        S.delay(stream, case.delay_ms)
        with torch.cuda.stream(stream):
            bound.late_copy()
        bound.call(stream.cuda_stream)
    busy = (not sa.query(), not sb.query())
    sa.synchronize()
    sb.synchronize()
    torch.cuda.synchronize()
    got_a, got_b = a.outputs(), b.outputs()
    assert not S.differs(want_a, got_a), (cid, "stream A", _describe(want_a, got_a))
    assert not S.differs(want_b, got_b), (cid, "stream B", _describe(want_b, got_b))
    a.check_surround(cid + " A")
    b.check_surround(cid + " B")
    assert busy[1], (cid, "stream B's delay was over when both calls had returned", busy)


@pytest.mark.parametrize("cid", S.NULL_STREAM_CASES)
def test_a_null_stream_launch_is_seen(device, cid):
    """the method can fail: GIVEN stream 0 while the side stream holds the delay and the late write, the kernel runs on the stale input
    and the comparison of the tests above reports it"""
    bound = S.Bound(S.BY_ID[cid], device)
    want = _default_runs(bound, cid)
    got, _, _ = S.late_input(bound, S.side_stream(device), call_stream=0)
    assert S.differs(want, got), S.NOT_ORDERED
    print(f"[streams] {cid} given the null stream: {_describe(want, got)} - a null-stream launch is detected")


def test_which_side_streams_the_null_stream_overtakes(device):
    """the premise of every test here, measured: of eight streams torch hands out in turn, the ones a null-stream fill overtakes while
    a delay holds them (the others share the null stream's hardware queue and are ordered behind it: tests/stream_cases.py).  The tests
    run behind streams of the first kind only (S.side_stream)"""
    streams = [torch.cuda.Stream(device) for _ in range(8)]
    S.cycles_per_ms()
    seen = [S.null_stream_overtakes(s) for s in streams]
    print(f"[streams] a null-stream fill overtakes {sum(seen)} of {len(seen)} side streams held by a delay: {''.join('x' if v else '.' for v in seen)}")
    assert any(seen), S.NOT_ORDERED


def test_first_spectral_call_of_a_process(device):
    """the library's only lazily built device state (csrc/istft.hip: spectral_tables): a fresh child whose first library call is
    mmk_stft_mag_f32 on a side stream behind the delay and a late input, then mmk_istft_f32 on a second side stream at once; both again
    on the default stream, bit for bit (tests/stream_cases.py: first_call)"""
    run = subprocess.run([sys.executable, "-m", "tests.stream_cases", "first-call"], cwd=str(S.ROOT), capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, (run.returncode, run.stdout[-2000:], run.stderr[-2000:])


# ---------------------------------------------------------------------------------------------------------------- plans
class PlanRun:
    """a PlanCase on the device: the network of the refs case, its plan committed on the default stream, the loop's tensors with the
    prompt (real or stale: class 0 / zero frames, another draw of the conditioning) and blanks behind it, and `drive`: the plan's
    calls on torch's current stream, every output into a tensor allocated here"""

    def __init__(self, pc, device, monkeypatch):
        self.pc, self.device, self.L = pc, device, native.lib()
        ref = self.ref = S.plan_ref(pc)
        for k in [k for k in native.PLAN_TUNING if k.startswith("MMK_")]:
            monkeypatch.delitem(native.PLAN_TUNING, k)
        if pc.network == "tr":
            from tests import transformer_refs as TR
            self.net = TR.build_case(ref, device)
            prompt, conds, self.P, self.B, self.hop, self.classes = ref.inputs(), (), ref.prompt, ref.clips, 1, ref.classes
        else:
            for k, v in ref.env.items():
                monkeypatch.setitem(native.PLAN_TUNING, k, v)
            self.net = ref.make()[0].to(device)
            prompt, conds = ref.inputs()
            self.P, self.B, self.hop, self.classes = ref.P, ref.clips, ref.hop or 1, ref.classes
        assert isinstance(prompt, torch.Tensor)
        self.resident_srnn = pc.network == "srnn" and pc.ref.startswith("resident")
        self.n = pc.n or (ref.parts[0] if self.resident_srnn else 2 * self.hop if pc.network == "s2s" else S.SHORT_BLOCK)
        B, P, n = self.B, self.P, self.n
        self.prompt = prompt.to(device)
        self.data = torch.cat([prompt, torch.zeros(B, n, *prompt.shape[2:], dtype=prompt.dtype)], 1).to(device)
        self.conds = tuple(c.to(device).contiguous() for c in conds)
        self.conds_real = tuple(c.clone() for c in self.conds)
        self.conds_stale = tuple(torch.rand(c.shape, generator=S.gen(S.STALE + j)).to(device) for j, c in enumerate(conds))
        self.temp = self.uni = None
        if pc.sampled:
            self.temp = torch.linspace(0.5, 1.5, B).to(device)
            self.uni = torch.rand(B, n, generator=S.gen(31)).to(device)
        self.net._ensure_plan(B, refresh_weights=True)           # commits (and fingerprints the weights): both wait, on the default stream
        self.plan = plan = self.net._plan
        cfg = plan.cfg
        self.logits = self.step_y = None
        if pc.network == "wavenet":
            assert isinstance(plan, native.WaveNetPlan)
            self.rf = plan.rf
            if self.classes:
                self.logits = torch.empty(B, plan._logit_columns("out_dim", 0), device=device)
        elif pc.network == "srnn":
            self.logits = torch.empty(B, plan._logit_columns("q_levels", 0), device=device)
        elif pc.network == "s2s":
            if self.classes:
                self.logits = torch.empty(B * self.hop, cfg.out_dim + (1 if cfg.learn_temp else 0), device=device)
                self.step_y = torch.empty(B, self.hop, dtype=torch.int64, device=device)
            else:
                self.step_y = torch.empty(B, self.hop, cfg.out_dim, device=device)
        else:
            self.rf = ref.rf
            self.logits = torch.empty(B, cfg.out_dim + (1 if cfg.learn_temp else 0), device=device)
            self.step_y = torch.empty(B, dtype=torch.int64, device=device)
        self.blocks = 0
        torch.cuda.synchronize()

    def place(self, which):
        """the real or the stale prompt and conditioning, blanks behind the prompt, outputs cleared (torch's current stream)"""
        if which == "real":
            self.data[:, :self.P].copy_(self.prompt)
        else:
            self.data[:, :self.P].zero_()
        self.data[:, self.P:].zero_()
        for c, v in zip(self.conds, self.conds_real if which == "real" else self.conds_stale):
            c.copy_(v)
        for t in (self.logits, self.step_y):
            if t is not None:
                t.fill_(-5)

    def late_copy(self):
        self.data[:, :self.P].copy_(self.prompt, non_blocking=True)
        for c, v in zip(self.conds, self.conds_real):
            c.copy_(v, non_blocking=True)

    def reset(self):
        if self.pc.network == "srnn":
            self.plan.reset()                                    # waits (csrc/srnn_plan.hip:402): before the delay

    def drive(self):
        pc, plan, L, B, P, n, data, s = self.pc, self.plan, self.L, self.B, self.P, self.n, self.data, native.stream_ptr(self.device)
        h, ptr = plan.handle, native.ptr
        if pc.network == "wavenet":
            plan.warmup(data, self.conds, P - self.rf, P - 1)
            plan.generate(data, self.conds, P, n, self.temp, self.uni)
            if self.classes:
                native.check(L.mmk_wavenet_last_logits_of(h, 0, B, ptr(self.logits), self.logits.stride(0), s), "mmk_wavenet_last_logits_of")
                native.check(L.mmk_wavenet_last_logits(h, B, ptr(self.logits), self.logits.stride(0), s), "mmk_wavenet_last_logits")
            self.blocks += 1
        elif pc.network == "srnn":
            if pc.ref == "launches" or pc.sampled:               # the one-input entry points; the other cases through native's wrappers: the _multi ones
                native.check(L.mmk_srnn_warmup(h, B, ptr(data), data.stride(0), P, s), "mmk_srnn_warmup")
                native.check(L.mmk_srnn_generate(h, B, ptr(data), data.stride(0), P, n, ptr(self.temp), ptr(self.uni), s), "mmk_srnn_generate")
            else:
                plan.warmup(data, P)
                plan.generate(data, P, n, self.temp, self.uni)
            native.check(L.mmk_srnn_last_logits_of(h, 0, B, ptr(self.logits), self.logits.stride(0), s), "mmk_srnn_last_logits_of")
            native.check(L.mmk_srnn_last_logits(h, B, ptr(self.logits), self.logits.stride(0), s), "mmk_srnn_last_logits")
            self.blocks += 1
        elif pc.network == "s2s":
            x, y = data[:, :self.hop], self.step_y
            if self.classes:
                native.check(L.mmk_s2s_step_classes(h, B, ptr(x), x.stride(0), x.stride(1), ptr(y), y.stride(0), y.stride(1), s), "mmk_s2s_step_classes")
                plan.generate_classes(data, P, n)
                native.check(L.mmk_s2s_last_logits(h, B, ptr(self.logits), self.logits.stride(0), s), "mmk_s2s_last_logits")
            else:
                native.check(L.mmk_s2s_step(h, B, ptr(x), x.stride(0), x.stride(1), ptr(y), y.stride(0), y.stride(1), s), "mmk_s2s_step")
                plan.generate(data, P, n)
            self.blocks += 1 + n // self.hop
        else:
            x, y = data[:, P - self.rf:P], self.step_y
            native.check(L.mmk_tr_step(h, B, ptr(x), x.stride(0), x.stride(1), ptr(y), y.stride(0), None, None, s), "mmk_tr_step")
            plan.generate(data, P, n, self.temp, self.uni)
            native.check(L.mmk_tr_last_logits(h, B, ptr(self.logits), self.logits.stride(0), s), "mmk_tr_last_logits")

    def results(self):
        out = dict(history=self.data.clone().cpu())
        for k, t in (("last_logits", self.logits), ("step", self.step_y)):
            if t is not None:
                out[k] = t.clone().cpu()
        return out

    def ran(self):
        return True if self.pc.network == "tr" else bool(self.ref.ran(self.plan, self.blocks))

    def run_default(self, which):
        self.place(which)
        self.reset()
        self.drive()
        torch.cuda.synchronize()
        assert self.ran(), (self.pc.id, "the plan took another kernel")
        return self.results()

    def sync_status(self):
        if self.plan._has_sync_status:
            self.plan.sync_status()


@pytest.mark.parametrize("pc", S.PLAN_CASES, ids=[pc.id for pc in S.PLAN_CASES])
def test_plan_behind_a_busy_stream(device, monkeypatch, pc):
    """one case per step kernel (net_refs / transformer_refs: the smallest), blocks below the graph threshold so that nothing is captured
    anew - and one launch-path WaveNet block of 2 kGraphSteps + 3 steps replayed from the same buffers (the same key)"""
    run = PlanRun(pc, device, monkeypatch)
    want = run.run_default("real")
    again = run.run_default("real")
    assert not S.differs(want, again), (pc.id, "two default-stream runs disagree", _describe(want, again))
    stale = run.run_default("stale")
    assert S.differs(want, stale), (pc.id, "the stale prompt gives the real prompt's bits: the case proves nothing")
    run.sync_status()
    side = S.side_stream(device)
    run.place("stale")
    with torch.cuda.stream(side):
        run.reset()
    torch.cuda.synchronize()
    S.delay(side, S.DELAY_MS)
    with torch.cuda.stream(side):
        run.late_copy()
        run.drive()
        busy = not side.query()
    side.synchronize()
    torch.cuda.synchronize()
    got = run.results()
    print(f"[streams] plan {pc.id}: {run.n} steps, busy after the plan's calls: {busy}")
    assert run.ran(), (pc.id, "the plan took another kernel on the side stream")
    assert not S.differs(want, got), (pc.id, "behind a late prompt on a side stream the outputs differ from the default-stream run", _describe(want, got))
    assert busy, (pc.id, "one of the plan's calls waited for the stream")
    with torch.cuda.stream(side):
        run.sync_status()


@pytest.mark.parametrize("pc", S.ERROR_WORD_CASES, ids=[pc.id for pc in S.ERROR_WORD_CASES])
def test_error_word_across_streams(device, monkeypatch, pc):
    """on a side stream: the injected word is reported once, the second look is clean, and a generation enqueued right behind it on the
    same stream gives the default-stream bits and leaves the word clean - a clear of the word that is not ordered on the caller's stream
    (the null-stream hipMemset this once was) could land in that generation"""
    run = PlanRun(pc, device, monkeypatch)
    want = run.run_default("real")
    run.sync_status()
    side = S.side_stream(device)
    run.place("real")
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        run.plan.inject_sync_error()
        with pytest.raises(native.NativeError):
            run.plan.sync_status()
        run.plan.sync_status()
        run.reset()
        run.drive()
    side.synchronize()
    torch.cuda.synchronize()
    got = run.results()
    assert run.ran()
    assert not S.differs(want, got), (pc.id, _describe(want, got))
    with torch.cuda.stream(side):
        run.plan.sync_status()
