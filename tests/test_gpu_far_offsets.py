"""Every strided entry point with its rows more than 4 GiB apart (tests/far_cases.py: the canvas, the layouts, the table, the limits).

Per case, layout and alignment class: the inputs go into their far slots of a 10.1 GiB canvas of NaN, the entry point is called through
the C ABI with the far strides (twice: the same bits), the outputs are copied out, the fill is put back over every slot and the WHOLE
canvas, lead-in included, is scanned for a word that is not fill.  The same call in a buffer of a few kilobytes with the same shapes,
base residues and stride residues (the near twin) must give the same bits: a condition, not a tolerance.  Where tests/f64_bounds.py or
the family's *_refs module has a bound that takes the case's inputs (FarCase.bound; tests/far_cases.py names the families that have none)
the far outputs are held to it as well, and the worst error / bound is printed.

The first test shows on a torch row copy that the checker sees a byte offset narrowed to int32: as a read (other bits than the twin) and
as a write (a foreign word in the lead-in).
"""
import math
import time

import pytest
import torch

from mimikit_amd import native
from tests import f64_bounds as B
from tests import far_cases as F
from tests import net_refs as R
from tests import stream_cases as S
from tests.plan_driver import switch as _switch

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)
NAN = float("nan")
_T0 = time.perf_counter()


@pytest.fixture(scope="module")
def canvas(device):
    free, total = torch.cuda.mem_get_info(device)
    need = F.CANVAS * F.WORD + 2 ** 30
    if free < need:
        pytest.skip(f"the far-offset canvas needs {need / 2 ** 30:.1f} GiB of free device memory (10.1 GiB and 1 GiB beside it); "
                    f"torch.cuda.mem_get_info reports {free / 2 ** 30:.1f} GiB free of {total / 2 ** 30:.1f}")
    buf = torch.empty(F.CANVAS, dtype=torch.float32, device=device)
    buf.fill_(NAN)
    torch.cuda.synchronize()
    assert buf.data_ptr() % 256 == 0
    yield buf
    del buf
    torch.cuda.empty_cache()
    print(f"[far] module wall time {time.perf_counter() - _T0:.1f} s")


def first_foreign(buf):
    """the offset of the first word of an fp32 buffer that is not the fill pattern, or None; chunks of at most 2^28 words"""
    chunks = range(0, buf.numel(), F.SCAN_CHUNK)
    flags = torch.stack([(buf[c:c + F.SCAN_CHUNK].view(torch.int32) != F.NAN_BITS).any() for c in chunks]).cpu()
    if not bool(flags.any()):
        return None
    c = int(flags.nonzero()[0]) * F.SCAN_CHUNK
    return c + int((buf[c:c + F.SCAN_CHUNK].view(torch.int32) != F.NAN_BITS).nonzero()[0])


def assert_clean(buf, what):
    off = first_foreign(buf)
    assert off is None, (f"{what}: word {off} of the buffer ({off * F.WORD} bytes in; the field begins at word {F.LEAD}) is not fill although every "
                         f"slot of the case was filled again: written through a wrong offset")


def assert_same_bits(far, near, what):
    for k in far:
        assert S.same_bits(far[k], near[k]), (f"{what} {k}: {int((far[k] != near[k]).sum())} of {far[k].numel()} elements differ from the near twin's "
                                              f"(a NaN counts: the far rows were not what was read or written)")


def view_of(buf, p, dtype):
    """the operand as the entry point sees it: a strided view whose data_ptr is the base"""
    flat = buf.view(dtype)
    if p.levels == 2:
        return torch.as_strided(flat, (p.B, p.R, p.K), (p.s0, p.s1, 1), p.off // p.ew)
    return torch.as_strided(flat, (p.R, p.K), (p.s1, 1), p.off // p.ew)


def words_of(buf, p):
    """the same rows as words of the fp32 buffer (to put the fill back)"""
    return torch.as_strided(buf, (p.B, p.R, p.K * p.ew), (p.s0 * p.ew, p.s1 * p.ew, 1), p.off)


def twin_buffer(words, device):
    buf = torch.full((words + words % 2,), NAN, dtype=torch.float32, device=device)
    assert buf.data_ptr() % 256 == 0
    return buf


# ====================================================================================================================== the harness itself
def _row_offsets(p, narrowed):
    """word offsets of the rows of a one-level operand from the buffer's start, right or through a byte offset narrowed to int32"""
    out = []
    for i in range(p.R):
        b = i * p.s1 * p.ew * F.WORD
        out.append(p.off + (F.to_i32(b) if narrowed else b) // F.WORD)
    return out


def _torch_row_copy(buf, src, dst, rows, narrow_read=False, narrow_write=False):
    """the 'kernel' of the self-test: dst row i = src row i, rows addressed by offsets computed here"""
    device = buf.device
    cols = torch.arange(src.K, device=device)
    rd = torch.tensor(_row_offsets(src, narrow_read), device=device)[:, None] + cols
    wr = torch.tensor(_row_offsets(dst, narrow_write), device=device)[:, None] + cols
    assert int(rd.min()) >= 0 and int(wr.min()) >= 0 and int(rd.max()) < buf.numel() and int(wr.max()) < buf.numel()      # the lead-in's purpose
    view_of(buf, src, torch.float32).copy_(rows)
    buf[wr.reshape(-1)] = buf[rd.reshape(-1)]
    torch.cuda.synchronize()
    got = dict(dst=view_of(buf, dst, torch.float32).clone().cpu())
    for p in (src, dst):
        words_of(buf, p).fill_(NAN)
    return got, wr


@pytest.mark.parametrize("mark", ["mid", "far"])
def test_the_checker_sees_a_narrowed_read_and_a_narrowed_write(canvas, device, mark):
    """torch operations only.  The correct copy passes; a read through a byte offset narrowed to int32 returns fill and fails the bit
    comparison; a write through one lands outside the slots (below the base, in the lead-in, for the row past 2^31 bytes) and fails the scan"""
    lay = F.build_layout([("src", 1, 1, 1, 3, 33), ("dst", 1, 1, 1, 3, 33)], "rows", mark, 0)
    rows = S.uni(S.gen(3), 3, 33).to(device)
    twin = twin_buffer(lay.twin_words, device)
    near, _ = _torch_row_copy(twin, *lay.twin, rows)
    assert torch.equal(near["dst"], rows.cpu())
    assert_clean(twin, "near twin")
    far, _ = _torch_row_copy(canvas, *lay.far, rows)
    assert_same_bits(far, near, "row copy")
    assert_clean(canvas, "row copy")
    bad_read, _ = _torch_row_copy(canvas, *lay.far, rows, narrow_read=True)
    with pytest.raises(AssertionError, match="differ from the near twin"):
        assert_same_bits(bad_read, near, "row copy, narrowed read")
    assert_clean(canvas, "row copy, narrowed read")                         # (a wrong read leaves no trace: only the bits show it)
    bad_write, wr = _torch_row_copy(canvas, *lay.far, rows, narrow_write=True)
    with pytest.raises(AssertionError, match="is not fill"):
        assert_clean(canvas, "row copy, narrowed write")
    foreign = first_foreign(canvas)
    dst = lay.far[1]
    moved = [w for w, true in zip(_row_offsets(dst, True), _row_offsets(dst, False)) if w != true]
    assert moved and foreign == min(moved) and (foreign < F.LEAD) == (mark == "mid"), (foreign, moved)
    canvas[wr.reshape(-1)] = NAN                                            # (the canvas is every later test's)
    assert_clean(canvas, "after the self-test")


# ====================================================================================================================== the stateless entry points
class Runner:
    """a FarCase on the device: the dense operands, outputs (PAD words of surround), workspaces and packed constants of stream_cases.Bound;
    run(placed, buf) puts the strided operands where `placed` says, calls twice and puts the fill back"""

    def __init__(self, fc, device):
        self.fc, self.L, self.device = fc, native.lib(), device
        self.host = fc.build(0)
        self.real = {k: v.to(device) for k, v in self.host.items()}
        self.outs = fc.outs(self.L, self.host)
        self.dense_in = {k: torch.empty_like(v) for k, v in self.real.items() if k not in fc.ops}
        self.bufs, self.dense_out = {}, {}
        for k, (shape, dtype) in self.outs.items():
            if k not in fc.ops:
                n = math.prod(shape)
                self.bufs[k] = torch.empty(n + 2 * S.PAD, dtype=dtype, device=device)
                self.dense_out[k] = self.bufs[k][S.PAD:S.PAD + n].view(shape)
        case = fc.case
        self.work = {k: torch.zeros(max(int(b), 16), dtype=torch.uint8, device=device) for k, b in (case.work(self.L, self.host) if case.work else {}).items()}
        self.const = {k: torch.zeros(shape, dtype=dtype, device=device) for k, (shape, dtype) in (case.const(self.L, self.host) if case.const else {}).items()}
        if case.setup:
            rc = case.setup(self.L, {**self.real, **self.const}, native.stream_ptr(device))
            assert rc == 0, (fc.id, "setup", rc, self.L.mmk_last_error())
        torch.cuda.synchronize()

    def dtype(self, name):
        return self.host[name].dtype if name in self.host else self.outs[name][1]

    def run(self, placed, buf, what):
        """-> (return code, outputs on the host in the shapes of the case's `outs`)"""
        views = {p.name: view_of(buf, p, self.dtype(p.name)) for p in placed}
        got, rc = [], 0
        for _ in range(2):
            for p in placed:                            # (a second call that wrote nothing must not show the first call's outputs)
                words_of(buf, p).fill_(NAN)
            for k, v in self.real.items():
                (views[k] if k in views else self.dense_in[k]).copy_(v.reshape(views[k].shape) if k in views else v)
            for b in self.bufs.values():
                b.fill_(S._FILL[b.dtype])
            for w in self.work.values():
                w.zero_()
            rc = self.fc.call(self.L, {**self.dense_in, **self.dense_out, **self.work, **self.const, **views}, native.stream_ptr(self.device))
            torch.cuda.synchronize()
            if rc != 0:
                break
            got.append({k: (views[k] if k in views else self.dense_out[k]).clone().reshape(shape).cpu() for k, (shape, _) in self.outs.items()})
        for p in placed:
            words_of(buf, p).fill_(NAN)
        if rc != 0:
            return rc, None
        assert not S.differs(got[0], got[1]), f"{what}: two calls disagree"
        for k, b in self.bufs.items():
            n = b.numel() - 2 * S.PAD
            edge = torch.cat([b[:S.PAD], b[S.PAD + n:]]).cpu()
            ok = torch.isnan(edge).all() if b.dtype.is_floating_point else (edge == S._FILL[b.dtype]).all()
            assert bool(ok), f"{what} {k}: written outside the dense output"
        return 0, got[0]


@pytest.mark.parametrize("fc", F.FAR_CASES, ids=[c.id for c in F.FAR_CASES])
def test_far_strides_give_the_near_twin_bits_and_touch_nothing_else(canvas, device, fc):
    runner = Runner(fc, device)
    bounds = fc.bound(runner.host) if fc.bound else {}
    worst = 0.0
    for lay in fc.layouts(runner.L):
        what = f"{fc.id} {lay.id}"
        twin = twin_buffer(lay.twin_words, device)
        rc, near = runner.run(lay.twin, twin, what + " near twin")
        assert_clean(twin, what + " near twin")
        if lay.cls == 1 and fc.odd == "refused":
            assert rc == -3, (what, "the table says this entry refuses bases 4 bytes in and odd strides", rc)
            rc, _ = runner.run(lay.far, canvas, what)
            assert rc == -3, (what, rc)
            assert_clean(canvas, what + " (refused)")
            continue
        assert rc == 0, (what, "near twin", rc, runner.L.mmk_last_error())
        rc, far = runner.run(lay.far, canvas, what)
        assert rc == 0, (what, rc, runner.L.mmk_last_error())
        assert_clean(canvas, what)
        assert_same_bits(far, near, what)
        for k, (want, bound) in bounds.items():
            B.check_bound(far[k], want, bound, f"{what} {k}")
            worst = max(worst, float(((far[k].double() - want).abs() / bound.clamp_min(1e-300)).max()))
    if bounds:
        print(f"{fc.id} far strides: worst error / bound {worst:.3f}")
    else:
        print(f"{fc.id} far strides: worst error / bound 0.000 (the near twin's bits in {len(fc.layouts(runner.L))} layouts)")


# ====================================================================================================================== the plans
def _strided_like(buf, p, shape, dtype):
    """the operand `p` as a view of `buf` with the dense tensor's shape: the far strides in front, the rest contiguous"""
    lead = (p.s0, p.s1) if p.levels == 2 else (p.s1,)
    rest = torch.empty(shape, dtype=dtype, device="meta").stride()[len(lead):]
    return torch.as_strided(buf.view(dtype), tuple(shape), lead + tuple(rest), p.off // p.ew)


def _drive_tr(run):
    """test_gpu_streams.PlanRun.drive for the transformer through the C ABI alone: native's generate refuses a class tensor whose time
    stride is not 1, the entry points take one"""
    L, h, B, P, n, data, y, s = run.L, run.plan.handle, run.B, run.P, run.n, run.data, run.step_y, native.stream_ptr(run.device)
    x = data[:, P - run.rf:P]
    native.check(L.mmk_tr_step(h, B, x.data_ptr(), x.stride(0), x.stride(1), y.data_ptr(), y.stride(0), None, None, s), "mmk_tr_step")
    native.check(L.mmk_tr_generate(h, B, data.data_ptr(), data.stride(0), data.stride(1), P, n, native.ptr(run.temp), native.ptr(run.uni), s), "mmk_tr_generate")
    if run.logits is not None:
        native.check(L.mmk_tr_last_logits(h, B, run.logits.data_ptr(), run.logits.stride(0), s), "mmk_tr_last_logits")


class TrFramesRun:
    """what _plan_run uses of test_gpu_streams.PlanRun, for a transformer of frames (PlanRun's transformer is the class one)"""

    def __init__(self, pc, device, monkeypatch):
        from tests import transformer_refs as TR
        for k in [k for k in native.PLAN_TUNING if k.startswith("MMK_")]:
            monkeypatch.delitem(native.PLAN_TUNING, k)
        self.pc, self.device, self.L, ref = pc, device, native.lib(), S.plan_ref(pc)
        self.net = TR.build_case(ref, device)
        prompt = ref.inputs()
        self.B, self.P, self.rf, self.n = ref.clips, ref.prompt, ref.rf, F.plan_steps(pc)
        self.prompt = prompt.to(device)
        self.data = torch.cat([prompt, torch.zeros(self.B, self.n, prompt.shape[2])], 1).to(device)
        self.step_y = torch.empty(self.B, prompt.shape[2], device=device)
        self.conds, self.temp, self.uni, self.logits = (), None, None, None
        self.net._ensure_plan(self.B, refresh_weights=True)
        self.plan = self.net._plan
        assert self.plan.cfg.in_kind == 1 and self.plan.cfg.head_kind == 1
        torch.cuda.synchronize()

    def place(self, which):
        self.data[:, :self.P].copy_(self.prompt)
        self.data[:, self.P:].zero_()
        self.step_y.fill_(-5)

    def reset(self):
        pass

    def sync_status(self):
        pass

    def ran(self):
        return True

    def results(self):
        return dict(history=self.data.clone().cpu(), step=self.step_y.clone().cpu())


def _plan_run(run, placed, buf, tensors, what):
    """the plan's calls of test_gpu_streams.PlanRun on operands that are views of `buf`: twice (the same bits), then the fill goes back"""
    views = {p.name: _strided_like(buf, p, *tensors[p.name]) for p in placed}
    run.data = views["data"]
    run.conds = tuple(views[f"cond{j}"] for j in range(len(run.conds)))
    if "step_y" in views:
        run.step_y = views["step_y"]
    if "logits" in views:
        run.logits = views["logits"]
    got = []
    for _ in range(2):
        run.place("real")
        run.reset()
        _drive_tr(run) if run.pc.network == "tr" else run.drive()
        torch.cuda.synchronize()
        run.sync_status()
        assert run.ran(), (what, "the plan took another kernel")
        got.append(run.results())
    for p in placed:
        words_of(buf, p).fill_(NAN)
    assert not S.differs(got[0], got[1]), f"{what}: two runs disagree"
    return got[0]


@pytest.mark.parametrize("pc", F.PLAN_CASES, ids=[pc.id for pc in F.PLAN_CASES])
def test_plan_with_far_strides(canvas, device, monkeypatch, pc):
    """the plan's entry points through native's plan classes (which pass tensor.stride()) on far-strided views of the canvas: warm-up,
    a generate block (below the graph threshold, and one WaveNet block above it), the step calls of Seq2Seq and the transformer, greedy
    and with the same uniforms, and last_logits into rows a far leading dimension apart; history, step output and logits have the
    near twin's bits, and nothing else is written"""
    from tests.test_gpu_streams import PlanRun
    run = (TrFramesRun if F.plan_ops(pc) is F.PLAN_OPS["tr frames"] else PlanRun)(pc, device, monkeypatch)
    cols = run.logits.shape[1] if run.logits is not None else F.LOGIT_COLS
    tensors = F.plan_tensors(pc, cols)
    assert tuple(run.data.shape) == tensors["data"][0] and run.n == F.plan_steps(pc)
    assert len(run.conds) == len(tensors) - 1 - ("step_y" in tensors) - ("logits" in tensors) and ("logits" in tensors) == (run.logits is not None)
    if run.logits is not None:
        assert (tuple(run.logits.shape), run.logits.dtype) == tensors["logits"]
    if "step_y" in tensors:
        assert (tuple(run.step_y.shape), run.step_y.dtype) == tensors["step_y"]
    layouts = F.plan_layouts(pc, cols)
    for lay in layouts:
        what = f"plan {pc.id} {lay.id}"
        assert not F.problems(lay.far, F.CANVAS), what                  # (placed with the plan's own logits columns: checked here)
        twin = twin_buffer(lay.twin_words, device)
        near = _plan_run(run, lay.twin, twin, tensors, what + " near twin")
        assert_clean(twin, what + " near twin")
        far = _plan_run(run, lay.far, canvas, tensors, what)
        assert_clean(canvas, what)
        assert_same_bits(far, near, what)
    print(f"plan {pc.id} far strides: worst error / bound 0.000 (the near twin's bits in {len(layouts)} layouts: {', '.join(near)})")


# ====================================================================================================================== the Seq2Seq plan
S2S_CASE = "resident-128-8-16-2layers"          # 16 clips x hop 8 = 128 rows, model_dim 128, one input segment of 65 bins: csrc/s2s_plan.hip's
#                                                 conditions for reading the caller's frames in place (lstm_seq_supported, lstm_inproj_supported)
S2S_FRAME_STRIDE = 68                           # > 65 bins, a multiple of 4


def _s2s_run(plan, case, buf, base, bs, prompt, what):
    """the case's n frames generated into a (clips, P + n, 65) view of `buf` whose clips are `bs` floats apart, then the first step once more
    through mmk_s2s_step into a y with the same far clip stride -> (history on the host, that y)"""
    M, P, n, hop, fs = case.clips, case.P, case.n, case.hop, S2S_FRAME_STRIDE
    frames = torch.as_strided(buf, (M, P + n, 65), (bs, fs, 1), base)
    ybase = base + F.roundup((P + n) * fs, 64) + 2 ** 15
    y = torch.as_strided(buf, (M, hop, 65), (bs, fs, 1), ybase)
    assert ybase + (hop - 1) * fs + 65 < base + bs or M == 1, what       # y's clips lie between the frames' clips
    frames[:, :P].copy_(prompt)
    before = plan.resident_launches()
    plan.generate(frames, P, n)
    plan.sync_status()
    assert plan.resident_launches() > before, (what, "the resident bi-LSTM was not taken: the input projection in place is not reachable")
    native.check(plan._lib.mmk_s2s_step(plan.handle, M, frames.data_ptr(), bs, fs, y.data_ptr(), bs, fs, native.stream_ptr(plan.device)), "mmk_s2s_step")
    plan.sync_status()
    hist, step = frames.clone().cpu(), y.clone().cpu()
    frames.fill_(NAN)
    y.fill_(NAN)
    assert S.same_bits(step, hist[:, P:P + hop]), f"{what}: mmk_s2s_step into a far y differs from the first step mmk_s2s_generate wrote"
    return hist


def test_s2s_frames_below_and_beyond_the_input_projection_limit(canvas, device, monkeypatch):
    """csrc/s2s_plan.hip reads the caller's frames in place through a buffer resource (csrc/lstm_inproj.hip: an `int` byte offset) while
    they span less than 2^31 bytes and gathers them first beyond.  Three spans of the same 16 clips: just below the limit (must take the
    twin's path: the twin's bits), just above it and above 2^32 bytes (the gather path, which may round differently: each other's bits);
    all within the networks' float64 envelope as tests/test_gpu_networks_f64.py holds the case.  The outputs y lie far apart as well."""
    case = next(c for c in R.S2S_CASES if c.id == S2S_CASE)
    _switch(monkeypatch, case)
    net = case.make()[0].to(device)
    prompt, conds = case.inputs()
    assert not conds and prompt.shape == (case.clips, case.P, 65)
    prompt = prompt.to(device)
    net.before_generate((prompt,), None)
    plan = net._plan
    M, hop, fs = case.clips, case.hop, S2S_FRAME_STRIDE
    # csrc/s2s_plan.hip reads the frames in place when: continuous inputs of one segment, the resident bi-LSTM (lstm_seq_supported: model_dim
    # 128 .. 1024 a power of two, hop >= 2, (D / 16) ceil(M / 16 or 32) 2 workgroups on the chip), and lstm_inproj_supported (16 rows or
    # more, D a multiple of 16, 1 .. 64 chunks of 16 inputs).  The plan does not report the path; its conditions are restated here
    cfg, cus = plan.cfg, torch.cuda.get_device_properties(device).multi_processor_count
    D, rows, chunks = cfg.model_dim, M * hop, -(-cfg.in_dim // 16)
    assert cfg.in_classes <= 0 and cfg.in_dim == 65 and len(case.inputs()[1]) == 0, "frames of one input segment"
    assert D in (128, 256, 512, 1024) and hop >= 2 and (D // 16) * -(-M // (32 if M > 16 else 16)) * 2 <= cus, "lstm_seq_supported"
    assert rows >= 16 and D % 16 == 0 and 1 <= chunks <= 64, "lstm_inproj_supported"
    stride = {w: F.s2s_batch_stride(w, M, hop, 65, fs) for w in ("below", "above", "beyond")}
    spans = {w: F.s2s_span_bytes(M, hop, 65, stride[w], fs) for w in stride}
    assert spans["below"] < F.S2S_SPAN_LIMIT <= spans["above"] < 2 ** 32 < spans["beyond"], spans
    near_bs = F.roundup(2 * (case.P + case.n) * fs + 2 ** 16, 64) + stride["below"] % 64
    twin = twin_buffer(64 + M * near_bs, device)
    hist = {"near": _s2s_run(plan, case, twin, 64, near_bs, prompt, "seq2seq near twin")}
    assert_clean(twin, "seq2seq near twin")
    for w in stride:
        hist[w] = _s2s_run(plan, case, canvas, F.LEAD, stride[w], prompt, f"seq2seq {w} ({spans[w]} bytes)")
        assert_clean(canvas, f"seq2seq {w}")
    assert S.same_bits(hist["below"], hist["near"]), "the span just below 2^31 bytes takes the near twin's path and must give its bits"
    assert S.same_bits(hist["above"], hist["beyond"]), "the spans above 2^31 and above 2^32 bytes both gather the frames first: the same bits"
    print(f"[far] seq2seq {case.id}: spans {spans}; the gather path's bits {'differ from' if S.differs(dict(a=hist['below']), dict(a=hist['above'])) else 'equal'} "
          f"the in-place path's")
    rows = case.rows()
    for w in ("below", "above"):
        env = R.envelope(hist[w], case, ())
        R64, E = env.R64[:, rows], env.E[:, rows]
        tol_max, tol_rms = R.tolerance(E)
        r_max, r_rms = R.ratios(hist[w][:, case.P:], R64, E)
        print(f"[far] seq2seq {case.id} {w}: max|dev - R64| / max(E) = {r_max:.2f}, rms(dev - R64) / rms(E) = {r_rms:.2f} (the margin allows {R.FACTOR:g})")
        R.check_outputs(hist[w][:, case.P:], R64, tol_max, tol_rms, f"seq2seq {case.id} {w}")
