"""The capture rule of include/mmk.h (conventions: streams) as two tables and a method, shared by tests/test_graph_cases.py (no GPU) and
tests/test_gpu_graphs.py.  Nothing here touches the GPU at import time.

The table of the C ABI, CAPTURE: one entry per exported function whose prototype takes an `mmk_stream_t`, over the seven headers under
include/, under exactly one of
  CAPTURED      a call can be recorded into a graph on its stream (global capture mode) and replayed: the cases below hold it to the bits of
                the eager call, on other inputs than the recorded ones and on the workspace the previous replay left;
  NOT_CAPTURED  with the reason: the header's words or the source line that waits (the lines stream_cases.ENTRY_POINTS quotes), or - for
                the plans' calls - what the code does.
A CAPTURED entry whose `unless` is set cannot be captured in the stated circumstance (the first spectral call of a process, which builds
its tables and waits); the tests stay outside it by calling eagerly first.

The cases are stream_cases.CASES and the STREAM_CASES of the families' own test files, each imported from where it lives, and three that
live here (EXTRA_CASES): the two NMF half-sweeps, which had no case yet, and mmk_gla_f32 on its general path (n_fft = 256), whose first
step is a device-to-device copy.

The table of the Python layer, FUNCTIONALS: every public Functional of mimikit_amd.features.functionals and the functions of
mimikit_amd.extract a caller puts in front of a plan, under the same two rules; a CAPTURED one has a FunctionalCase: how to build it, the
shape and kind of its input.

The method, `captured(bound, stream)`: the eager bits of the real and the stale draw on the default stream (the warm-up: code objects,
function attributes, lazy tables); ONE call recorded with torch.cuda.graph on `stream` in global capture mode while the stale input is in
place - one stream, no fork or join, so the graph is a chain; the outputs still hold their fill pattern afterwards (a capture runs
nothing: a written output is a launch that left the capturing stream); replay A on the real input and a zeroed workspace, replay B on the
stale input and the workspace as A left it, replay A again on the workspace as B left it - each the eager bits of its draw, nothing
written around the outputs.  A value the host read from the device and folded into a launch is frozen at its capture-time (stale) value
and shows in replay A; a counter, flag or accumulator that is expected zero shows in replay B.
"""
import ctypes as C
import inspect
import re

import numpy as np
import torch

from mimikit_amd import native
from tests import stream_cases as S

HEADERS = ("mmk.h", "mmk_factor_analysis.h", "mmk_kmeans.h", "mmk_nmf.h", "mmk_nn_filter.h", "mmk_samplify.h", "mmk_spec_filter.h")


# ====================================================================================================================== the C ABI's table
class Rule:
    def __init__(self, rule, reason=None, unless=None):
        assert rule in ("CAPTURED", "NOT_CAPTURED")
        assert rule == "CAPTURED" or reason, "a NOT_CAPTURED entry says why"
        self.rule, self.reason, self.unless = rule, reason, unless


def _yes(unless=None):
    return Rule("CAPTURED", unless=unless)


def _no(reason):
    return Rule("NOT_CAPTURED", reason)


def _waits(name):
    e = S.ENTRY_POINTS[name]
    return _no(f"waits for its stream: {e.where} ({e.why})")


_FIRST = S._FIRST + ": a capture must not be the first spectral call"
_PLAN = ("a plan's call: it works on the plan's own state on the device (workspace, position counter, rings, error word) and on the host "
         "(the graph cache `gc` with its key, the last mode), which a replay would advance behind the plan's back")
_PLAN_GRAPH = (_PLAN + "; from 2 kGraphSteps = 16 steps on it begins a capture of its own on the plan's cap_stream "
               "(hipStreamBeginCapture(p->cap_stream, hipStreamCaptureModeThreadLocal), {}) and replays it with hipGraphLaunch on `stream`, and "
               "a new key waits for `stream` first")
_PLAN_STEP = _PLAN + " ({}: every step reads and leaves the recurrent state in the plan's workspace)"
_PLAN_LOGITS = _PLAN + " ({}: a copy out of the plan's workspace, meaningful only behind that plan's last step)"

CAPTURE = {
    "mmk_fingerprint_u32": _yes(),
    "mmk_fingerprint_buffers_u32": _yes(),
    "mmk_mulaw_compress_f32_i64": _yes(),
    "mmk_mulaw_expand_i64_f32": _yes(),
    "mmk_resample_f32": _yes(),
    "mmk_lfilter1_f32": _yes(),
    "mmk_row_normalize_f32": _yes(),
    "mmk_inv_row_norm_f32": _yes(),
    "mmk_cosine_cost_f32": _yes(),
    "mmk_dtw_subseq_f32": _yes(),
    "mmk_nn_cosine_f32": _yes(),
    "mmk_cum_entropy_i64": _yes(),
    "mmk_nn_cosine_self_f32": _yes(),
    "mmk_nn_components_i64": _yes(),
    "mmk_segment_mean_f32": _yes(),
    "mmk_nn_topk_f32": _yes(),
    "mmk_half_neg_sqnorm_f32": _yes(),
    "mmk_edge_components_i64": _waits("mmk_edge_components_i64"),
    "mmk_novelty_f32": _yes(),
    "mmk_novelty_finish_f32": _yes(),
    "mmk_pick_peaks_f32": _yes(),
    "mmk_pca_colstats_f64": _yes(),
    "mmk_pca_cov_f64": _yes(),
    "mmk_pca_eig_f64": _waits("mmk_pca_eig_f64"),
    "mmk_pca_project_f32": _yes(),
    "mmk_stft_mag_f32": _yes(_FIRST),
    "mmk_stft_f32": _yes(_FIRST),
    "mmk_stft_energy_f32": _yes(_FIRST),
    "mmk_interp1d_f32": _yes(),
    "mmk_derivative_f32": _yes(),
    "mmk_hpss_f32": _yes(),
    "mmk_melbank_f32": _yes(),
    "mmk_stft_mel_f32": _yes(_FIRST),
    "mmk_istft_f32": _yes(_FIRST),
    "mmk_gla_f32": _yes(_FIRST),
    "mmk_pack_weight_f32": _yes(),
    "mmk_linear_f32": _yes(),
    "mmk_gemm_f32": _yes(),
    "mmk_gemm_bias_act_f32": _yes(),
    "mmk_skinny_linear_f32": _yes(),
    "mmk_tr_attention_f32": _yes(),
    "mmk_tr_add_ln_f32": _yes(),
    "mmk_categorical_sample_f32_i64": _yes(),
    # ---- WaveNet plans
    "mmk_wavenet_commit": _waits("mmk_wavenet_commit"),
    "mmk_wavenet_warmup": _no(_PLAN_GRAPH.format("csrc/wavenet_plan.hip:1258, run_steps")),
    "mmk_wavenet_generate": _no(_PLAN_GRAPH.format("csrc/wavenet_plan.hip:1258, run_steps")),
    "mmk_wavenet_last_logits": _no(_PLAN_LOGITS.format("csrc/wavenet_plan.hip:1337")),
    "mmk_wavenet_last_logits_of": _no(_PLAN_LOGITS.format("csrc/wavenet_plan.hip:1351")),
    "mmk_wavenet_profile_steps": _no("a measurement aid of bench.py: it records an event around every launch and waits for them "
                                     "(include/mmk.h: `mmk_wavenet_profile_steps: waits for its events`)"),
    "mmk_wavenet_sync_status": _waits("mmk_wavenet_sync_status"),
    "mmk_wavenet_inject_sync_error": _waits("mmk_wavenet_inject_sync_error"),
    # ---- SampleRNN plans
    "mmk_srnn_commit": _waits("mmk_srnn_commit"),
    "mmk_srnn_reset": _waits("mmk_srnn_reset"),
    "mmk_srnn_warmup": _no(_PLAN_GRAPH.format("csrc/srnn_plan.hip:864; SampleRNN: from two periods of frame_sizes[0] on")),
    "mmk_srnn_warmup_multi": _no(_PLAN_GRAPH.format("csrc/srnn_plan.hip:864; SampleRNN: from two periods of frame_sizes[0] on")),
    "mmk_srnn_generate": _no(_PLAN_GRAPH.format("csrc/srnn_plan.hip:864; SampleRNN: from two periods of frame_sizes[0] on")),
    "mmk_srnn_generate_multi": _no(_PLAN_GRAPH.format("csrc/srnn_plan.hip:864; SampleRNN: from two periods of frame_sizes[0] on")),
    "mmk_srnn_last_logits": _no(_PLAN_LOGITS.format("csrc/srnn_plan.hip:1104")),
    "mmk_srnn_last_logits_of": _no(_PLAN_LOGITS.format("csrc/srnn_plan.hip:1141")),
    "mmk_srnn_sync_status": _waits("mmk_srnn_sync_status"),
    "mmk_srnn_inject_sync_error": _waits("mmk_srnn_inject_sync_error"),
    # ---- Seq2Seq plans
    "mmk_s2s_commit": _waits("mmk_s2s_commit"),
    "mmk_s2s_step": _no(_PLAN_STEP.format("csrc/s2s_plan.hip:605, s2s_step")),
    "mmk_s2s_generate": _no(_PLAN_STEP.format("csrc/s2s_plan.hip:635, a host loop of s2s_step")),
    "mmk_s2s_step_classes": _no(_PLAN_STEP.format("csrc/s2s_plan.hip:616, s2s_step")),
    "mmk_s2s_generate_classes": _no(_PLAN_STEP.format("csrc/s2s_plan.hip:654, a host loop of s2s_step")),
    "mmk_s2s_last_logits": _no(_PLAN_LOGITS.format("csrc/s2s_plan.hip:627")),
    "mmk_s2s_sync_status": _waits("mmk_s2s_sync_status"),
    "mmk_s2s_inject_sync_error": _waits("mmk_s2s_inject_sync_error"),
    # ---- SimpleTransformer plans
    "mmk_tr_commit": _waits("mmk_tr_commit"),
    "mmk_tr_step": _no(_PLAN_STEP.format("csrc/transformer_plan.hip:417: the key / value cache and the position")),
    "mmk_tr_generate": _no(_PLAN_GRAPH.format("csrc/transformer_plan.hip:378")),
    "mmk_tr_last_logits": _no(_PLAN_LOGITS.format("csrc/transformer_plan.hip:445")),
    # ---- include/mmk_kmeans.h
    "mmk_kmeans_assign_f32": _yes(),
    "mmk_kmeans_label_sums_f64": _yes(),
    "mmk_kmeans_pp_step_f64": _yes(),
    # ---- include/mmk_nmf.h
    "mmk_nmf_start_f64": _no("include/mmk_nmf.h: `mmk_nmf_start_f64 waits for `stream` (inside mmk_pca_eig_f64, and once more to read the "
                             "smallest entry and the eigenvalues)` - csrc/nmf.hip:596: MMK_HIP(hipStreamSynchronize(st));"),
    "mmk_nmf_w_half_f64": _yes(),
    "mmk_nmf_h_half_f64": _yes(),
    "mmk_nmf_solve_f64": _no("include/mmk_nmf.h: `mmk_nmf_solve_f64 waits every `poll` iterations to read its convergence flag` - "
                             "csrc/nmf.hip:698: MMK_HIP(hipStreamSynchronize(st));"),
    # ---- include/mmk_factor_analysis.h
    "mmk_fa_fit_f64": _no("include/mmk_factor_analysis.h: `mmk_fa_fit_f64 waits for `stream` every MMK_FA_POLL inner iterations to read its "
                          "state; it cannot be captured into a graph` - csrc/factor_analysis.hip:338: MMK_HIP(hipStreamSynchronize(st));"),
    "mmk_fa_transform_matrix_f64": _yes(),
    # ---- include/mmk_nn_filter.h, include/mmk_spec_filter.h, include/mmk_samplify.h
    "mmk_nn_aggregate_f32": _yes(),
    "mmk_auto_convolve_f32": _yes(),
    "mmk_f0_filter_f32": _yes(),
    "mmk_spline2_coef_f64": _yes(),
    "mmk_spline2_eval_f32": _yes(),
    "mmk_periods_count_i64": _yes(),
    "mmk_periods_fill_i64": _yes(),
    "mmk_samplify_scores_f32": _yes(),
    "mmk_samplify_cuts_i64": _yes(),
}
CAPTURED = tuple(k for k, r in CAPTURE.items() if r.rule == "CAPTURED")
NOT_CAPTURED = tuple(k for k, r in CAPTURE.items() if r.rule == "NOT_CAPTURED")


def header_texts():
    return {h: (S.ROOT / "include" / h).read_text() for h in HEADERS}


def header_stream_functions(texts=None):
    """the functions of the seven headers whose prototype has an mmk_stream_t parameter (stream_cases' parser on each) -> sorted names"""
    texts = header_texts() if texts is None else texts
    return sorted(name for text in texts.values() for name in S.header_stream_functions(text))


def header_waiting_names(paragraph=None):
    """the entry points the streams paragraph of include/mmk.h lists as waiting: the names of its indented list, `mmk_{a,b}_x`-free"""
    paragraph = S.header_streams_paragraph() if paragraph is None else paragraph
    start = paragraph.index("behind a busy side stream.")
    listed = paragraph[start:paragraph.index("Two more waits depend on what came before the call.")]
    return sorted(set(re.findall(r"\bmmk_[a-z0-9_]+", listed)) - {"mmk_nmf", "mmk_factor_analysis"})


# ====================================================================================================================== the cases
NMF_HALF = "tiny"


def _half_sweep(which):
    """one half-sweep of include/mmk_nmf.h on the factors nmf_refs.sweep_inputs leaves after two iterations (exact zeros in them).  The
    updated factor is IN/OUT: the call copies its given state into the output on the call's stream first, as test_gpu_nmf.py's transform
    case does with sklearn's zeros"""
    from tests import nmf_refs as R
    f = R.FIXTURES[NMF_HALF]
    n, d, k = f["n"], f["d"], f["k"]
    moved, shape = ("w", (n, k)) if which == "w" else ("ht", (d, k))

    def build(seed):
        _, w, ht = R.sweep_inputs(NMF_HALF)
        x = R.fixture_case(NMF_HALF)["x"]
        if seed:                                                      # another valid state: the frames reversed and halved, the factors scaled
            x, w, ht = np.ascontiguousarray(x[::-1] * np.float32(0.5)), w[::-1] * 0.75, ht * 1.25
        return dict(x=torch.from_numpy(x.copy()), w0=torch.from_numpy(np.ascontiguousarray(w)), ht0=torch.from_numpy(np.ascontiguousarray(ht)))

    def call(L, a, s):
        with torch.cuda.stream(torch.cuda.ExternalStream(s) if s else torch.cuda.default_stream()):
            a[moved].copy_(a[moved + "0"], non_blocking=True)
        fn = L.mmk_nmf_w_half_f64 if which == "w" else L.mmk_nmf_h_half_f64
        given, out = (a["ht0"], a["w"]) if which == "w" else (a["w0"], a["ht"])
        return fn(S.P(a["x"]), d, n, d, k, S.P(given), S.P(out), S.P(a["violation"]), S.P(a["ws"]), a["ws"].numel(), s)

    def ref(i):
        x64, w, ht = i["x"].double().numpy(), i["w0"].numpy().copy(), i["ht0"].numpy().copy()
        (R.w_half64 if which == "w" else R.h_half64)(x64, w, ht)
        return torch.from_numpy(w if which == "w" else ht)
    return S.Case(f"mmk_nmf_{which}_half_f64", build, lambda L, i: {moved: (shape, torch.float64), "violation": ((1,), torch.float64)}, call,
                  work=lambda L, i: dict(ws=L.mmk_nmf_half_workspace_bytes(n, d, k)), ref=ref)


HALF_SWEEP_CASES = [_half_sweep("w"), _half_sweep("h")]


def _gla_general():
    """mmk_gla_f32 at n_fft = 256: the general path (stream_cases has the fused one of 1024), whose first step is a device-to-device copy
    of the initial estimates - a memcpy node in a graph, the only one a stateless entry point makes"""
    n_fft, hop, n_iter = 256, 64, 3
    bins, clips, frames = n_fft // 2 + 1, S.SPECTRAL_CLIPS, S.SPECTRAL_FRAMES

    def build(seed):
        g = S.gen(seed + n_fft)
        return dict(mag=S.uni(g, clips, frames, bins, lo=0.0), init=S.uni(g, clips, frames, bins, 2, lo=0.0))

    def call(L, a, s):
        return L.mmk_gla_f32(S.P(a["mag"]), S.P(a["init"]), clips, frames, n_fft, hop, n_iter, 0.99, S.P(a["ws"]), S.P(a["out"]), s)
    return S.Case("mmk_gla_f32", build, lambda L, i: dict(out=((clips, hop * (frames - 1)), torch.float32)), call, tag=str(n_fft),
                  work=lambda L, i: dict(ws=4 * L.mmk_gla_workspace_floats(clips, frames, n_fft, hop)))


EXTRA_CASES = HALF_SWEEP_CASES + [_gla_general()]
FAMILY_MODULES = ("test_gpu_kmeans", "test_gpu_nmf", "test_gpu_nn_filter", "test_gpu_samplify", "test_gpu_spec_filter", "test_gpu_factor_analysis")
_all_cases = None


def all_cases():
    """stream_cases.CASES, the families' STREAM_CASES (imported from where they live) and the half-sweeps - every Case there is, once"""
    global _all_cases
    if _all_cases is None:
        import importlib
        cases = list(S.CASES)
        for module in FAMILY_MODULES:
            cases += importlib.import_module(f"tests.{module}").STREAM_CASES
        _all_cases = cases + EXTRA_CASES
    return _all_cases


def captured_cases():
    """the cases whose entry point is CAPTURED.  A case that calls a second entry point on the way (periods_fill after periods_count, the
    projection behind the transform matrix) is captured with it: every such companion is CAPTURED itself (test_graph_cases.py)"""
    return [c for c in all_cases() if CAPTURE[c.entry].rule == "CAPTURED"]


# the entry points a case of another entry calls on the way: the case is captured only if these are CAPTURED too
COMPANIONS = {"mmk_periods_fill_i64": ("mmk_periods_count_i64",), "mmk_fa_transform_matrix_f64[transform]": ("mmk_pca_project_f32",)}


# ====================================================================================================================== the method
def describe(a, b):
    return {k: f"{int((a[k] != b[k]).sum())} of {a[k].numel()} differ" for k in a if not S.same_bits(a[k], b[k])}


def untouched(bound):
    """every output buffer still holds its fill pattern, surround included -> the names that do not"""
    bad = []
    for k, b in bound.bufs.items():
        host = b.cpu()
        fill = S._FILL[b.dtype]
        same = torch.isnan(host) if b.dtype.is_floating_point else host == fill
        if not bool(same.all()):
            bad.append(f"{k}: {int((~same).sum())} of {host.numel()} elements")
    return bad


def captured(bound, stream):
    """the method of the module docstring -> the records of the run (dict); raises AssertionError with the case's id on any difference"""
    cid = bound.case.id
    real = bound.run_default("real")                                               # 1: eager bits of both draws, and the warm-up
    stale = bound.run_default("stale")
    assert S.differs(real, stale), (cid, "the stale input gives the real input's bits: the case proves nothing")
    bound.fill("stale")                                                            # 2: one call recorded, the stale input in place
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=stream, capture_error_mode="global"):
        bound.call(stream.cuda_stream)
    torch.cuda.synchronize()
    bad = untouched(bound)                                                         # 3: a capture runs nothing
    assert not bad, (cid, "an output was written during the capture: a launch left the capturing stream", bad)

    def replay(which, what, want, keep_work):
        bound.fill(which, keep_work=keep_work)
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        got = bound.outputs()
        assert not S.differs(want, got), (cid, f"{what}: other bits than the eager call on the same input", describe(want, got))
        bound.check_surround(f"{cid} {what}")

    replay("real", "replay A (real input, zeroed workspace)", real, False)         # 4
    replay("stale", "replay B (stale input, the workspace as replay A left it)", stale, True)      # 5
    replay("real", "replay A again (the workspace as replay B left it)", real, True)               # 6
    return dict(case=cid, replays=3)


# ====================================================================================================================== the chains
class Chain:
    """entry points in the order a caller uses them, intermediates left on the device: build(draw) -> host inputs of draw 0 / 1 (numpy),
    alloc(L, inputs, device) -> every other buffer by name (intermediates, outputs, workspaces), reset(a): what a caller puts in place
    before every run (IN/OUT state), run(L, a, s) -> the first non-zero return code, outs: the names compared"""

    def __init__(self, name, entries, build, alloc, run, outs, reset=None):
        self.id, self.entries, self.build, self.alloc, self.run, self.outs, self.reset = name, entries, build, alloc, run, outs, reset


def _nnn_chain():
    from tests import nnn_refs as R
    batch, n, m, k = 3, 63, 65, 4             # nnn_refs' grid: three clips, one row short of the 64 a wave aligns (padded to 64), one corpus frame past 64

    def build(draw):
        x, y, _, _ = R.cost_case(batch, n, m, k)
        return dict(x=x.copy() if draw == 0 else np.ascontiguousarray(x[::-1, ::-1]), y=y.copy())

    def alloc(L, i, dev):
        f32 = dict(dtype=torch.float32, device=dev)
        return dict(rx=torch.empty(batch * n, **f32), ry=torch.empty(m, **f32), cost=torch.empty(batch, m, native.nnn_n_pad(n), **f32),
                    end_col=torch.empty(batch, dtype=torch.int64, device=dev), end_val=torch.empty(batch, **f32), last_row=torch.empty(batch, m, **f32))

    def run(L, a, s):
        return (L.mmk_inv_row_norm_f32(S.P(a["x"]), n * k, k, batch, n, k, S.P(a["rx"]), s)
                or L.mmk_inv_row_norm_f32(S.P(a["y"]), m * k, k, 1, m, k, S.P(a["ry"]), s)
                or L.mmk_cosine_cost_f32(S.P(a["x"]), n * k, k, S.P(a["rx"]), batch, n, S.P(a["y"]), k, S.P(a["ry"]), m, k, S.P(a["cost"]), s)
                or L.mmk_dtw_subseq_f32(S.P(a["cost"]), batch, n, m, S.P(a["end_col"]), S.P(a["end_val"]), S.P(a["last_row"]), s))
    return Chain("nnn", ("mmk_inv_row_norm_f32", "mmk_cosine_cost_f32", "mmk_dtw_subseq_f32"), build, alloc, run, ("cost", "end_col", "end_val", "last_row"))


def _novelty_chain():
    from tests import segment_refs as R
    T, D, halves = R.TILE + 1, 33, (1, 6, R.MAX_HALF)      # one frame past a tile of output frames
    q = len(halves)

    def build(draw):
        x = R.frames_case(T, D)
        return dict(x=x.copy() if draw == 0 else np.ascontiguousarray(x[:, ::-1]))

    def alloc(L, i, dev):
        f32 = dict(dtype=torch.float32, device=dev)
        return dict(raw=torch.empty(1, q, T, **f32), scores=torch.empty(1, q, T, **f32), dg=torch.empty(1, T, **f32),
                    picked=torch.empty(T, dtype=torch.uint8, device=dev),
                    ws_finish=torch.zeros(max(4 * L.mmk_novelty_finish_workspace_floats(1, q, T), 16), dtype=torch.uint8, device=dev),
                    ws_pick=torch.zeros(max(L.mmk_pick_peaks_workspace_bytes(T), 16), dtype=torch.uint8, device=dev))

    def run(L, a, s):
        h = (C.c_int32 * q)(*halves)
        return (L.mmk_novelty_f32(S.P(a["x"]), T * D, D, None, 1, T, D, h, q, S.P(a["raw"]), s)
                or L.mmk_novelty_finish_f32(S.P(a["raw"]), 1, q, T, S.P(a["scores"]), S.P(a["dg"]), S.P(a["ws_finish"]), a["ws_finish"].numel() // 4, s)
                or L.mmk_pick_peaks_f32(S.P(a["dg"]), T, 4, 4, 0.03, S.P(a["picked"]), S.P(a["ws_pick"]), a["ws_pick"].numel(), s))
    return Chain("novelty", ("mmk_novelty_f32", "mmk_novelty_finish_f32", "mmk_pick_peaks_f32"), build, alloc, run, ("raw", "scores", "dg", "picked"))


def _lloyd_chain():
    from tests import kmeans_refs as R
    n, d, k = 257, 33, 33                     # kmeans_refs' grid: one past two workgroups' rows, one past a chunk of bins, one past 32 centres

    def build(draw):
        x, offset, centres = R.kernel_case(n, d, k)
        x = x.copy() if draw == 0 else (x[::-1] * np.float32(0.75) + offset * np.float32(0.25)).astype(np.float32)
        return dict(x=x, offset=offset.copy(), centres=centres.copy(), shift=(-(centres.astype(np.float64) ** 2).sum(-1) / 2).astype(np.float32))

    def alloc(L, i, dev):
        f64 = dict(dtype=torch.float64, device=dev)
        return dict(labels=torch.empty(n, dtype=torch.int32, device=dev), key=torch.empty(n, dtype=torch.float32, device=dev),
                    changed=torch.empty(1, dtype=torch.int64, device=dev), sums=torch.empty(k, d, **f64),
                    counts=torch.empty(k, dtype=torch.int64, device=dev), row_d2=torch.empty(n, **f64), inertia=torch.empty(1, **f64),
                    ws=torch.zeros(max(L.mmk_kmeans_label_sums_workspace_bytes(n, d, k), 16), dtype=torch.uint8, device=dev))

    def reset(a):
        a["labels"].fill_(-1)                 # IN/OUT: the labels of the step before - none yet; `changed` is zeroed inside the chain, as lloyd does

    def run(L, a, s):
        with torch.cuda.stream(torch.cuda.ExternalStream(s) if s else torch.cuda.default_stream()):
            a["changed"].zero_()
        return (L.mmk_kmeans_assign_f32(S.P(a["x"]), d, S.P(a["offset"]), n, d, S.P(a["centres"]), d, S.P(a["shift"]), k, S.P(a["labels"]), S.P(a["key"]),
                                        S.P(a["changed"]), s)
                or L.mmk_kmeans_label_sums_f64(S.P(a["x"]), d, S.P(a["offset"]), n, d, S.P(a["labels"]), k, S.P(a["sums"]), S.P(a["counts"]), S.P(a["centres"]),
                                               d, S.P(a["row_d2"]), S.P(a["inertia"]), S.P(a["ws"]), a["ws"].numel(), s))
    return Chain("lloyd-step", ("mmk_kmeans_assign_f32", "mmk_kmeans_label_sums_f64"), build, alloc, run,
                 ("labels", "key", "changed", "sums", "counts", "row_d2", "inertia"), reset=reset)


CHAINS = [_nnn_chain(), _novelty_chain(), _lloyd_chain()]


class BoundChain:
    """a Chain on a device: the two draws, the input buffers the chain reads, every other buffer"""

    def __init__(self, chain, device):
        self.chain, self.L, self.device = chain, native.lib(), device
        self.draws = [{k: torch.from_numpy(v).to(device) for k, v in chain.build(j).items()} for j in (0, 1)]
        self.inp = {k: torch.empty_like(v) for k, v in self.draws[0].items()}
        self.rest = chain.alloc(self.L, self.draws[0], device)
        torch.cuda.synchronize()

    def place(self, draw):
        """the inputs of a draw, the outputs and intermediates poisoned - the workspaces stay as they are"""
        for k, v in self.draws[draw].items():
            self.inp[k].copy_(v)
        for k, t in self.rest.items():
            if not k.startswith("ws"):
                t.fill_(float("nan") if t.dtype.is_floating_point else 0x5A if t.dtype == torch.uint8 else -7777)
        if self.chain.reset:
            self.chain.reset(self.rest)

    def run(self, stream_ptr):
        rc = self.chain.run(self.L, {**self.inp, **self.rest}, stream_ptr)
        assert rc == 0, (self.chain.id, rc, self.L.mmk_last_error())

    def outputs(self):
        return {k: self.rest[k].clone().cpu() for k in self.chain.outs}

    def eager(self, draw):
        self.place(draw)
        for k, t in self.rest.items():
            if k.startswith("ws"):
                t.zero_()
        self.run(native.stream_ptr(self.device))
        torch.cuda.synchronize()
        return self.outputs()


def captured_chain(bc, stream):
    """the chain recorded once as one graph on draw 0, then replayed on draw 1, draw 0 and draw 1 again without touching the workspaces:
    each the bits of the same chain run eagerly on that draw"""
    want = [bc.eager(0), bc.eager(1)]
    assert S.differs(want[0], want[1]), (bc.chain.id, "the second draw gives the first draw's bits: the chain proves nothing")
    bc.place(0)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=stream, capture_error_mode="global"):
        bc.run(stream.cuda_stream)
    torch.cuda.synchronize()
    for draw in (1, 0, 1):
        bc.place(draw)
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        got = bc.outputs()
        assert not S.differs(want[draw], got), (bc.chain.id, f"replay on draw {draw} with the workspaces as the last run left them", describe(want[draw], got))


# ====================================================================================================================== the Python layer
class FunctionalCase:
    """make() -> the callable a user captures (a Functional, or a function of mimikit_amd.extract with its fixed arguments bound - made on
    the device, outside the capture, as a user holds it); draw(seed) -> the host input of that seed (another seed: another valid input
    of the same shape).  The output may be a tensor or a tuple of tensors."""

    def __init__(self, make, draw):
        self.make, self.draw = make, draw


def _signal(n, clips=2):
    return lambda seed: S.uni(S.gen(1000 + seed), clips, n)


def _mags(frames, bins, clips=None):
    shape = (frames, bins) if clips is None else (clips, frames, bins)
    return lambda seed: S.uni(S.gen(2000 + seed), *shape, lo=0.0)


def _frames(rows, bins):
    return lambda seed: S.uni(S.gen(3000 + seed), rows, bins)


F_NOT = "NOT_CAPTURED"


def _fn():
    from mimikit_amd.features import functionals as F
    return F


def _gla(device):
    """GLA with the initial phases given: its __call__ draws them with torch.rand at every call, which a replay and an eager call do not
    share, so the bits could not be compared; the launches are the same"""
    F = _fn()
    gla = F.GLA(1024, 256)
    init = torch.polar(torch.ones(2, 9, 513), S.uni(S.gen(77), 2, 9, 513, lo=-3.0, hi=3.0)).to(device)
    return lambda x: gla.torch_func(x, init=init)


def _fitted_pca(device):
    F = _fn()
    pca = F.PCA(n_components=3).fit(S._pca_x(0).to(device))          # fit waits (mmk_pca_eig_f64): outside the capture
    return pca.transform


def _nn_scorer(device):
    from mimikit_amd.extract.from_neighbors import NeighborScorer
    return NeighborScorer(S.uni(S.gen(7), 200, 33).to(device)).neighbors      # (the constructor reads a flag back: outside the capture)


def _mel_from_signal(device):
    F = _fn()
    mel, mag = F.MelSpec(n_mels=20), F.MagSpec(1024, 256)
    return lambda x: mel.from_signal(x, mag)


def _mfcc_from_signal(device):
    F = _fn()
    mfcc, mel, mag = F.MFCC(n_mfcc=7), F.MelSpec(n_mels=20), F.MagSpec(1024, 256)
    return lambda x: mfcc.from_signal(x, mag, mel)


def _compose(device):
    F = _fn()
    return F.Compose(F.Emphasis(0.9), F.MagSpec(1024, 256), F.MelSpec(n_mels=20))


def _f(name, **kw):
    return lambda device: getattr(_fn(), name)(**kw)


def _ext(module, name, **kw):
    def make(device):
        import importlib
        fn = getattr(importlib.import_module(module), name)
        return (lambda x: fn(x, **kw)) if kw else fn
    return make


_SIG = _signal(1024 + 8 * 256)              # nine frames of 1024 at hop 256, uncentred
_FIT = "fits on every call: {}"

# name -> FunctionalCase (CAPTURED) or (NOT_CAPTURED, the reason with the line quoted)
FUNCTIONALS = {
    "Functional": (F_NOT, "the abstract base: `class Functional(Config, abc.ABC)` has no torch_func of its own"),
    "Identity": FunctionalCase(lambda device: _fn().Compose(_fn().Identity(), _fn().Emphasis(0.9), _fn().Identity()), _signal(300)),      # (alone it launches nothing)
    "Compose": FunctionalCase(_compose, _SIG),
    "FileToSignal": (F_NOT, "opens a file (and raises here): `raise NotImplementedError(\"decoding audio files is dataset preparation ...\")`"),
    "RemoveDC": FunctionalCase(_f("RemoveDC"), _signal(S.LFILTER_N)),
    "Normalize": FunctionalCase(_f("Normalize", p=2), _signal(S.LFILTER_N)),
    "Emphasis": FunctionalCase(_f("Emphasis", emphasis=0.9), _signal(S.LFILTER_N)),
    "Deemphasis": FunctionalCase(_f("Deemphasis", emphasis=0.9), _signal(S.LFILTER_N)),
    "MuLawCompress": FunctionalCase(_f("MuLawCompress"), _signal(3001)),
    "MuLawExpand": FunctionalCase(_f("MuLawExpand"), lambda seed: torch.randint(0, 256, (2, 3001), generator=S.gen(4000 + seed))),
    "STFT": FunctionalCase(_f("STFT", n_fft=1024, hop_length=256), _SIG),
    "ISTFT": FunctionalCase(_f("ISTFT", n_fft=1024, hop_length=256), lambda seed: S.uni(S.gen(5000 + seed), 2, 9, 513, 2)),
    "MagSpec": FunctionalCase(_f("MagSpec", n_fft=256, hop_length=64), _signal(256 + 8 * 64)),
    "GLA": FunctionalCase(_gla, _mags(9, 513, clips=2)),
    "Resample": FunctionalCase(_f("Resample", orig_sr=2, target_sr=3), _signal(101)),
    "Envelop": FunctionalCase(_f("Envelop", n_fft=256, hop_length=64), _signal(2000)),
    "EnvelopBank": FunctionalCase(_f("EnvelopBank", n_fft=(256, 1024), hop_length=(64, 256)), _signal(3000)),
    "Interpolate": FunctionalCase(_f("Interpolate", mode="quadratic", length=900), _signal(300)),
    "Derivative": FunctionalCase(_f("Derivative", max_lag=3, normalize=True), _signal(native.DERIV_TILE + 6)),
    "PCA": (F_NOT, _FIT.format("`self.components_, self.explained_variance_, self.n_iter_ = native.pca_eig(c, k)` - mmk_pca_eig_f64 waits; the "
                               "transform of a fitted PCA is `PCA.transform` below")),
    "HarmonicSource": FunctionalCase(_f("HarmonicSource"), _mags(*S.HPSS_SHAPE[1:])),
    "PercussiveSource": FunctionalCase(_f("PercussiveSource"), _mags(*S.HPSS_SHAPE[1:])),
    "MelSpec": FunctionalCase(_f("MelSpec", n_mels=20), _mags(9, 513, clips=2)),
    "MFCC": FunctionalCase(_f("MFCC", n_mfcc=7), _mags(9, 20, clips=2)),
    "NearestNeighborFilter": FunctionalCase(_f("NearestNeighborFilter", n_neighbors=5), _frames(129, 33)),
    "NMF": (F_NOT, _FIT.format("`w, ht, _, _, _ = native.nmf_start(x, k)` and `self.n_iter_ = native.nmf_solve(...)` - both wait, and "
                               "NMF.transform solves again (`n_iter = native.nmf_solve(y, w, ...)`)")),
    "AutoConvolve": FunctionalCase(_f("AutoConvolve", window_size=3), _mags(9, 257, clips=2)),
    "F0Filter": FunctionalCase(_f("F0Filter"), _mags(9, 257, clips=2)),
    "FactorAnalysis": (F_NOT, _FIT.format("`components, noise, loglike, n_iter, converged, _ = native.fa_fit(c, n, k, self.tol, self.max_iter)` "
                                          "- mmk_fa_fit_f64 waits and `loglike[:int(n_iter.value)]` sizes a tensor by a count")),
    # ---- beside the module's classes
    "MelSpec.from_signal": FunctionalCase(_mel_from_signal, _SIG),
    "MFCC.from_signal": FunctionalCase(_mfcc_from_signal, _SIG),
    "PCA.transform": FunctionalCase(_fitted_pca, lambda seed: S._pca_x(seed)),
    "mmk.discontinuity_scores": FunctionalCase(_ext("mimikit_amd.extract.segment", "discontinuity_scores", kernel_sizes=(1, 6)),
                                               lambda seed: S.uni(S.gen(6000 + seed), S.NOVELTY_T, S.NOVELTY_D, lo=0.0)),
    "extract.nearest_neighbor": (F_NOT, "reads a flag: `return bool((t < 0).any())` (extract/from_neighbors.py: _has_negatives, for the corpus in "
                                        "NeighborScorer.__init__ and for the queries in __call__); the search itself is `NeighborScorer.neighbors` below"),
    "extract.NeighborScorer.neighbors": FunctionalCase(_nn_scorer, lambda seed: S.uni(S.gen(7000 + seed), 2, 25, 33)),
    "extract.cum_entropy": FunctionalCase(_ext("mimikit_amd.extract.from_neighbors", "cum_entropy"),
                                          lambda seed: torch.randint(0, 7, (3, 40), generator=S.gen(8000 + seed))),
}
FUNCTIONALS_CAPTURED = tuple(k for k, v in FUNCTIONALS.items() if isinstance(v, FunctionalCase))
FUNCTIONALS_NOT_CAPTURED = tuple(k for k, v in FUNCTIONALS.items() if not isinstance(v, FunctionalCase))


def public_functionals():
    """the names of mimikit_amd.features.functionals.__all__ that are Functional classes"""
    F = _fn()
    return sorted(n for n in F.__all__ if inspect.isclass(getattr(F, n)) and issubclass(getattr(F, n), F.Functional))


def _tensors(y):
    return list(y) if isinstance(y, (tuple, list)) else [y]


def captured_functional(fc, device):
    """a user's capture: a static input, one eager call (tables cached, code loaded), `y = f(x_static)` under torch.cuda.graph (global
    capture mode, torch's own side stream and pool), then the second draw copied into the static input and a replay: y is the eager
    f(second draw), bit for bit -> the number of output tensors"""
    f = fc.make(device)
    first, second = fc.draw(0).to(device), fc.draw(1).to(device)
    assert not torch.equal(first, second)
    x_static = first.clone()
    want_first = [t.clone() for t in _tensors(f(x_static))]
    want = [t.clone() for t in _tensors(f(second))]
    assert any(not S.same_bits(a, b) for a, b in zip(want_first, want)), "the second draw gives the first draw's bits: the case proves nothing"
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, capture_error_mode="global"):
        y = f(x_static)
    ys = _tensors(y)
    x_static.copy_(second)
    g.replay()
    torch.cuda.synchronize()
    for j, (got, w) in enumerate(zip(ys, want)):
        assert S.same_bits(got, w), (f"output {j}", f"{int((got != w).sum())} of {w.numel()} elements differ from the eager call on the second draw")
    x_static.copy_(first)
    g.replay()
    torch.cuda.synchronize()
    for j, (got, w) in enumerate(zip(ys, want_first)):
        assert S.same_bits(got, w), (f"output {j}", f"{int((got != w).sum())} of {w.numel()} elements differ from the eager call on the first draw")
    return len(ys)
