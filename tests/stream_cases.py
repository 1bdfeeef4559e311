"""The stream contract of include/mmk.h (conventions: streams) as a table and a method, shared by tests/test_stream_cases.py (no GPU) and
tests/test_gpu_streams.py.  Nothing here touches the GPU at import time.

The table, ENTRY_POINTS: one entry per exported function whose prototype takes an `mmk_stream_t`, under exactly one of
  ASYNC    returns without waiting for `stream` (the header's rule);
  WAITS    waits for `stream` by design - `where` quotes the source line, `why` the reason; the header's streams paragraph names each;
  NOT_RUN  not run by the stream tests, with the reason.
An ASYNC entry whose `unless` is set waits in the stated circumstance only (a graph captured anew, the first spectral call of a process);
the tests stay outside it, and the header states it.

The stateless entry points have a Case each (CASES): how to call it through the C ABI on the smallest input that still takes every launch
it can make, which buffers are inputs (`build(seed)`: tensors on the host, another seed is another draw of the same, valid, kind), which
are outputs (`outs`) and which workspace (`work`, zero-filled before every call, so that an index a mis-ordered kernel finds there is a
valid one).  The plans' entry points are driven by PLAN_CASES through native's plan classes (tests/test_gpu_streams.py).

The method: `delay(stream, ms)` keeps a stream busy with torch.cuda._sleep (cycles per ms measured once per process between two
events); `late_input(bound, stream)` puts a STALE input in place, synchronises the device, and then on `stream`: the delay, a
device-to-device copy of the REAL input over the stale one, the entry point - and reads `busy = not stream.query()` as the first
statement after the call.  A launch, memset or copy that is not ordered behind the copy on `stream` (the null stream, a stream of the
library's own) computes from the stale input and gives other bits than the default-stream run; a call that waits for `stream` comes back
not busy.

The side streams come through a probe (`side_stream`): the runtime maps streams onto a few hardware queues, a queue takes its packets in
order, and a side stream that shares the null stream's queue hides exactly the mistakes this method is for (null_stream_overtakes).

`python -m tests.stream_cases first-call` is the child of test_gpu_streams.py's first-spectral-call test.
"""
import ctypes as C
import math
import re
import sys
import time
from pathlib import Path

import torch

from mimikit_amd import native
from tests import f64_bounds as B
from tests import filter_refs as FR
from tests import segment_refs as SR

ROOT = Path(__file__).resolve().parent.parent
PAD = 64                        # elements of surround on either side of every output (256 bytes of fp32: 16-byte alignment is kept)
DELAY_MS = 50.0                 # a parameter, not a tolerance: the `busy` assertion is the condition
STALE = 7919                    # seed offset of the stale draw
SLEEP_PROBE_CYCLES = 5_000_000  # the fixed cycle count the delay is calibrated with


# ====================================================================================================================== the table
class Entry:
    def __init__(self, rule, how, where=None, why=None, unless=None):
        assert rule in ("ASYNC", "WAITS", "NOT_RUN")
        assert rule != "WAITS" or (where and why), "a WAITS entry quotes its source line and its reason"
        self.rule, self.how, self.where, self.why, self.unless = rule, how, where, why, unless


_FIRST = "the first spectral call of a process on a device builds the twiddle and window tables and waits once (csrc/istft.hip:106)"
_GRAPH = "a block of 16 steps or more whose graph key differs from the cached one waits before capturing again ({})"
_CASE, _PLAN, _ERRW = "a Case of CASES behind late_input", "a PlanCase of PLAN_CASES: the plan's calls behind the delay", "the error-word test"
_COMMIT = "before the plan tests: every plan is committed on the default stream"

ENTRY_POINTS = {
    "mmk_fingerprint_u32": Entry("ASYNC", _CASE),
    "mmk_fingerprint_buffers_u32": Entry("ASYNC", _CASE),
    "mmk_mulaw_compress_f32_i64": Entry("ASYNC", _CASE),
    "mmk_mulaw_expand_i64_f32": Entry("ASYNC", _CASE),
    "mmk_resample_f32": Entry("ASYNC", _CASE),
    "mmk_lfilter1_f32": Entry("ASYNC", _CASE),
    "mmk_row_normalize_f32": Entry("ASYNC", _CASE),
    "mmk_inv_row_norm_f32": Entry("ASYNC", _CASE),
    "mmk_cosine_cost_f32": Entry("ASYNC", _CASE),
    "mmk_dtw_subseq_f32": Entry("ASYNC", _CASE),
    "mmk_nn_cosine_f32": Entry("ASYNC", _CASE),
    "mmk_cum_entropy_i64": Entry("ASYNC", _CASE),
    "mmk_nn_cosine_self_f32": Entry("ASYNC", _CASE),
    "mmk_nn_components_i64": Entry("ASYNC", _CASE),
    "mmk_segment_mean_f32": Entry("ASYNC", _CASE),
    "mmk_nn_topk_f32": Entry("ASYNC", _CASE),
    "mmk_half_neg_sqnorm_f32": Entry("ASYNC", _CASE),
    "mmk_edge_components_i64": Entry("WAITS", _CASE, "csrc/hcluster.hip:286: MMK_HIP(hipStreamSynchronize(st));",
                                     "the component sweeps read a `changed` flag back once per four rounds"),
    "mmk_novelty_f32": Entry("ASYNC", _CASE),
    "mmk_novelty_finish_f32": Entry("ASYNC", _CASE),
    "mmk_pick_peaks_f32": Entry("ASYNC", _CASE),
    "mmk_pca_colstats_f64": Entry("ASYNC", _CASE),
    "mmk_pca_cov_f64": Entry("ASYNC", _CASE),
    "mmk_pca_eig_f64": Entry("WAITS", _CASE, "csrc/pca.hip:730: MMK_HIP(hipStreamSynchronize(st));",
                             "the convergence flag is read back every 8 iterations"),
    "mmk_pca_project_f32": Entry("ASYNC", _CASE),
    "mmk_stft_mag_f32": Entry("ASYNC", _CASE, unless=_FIRST),
    "mmk_stft_f32": Entry("ASYNC", _CASE, unless=_FIRST),
    "mmk_stft_energy_f32": Entry("ASYNC", _CASE, unless=_FIRST),
    "mmk_interp1d_f32": Entry("ASYNC", _CASE),
    "mmk_derivative_f32": Entry("ASYNC", _CASE),
    "mmk_hpss_f32": Entry("ASYNC", _CASE),
    "mmk_melbank_f32": Entry("ASYNC", _CASE),
    "mmk_stft_mel_f32": Entry("ASYNC", _CASE, unless=_FIRST),
    "mmk_istft_f32": Entry("ASYNC", _CASE, unless=_FIRST),
    "mmk_gla_f32": Entry("ASYNC", _CASE, unless=_FIRST),
    "mmk_pack_weight_f32": Entry("ASYNC", _CASE),
    "mmk_linear_f32": Entry("ASYNC", _CASE),
    "mmk_gemm_f32": Entry("ASYNC", _CASE),
    "mmk_gemm_bias_act_f32": Entry("ASYNC", _CASE),
    "mmk_skinny_linear_f32": Entry("ASYNC", _CASE),
    "mmk_tr_attention_f32": Entry("ASYNC", _CASE),
    "mmk_tr_add_ln_f32": Entry("ASYNC", _CASE),
    "mmk_categorical_sample_f32_i64": Entry("ASYNC", _CASE),
    # ---- WaveNet plans
    "mmk_wavenet_commit": Entry("WAITS", _COMMIT, "csrc/wavenet_plan.hip:549: MMK_HIP(hipStreamSynchronize(st));   // replays of the cached graph may still be queued",
                                "the workspace is laid out anew under a graph that may still be queued; host-built tables are copied (:767, :842)"),
    "mmk_wavenet_warmup": Entry("ASYNC", _PLAN, unless=_GRAPH.format("csrc/wavenet_plan.hip:1256, the launch path's step-by-step warm-up")),
    "mmk_wavenet_generate": Entry("ASYNC", _PLAN, unless=_GRAPH.format("csrc/wavenet_plan.hip:1256, the launch path")),
    "mmk_wavenet_last_logits": Entry("ASYNC", _PLAN),
    "mmk_wavenet_last_logits_of": Entry("ASYNC", _PLAN),
    "mmk_wavenet_profile_steps": Entry("NOT_RUN", "a measurement aid of bench.py that times every launch with events and waits for them"),
    "mmk_wavenet_sync_status": Entry("WAITS", _ERRW, "csrc/wavenet_plan.hip:1420: MMK_HIP(hipStreamSynchronize(st));",
                                     "it is the call that waits for the stream and reads the plan's error word"),
    "mmk_wavenet_inject_sync_error": Entry("WAITS", _ERRW, "csrc/wavenet_plan.hip:1405: MMK_HIP(hipStreamSynchronize((hipStream_t)stream));",
                                           "the word is copied from a host local"),
    # ---- SampleRNN plans
    "mmk_srnn_commit": Entry("WAITS", _COMMIT, "csrc/srnn_plan.hip:455: MMK_HIP(hipStreamSynchronize(st));   // replays of the cached graph may still be queued",
                             "the workspace is laid out anew under a graph that may still be queued"),
    "mmk_srnn_reset": Entry("WAITS", _PLAN + " (called before the delay)", "csrc/srnn_plan.hip:402: MMK_HIP(hipStreamSynchronize(st));",
                            "the error word of the previous generation is read back first"),
    "mmk_srnn_warmup": Entry("ASYNC", _PLAN + " (the `launches` and the sampled case call it; it hands one stream to mmk_srnn_warmup_multi)",
                             unless=_GRAPH.format("csrc/srnn_plan.hip:862; SampleRNN: two periods of frame_sizes[0]")),
    "mmk_srnn_warmup_multi": Entry("ASYNC", _PLAN, unless=_GRAPH.format("csrc/srnn_plan.hip:862; SampleRNN: two periods of frame_sizes[0]")),
    "mmk_srnn_generate": Entry("ASYNC", _PLAN + " (the `launches` and the sampled case call it; it hands one stream to mmk_srnn_generate_multi)",
                               unless=_GRAPH.format("csrc/srnn_plan.hip:862; SampleRNN: two periods of frame_sizes[0]")),
    "mmk_srnn_generate_multi": Entry("ASYNC", _PLAN, unless=_GRAPH.format("csrc/srnn_plan.hip:862; SampleRNN: two periods of frame_sizes[0]")),
    "mmk_srnn_last_logits": Entry("ASYNC", _PLAN),
    "mmk_srnn_last_logits_of": Entry("ASYNC", _PLAN),
    "mmk_srnn_sync_status": Entry("WAITS", _ERRW, "csrc/srnn_plan.hip:1090: MMK_HIP(hipStreamSynchronize(st));",
                                  "it is the call that waits for the stream and reads the plan's error word"),
    "mmk_srnn_inject_sync_error": Entry("WAITS", _ERRW, "csrc/srnn_plan.hip:1075: MMK_HIP(hipStreamSynchronize((hipStream_t)stream));",
                                        "the word is copied from a host local"),
    # ---- Seq2Seq plans
    "mmk_s2s_commit": Entry("WAITS", _COMMIT, "include/mmk.h: `*_commit` may wait (csrc/s2s_plan.hip enqueues everything today)",
                            "a commit is allowed to wait like the other three; callers must not rely on this one returning early"),
    "mmk_s2s_step": Entry("ASYNC", _PLAN),
    "mmk_s2s_generate": Entry("ASYNC", _PLAN),
    "mmk_s2s_step_classes": Entry("ASYNC", _PLAN),
    "mmk_s2s_generate_classes": Entry("ASYNC", _PLAN),
    "mmk_s2s_last_logits": Entry("ASYNC", _PLAN),
    "mmk_s2s_sync_status": Entry("WAITS", _ERRW, "csrc/s2s_plan.hip:681: MMK_HIP(hipStreamSynchronize(st));",
                                 "it is the call that waits for the stream and reads the plan's error word"),
    "mmk_s2s_inject_sync_error": Entry("WAITS", _ERRW, "csrc/s2s_plan.hip:712: MMK_HIP(hipStreamSynchronize((hipStream_t)stream));",
                                       "the word is copied from a host local"),
    # ---- SimpleTransformer plans
    "mmk_tr_commit": Entry("WAITS", _COMMIT, "csrc/transformer_plan.hip:197: MMK_HIP(hipStreamSynchronize(st));",
                           "a cached graph holds the previous workspace's addresses and may still be in flight"),
    "mmk_tr_step": Entry("ASYNC", _PLAN),
    "mmk_tr_generate": Entry("ASYNC", _PLAN, unless=_GRAPH.format("csrc/transformer_plan.hip:375")),
    "mmk_tr_last_logits": Entry("ASYNC", _PLAN),
}
ASYNC = tuple(k for k, e in ENTRY_POINTS.items() if e.rule == "ASYNC")
WAITS = tuple(k for k, e in ENTRY_POINTS.items() if e.rule == "WAITS")
NOT_RUN = tuple(k for k, e in ENTRY_POINTS.items() if e.rule == "NOT_RUN")


def header_text():
    return (ROOT / "include" / "mmk.h").read_text()


def header_stream_functions(text=None):
    """the functions of include/mmk.h whose prototype has an mmk_stream_t parameter (comments stripped first)"""
    text = re.sub(r"/\*.*?\*/", " ", header_text() if text is None else text, flags=re.S)
    return sorted(m.group(1) for m in re.finditer(r"\b(mmk_[a-z0-9_]+)\s*\(([^;{}]*?)\)\s*;", text) if "mmk_stream_t" in m.group(2))


def header_streams_paragraph(text=None):
    """the streams item of the header's conventions: from '- streams.' to the next item of the list"""
    text = header_text() if text is None else text
    start = text.index("- streams.")
    return text[start:text.index("no torch / C++ types cross the boundary", start)]


# ====================================================================================================================== the cases
def gen(seed):
    return torch.Generator().manual_seed(int(seed))


def uni(g, *shape, lo=-1.0, hi=1.0):
    return torch.rand(*shape, generator=g) * (hi - lo) + lo


def P(t):
    return None if t is None else t.data_ptr()


def floats(n):
    return ((int(n),), torch.float32)


class Case:
    """entry: the exported function; tag: the case's own name under it; build(seed) -> {name: host tensor}, the inputs, all of them written
    late; outs(L, i) -> {name: (shape, dtype)}; work(L, i) -> {name: bytes}, zero-filled before every call; const(L, i) -> {name: (shape,
    dtype)} filled once by setup(L, a, s) on the default stream from the REAL inputs (packed weights); call(L, a, s) -> the return code,
    a = inputs, outputs, workspaces and constants by name, s = the stream as an integer; ref(i) -> float64 restatement on the host (numpy
    or torch), where the family's refs module has one."""

    def __init__(self, entry, build, outs, call, tag="", work=None, const=None, setup=None, ref=None, delay_ms=DELAY_MS):
        self.entry, self.tag, self.build, self.outs, self.call = entry, tag, build, outs, call
        self.work, self.const, self.setup, self.ref, self.delay_ms = work, const, setup, ref, delay_ms

    @property
    def id(self):
        return self.entry + (f"[{self.tag}]" if self.tag else "")

    def stale(self, seed=0):
        return self.build(seed + STALE)


def _inv_norm(x):
    n = x.double().norm(dim=-1)
    return torch.where(n > 0, 1.0 / n, torch.zeros_like(n)).float()


def _fingerprint():
    def build(seed):
        return dict(words=torch.randint(-2 ** 31, 2 ** 31 - 1, (1000,), generator=gen(seed), dtype=torch.int64).to(torch.int32))
    return Case("mmk_fingerprint_u32", build, lambda L, i: dict(out=((1,), torch.int64)),
                lambda L, a, s: L.mmk_fingerprint_u32(P(a["words"]), 1000, P(a["out"]), s))


def _fingerprint_buffers():
    n_buf, each = 97, 40          # one launch per 96 buffers: two launches

    def build(seed):
        return dict(words=torch.randint(-2 ** 31, 2 ** 31 - 1, (n_buf * each,), generator=gen(seed), dtype=torch.int64).to(torch.int32))

    def call(L, a, s):
        ptrs = (native.vp * n_buf)(*[a["words"].data_ptr() + 4 * each * k for k in range(n_buf)])
        counts = (native.i64 * n_buf)(*[each] * n_buf)
        return L.mmk_fingerprint_buffers_u32(ptrs, counts, n_buf, P(a["out"]), s)
    return Case("mmk_fingerprint_buffers_u32", build, lambda L, i: dict(out=((1,), torch.int64)), call)


def _mulaw_compress():
    from mimikit_amd.features.functionals import mulaw_edges

    def build(seed):
        return dict(x=uni(gen(seed), 3001), edges=mulaw_edges(256, 1.0).clone())
    return Case("mmk_mulaw_compress_f32_i64", build, lambda L, i: dict(codes=((3001,), torch.int64)),
                lambda L, a, s: L.mmk_mulaw_compress_f32_i64(P(a["x"]), P(a["codes"]), 3001, 256, 1.0, P(a["edges"]), s))


def _mulaw_expand():
    from mimikit_amd.features.functionals import mulaw_table

    def build(seed):
        return dict(codes=torch.randint(0, 256, (3001,), generator=gen(seed)), table=mulaw_table(256, 1.0).clone())
    return Case("mmk_mulaw_expand_i64_f32", build, lambda L, i: dict(x=floats(3001)),
                lambda L, a, s: L.mmk_mulaw_expand_i64_f32(P(a["codes"]), P(a["x"]), 3001, 256, 1.0, P(a["table"]), s))


def _resample():
    orig, new, width, batch, n = 2, 3, 6, 2, 101

    def build(seed):
        return dict(x=uni(gen(seed), batch, n), table=uni(gen(5), new, 2 * width + orig))

    def outs(L, i):
        return dict(out=((batch, L.mmk_resample_n_out(n, orig, new)), torch.float32))

    def call(L, a, s):
        return L.mmk_resample_f32(P(a["x"]), n, batch, n, P(a["table"]), orig, new, width, P(a["out"]), a["out"].shape[1], s)
    return Case("mmk_resample_f32", build, outs, call,
                ref=lambda i: B.resample_ref(i["x"].double(), i["table"].double(), orig, new, width)[0])


LFILTER_N = min(n for n in FR.LENGTHS if n > FR.CHUNK)      # the shortest length of filter_refs.LENGTHS that is cut into more than one chunk


def _lfilter1():
    b0, b1, a1 = FR.REMOVE_DC
    batch, n = 3, LFILTER_N

    def build(seed):
        return dict(x=uni(gen(seed), batch, n))
    return Case("mmk_lfilter1_f32", build, lambda L, i: dict(y=((batch, n), torch.float32)),
                lambda L, a, s: L.mmk_lfilter1_f32(P(a["x"]), n, batch, n, b0, b1, a1, P(a["y"]), n, P(a["ws"]), s),
                work=lambda L, i: dict(ws=4 * L.mmk_lfilter1_workspace_floats(batch, n)),
                ref=lambda i: FR.lfilter1_ref(i["x"].double().numpy(), b0, b1, a1))


def _row_normalize():
    batch, n = 3, LFILTER_N

    def build(seed):
        return dict(x=uni(gen(seed), batch, n))
    return Case("mmk_row_normalize_f32", build, lambda L, i: dict(y=((batch, n), torch.float32)),
                lambda L, a, s: L.mmk_row_normalize_f32(P(a["x"]), n, batch, n, 2, 1e-12, P(a["y"]), n, P(a["ws"]), s),
                work=lambda L, i: dict(ws=4 * L.mmk_row_normalize_workspace_floats(batch, n)),
                ref=lambda i: FR.normalize_ref(i["x"].double().numpy(), 2))


def _inv_row_norm():
    batch, rows, k = 2, 5, 33

    def build(seed):
        return dict(x=uni(gen(seed), batch, rows, k))
    return Case("mmk_inv_row_norm_f32", build, lambda L, i: dict(out=((batch, rows), torch.float32)),
                lambda L, a, s: L.mmk_inv_row_norm_f32(P(a["x"]), rows * k, k, batch, rows, k, P(a["out"]), s),
                ref=lambda i: 1.0 / i["x"].double().norm(dim=-1))


def _cosine_cost():
    batch, n, m, k = 2, 5, 70, 33

    def build(seed):
        g = gen(seed)
        x, y = uni(g, batch, n, k), uni(gen(6), m, k)
        return dict(x=x, rx=_inv_norm(x).reshape(-1), y=y, ry=_inv_norm(y))

    def call(L, a, s):
        return L.mmk_cosine_cost_f32(P(a["x"]), n * k, k, P(a["rx"]), batch, n, P(a["y"]), k, P(a["ry"]), m, k, P(a["cost"]), s)
    return Case("mmk_cosine_cost_f32", build, lambda L, i: dict(cost=((batch, m, native.nnn_n_pad(n)), torch.float32)), call)


def _dtw_subseq():
    batch, n, m = 2, 5, 70

    def build(seed):
        cost = uni(gen(seed), batch, m, native.nnn_n_pad(n), lo=0.0, hi=2.0)
        cost[..., n:] = 1.0
        return dict(cost=cost)

    def call(L, a, s):
        return L.mmk_dtw_subseq_f32(P(a["cost"]), batch, n, m, P(a["end_col"]), P(a["end_val"]), P(a["last_row"]), s)
    return Case("mmk_dtw_subseq_f32", build,
                lambda L, i: dict(end_col=((batch,), torch.int64), end_val=((batch,), torch.float32), last_row=((batch, m), torch.float32)), call)


def _nn_cosine():
    rows, m, k = 50, 200, 33

    def build(seed):
        x, y = uni(gen(seed), rows, k), uni(gen(7), m, k)
        return dict(x=x, rx=_inv_norm(x), y=y, ry=_inv_norm(y))

    def call(L, a, s):
        return L.mmk_nn_cosine_f32(P(a["x"]), k, P(a["rx"]), rows, P(a["y"]), k, P(a["ry"]), m, k, P(a["index"]), P(a["best"]), P(a["ws"]),
                                   a["ws"].numel(), s)
    return Case("mmk_nn_cosine_f32", build, lambda L, i: dict(index=((rows,), torch.int64), best=((rows,), torch.float32)), call,
                work=lambda L, i: dict(ws=L.mmk_nn_cosine_workspace_bytes(rows, m)))


def _cum_entropy():
    batch, t = 3, 40

    def build(seed):
        return dict(items=torch.randint(0, 7, (batch, t), generator=gen(seed)))

    def ref(i):
        from tests import neighbors_refs as NR
        return torch.stack([torch.from_numpy(NR.cum_entropy64(row.numpy())) for row in i["items"]])
    return Case("mmk_cum_entropy_i64", build, lambda L, i: dict(total=((batch,), torch.float32), e=((batch, t), torch.float32)),
                lambda L, a, s: L.mmk_cum_entropy_i64(P(a["items"]), t, batch, t, P(a["total"]), P(a["e"]), t, s), ref=ref)


def _nn_cosine_self():
    rows, k = 50, 33

    def build(seed):
        x = uni(gen(seed), rows, k)
        return dict(x=x, rx=_inv_norm(x))

    def call(L, a, s):
        return L.mmk_nn_cosine_self_f32(P(a["x"]), k, P(a["rx"]), rows, k, P(a["index"]), P(a["best"]), P(a["ws"]), a["ws"].numel(), s)
    return Case("mmk_nn_cosine_self_f32", build, lambda L, i: dict(index=((rows,), torch.int64), best=((rows,), torch.float32)), call,
                work=lambda L, i: dict(ws=L.mmk_nn_cosine_workspace_bytes(rows, rows)))


def _nn_components():
    n = 300          # more than one block of 256 nodes

    def build(seed):
        return dict(nearest=torch.randint(0, n, (n,), generator=gen(seed)))

    def call(L, a, s):
        return L.mmk_nn_components_i64(P(a["nearest"]), n, P(a["labels"]), P(a["count"]), P(a["ws"]), a["ws"].numel(), s)
    return Case("mmk_nn_components_i64", build, lambda L, i: dict(labels=((n,), torch.int64), count=((1,), torch.int64)), call,
                work=lambda L, i: dict(ws=L.mmk_nn_components_workspace_bytes(n)))


def _segment_mean():
    n, k = 20, 7

    def build(seed):
        return dict(x=uni(gen(seed), n, k), order=torch.randperm(n, generator=gen(8)), offsets=torch.tensor([0, 5, 9, n]))

    def call(L, a, s):
        return L.mmk_segment_mean_f32(P(a["x"]), k, n, k, P(a["order"]), P(a["offsets"]), 3, P(a["out"]), k, s)
    return Case("mmk_segment_mean_f32", build, lambda L, i: dict(out=((3, k), torch.float32)), call)


def _nn_topk():
    rows, m, k, t = 50, 200, 33, 3

    def build(seed):
        x, y = uni(gen(seed), rows, k), uni(gen(9), m, k)
        return dict(x=x, y=y, ones=torch.ones(m), cshift=(-(y.double() ** 2).sum(-1) / 2).float())

    def call(L, a, s):
        return L.mmk_nn_topk_f32(P(a["x"]), k, P(a["ones"]), rows, P(a["y"]), k, P(a["ones"]), P(a["cshift"]), -math.inf, math.inf, m, k, t, 0,
                                 P(a["index"]), P(a["key"]), P(a["ws"]), a["ws"].numel(), s)
    return Case("mmk_nn_topk_f32", build, lambda L, i: dict(index=((rows, t), torch.int64), key=((rows, t), torch.float32)), call,
                work=lambda L, i: dict(ws=L.mmk_nn_topk_workspace_bytes(rows, m, t)))


def _half_neg_sqnorm():
    m, k = 200, 33

    def build(seed):
        return dict(y=uni(gen(seed), m, k))
    return Case("mmk_half_neg_sqnorm_f32", build, lambda L, i: dict(out=floats(m)),
                lambda L, a, s: L.mmk_half_neg_sqnorm_f32(P(a["y"]), k, m, k, P(a["out"]), s),
                ref=lambda i: -(i["y"].double() ** 2).sum(-1) / 2)


def _edge_components():
    n, n_edges = 300, 200

    def build(seed):
        g = gen(seed)
        return dict(src=torch.randint(0, n, (n_edges,), generator=g), dst=torch.randint(0, n, (n_edges,), generator=g))

    def call(L, a, s):
        return L.mmk_edge_components_i64(P(a["src"]), P(a["dst"]), n_edges, n, P(a["labels"]), P(a["count"]), P(a["ws"]), a["ws"].numel(), s)
    return Case("mmk_edge_components_i64", build, lambda L, i: dict(labels=((n,), torch.int64), count=((1,), torch.int64)), call,
                work=lambda L, i: dict(ws=L.mmk_edge_components_workspace_bytes(n)))


NOVELTY_T, NOVELTY_D, NOVELTY_HALVES = SR.TILE + 1, 33, (1, 6, SR.MAX_HALF)


def _novelty():
    T, D, halves = NOVELTY_T, NOVELTY_D, NOVELTY_HALVES

    def build(seed):
        return dict(x=uni(gen(seed), 1, T, D, lo=0.0))

    def call(L, a, s):
        h = (C.c_int32 * len(halves))(*halves)
        return L.mmk_novelty_f32(P(a["x"]), T * D, D, None, 1, T, D, h, len(halves), P(a["raw"]), s)
    return Case("mmk_novelty_f32", build, lambda L, i: dict(raw=((1, len(halves), T), torch.float32)), call,
                ref=lambda i: torch.from_numpy(SR.raw64(i["x"][0].double().numpy(), halves[1])))


def _novelty_finish():
    T, q = NOVELTY_T, len(NOVELTY_HALVES)

    def build(seed):
        return dict(raw=uni(gen(seed), 1, q, T))

    def call(L, a, s):
        return L.mmk_novelty_finish_f32(P(a["raw"]), 1, q, T, P(a["scores"]), P(a["dg"]), P(a["ws"]), a["ws"].numel() // 4, s)
    return Case("mmk_novelty_finish_f32", build, lambda L, i: dict(scores=((1, q, T), torch.float32), dg=((1, T), torch.float32)), call,
                work=lambda L, i: dict(ws=4 * L.mmk_novelty_finish_workspace_floats(1, q, T)),
                ref=lambda i: i["raw"].double() - i["raw"].double().min(-1, keepdim=True).values)


def _pick_peaks():
    n = 300

    def build(seed):
        return dict(x=uni(gen(seed), n, lo=0.0))

    def call(L, a, s):
        return L.mmk_pick_peaks_f32(P(a["x"]), n, 3, 5, 0.02, P(a["picked"]), P(a["ws"]), a["ws"].numel(), s)
    return Case("mmk_pick_peaks_f32", build, lambda L, i: dict(picked=((n,), torch.uint8)), call,
                work=lambda L, i: dict(ws=L.mmk_pick_peaks_workspace_bytes(n)))


PCA_N, PCA_D, PCA_K = 50, 9, 3


def _pca_x(seed):
    return uni(gen(seed), PCA_N, PCA_D) * torch.arange(1, PCA_D + 1)


def _pca_stats(x):
    x = x.double()
    return x.mean(0), x.std(0, unbiased=False)


def _pca_colstats():
    def build(seed):
        return dict(x=_pca_x(seed))

    def call(L, a, s):
        return L.mmk_pca_colstats_f64(P(a["x"]), PCA_D, PCA_N, PCA_D, P(a["mean"]), P(a["scale"]), P(a["ws"]), a["ws"].numel(), s)
    return Case("mmk_pca_colstats_f64", build, lambda L, i: dict(mean=((PCA_D,), torch.float64), scale=((PCA_D,), torch.float64)), call,
                work=lambda L, i: dict(ws=L.mmk_pca_colstats_workspace_bytes(PCA_N, PCA_D)), ref=lambda i: _pca_stats(i["x"])[1])


def _pca_cov():
    def build(seed):
        x = _pca_x(seed)
        mean, scale = _pca_stats(x)
        return dict(x=x, mean=mean, scale=scale)

    def call(L, a, s):
        return L.mmk_pca_cov_f64(P(a["x"]), PCA_D, PCA_N, PCA_D, P(a["mean"]), P(a["scale"]), P(a["c"]), P(a["ws"]), a["ws"].numel(), s)
    return Case("mmk_pca_cov_f64", build, lambda L, i: dict(c=((PCA_D, PCA_D), torch.float64)), call,
                work=lambda L, i: dict(ws=L.mmk_pca_cov_workspace_bytes(PCA_N, PCA_D)))


def _pca_cov64(seed):
    x = _pca_x(seed)
    mean, scale = _pca_stats(x)
    z = (x.double() - mean) / scale
    return z.t() @ z / (PCA_N - 1)


def _pca_eig():
    def build(seed):
        return dict(c=_pca_cov64(seed))

    def call(L, a, s):
        n_iter = C.c_int32(0)
        return L.mmk_pca_eig_f64(P(a["c"]), PCA_D, PCA_K, 0, P(a["components"]), P(a["variance"]), C.byref(n_iter), P(a["ws"]), a["ws"].numel(), s)
    return Case("mmk_pca_eig_f64", build, lambda L, i: dict(components=((PCA_K, PCA_D), torch.float64), variance=((PCA_K,), torch.float64)), call,
                work=lambda L, i: dict(ws=L.mmk_pca_eig_workspace_bytes(PCA_D, PCA_K)),
                ref=lambda i: torch.linalg.eigvalsh(i["c"]).flip(0)[:PCA_K])


def _pca_project():
    def build(seed):
        x = _pca_x(seed)
        mean, scale = _pca_stats(x)
        comp = torch.linalg.qr(uni(gen(10), PCA_D, PCA_K).double())[0].t().contiguous()
        return dict(y=x, mean=mean, scale=scale, components=comp)

    def call(L, a, s):
        return L.mmk_pca_project_f32(P(a["y"]), PCA_D, PCA_N, PCA_D, P(a["mean"]), P(a["scale"]), P(a["components"]), PCA_K, P(a["out"]), PCA_K, s)
    return Case("mmk_pca_project_f32", build, lambda L, i: dict(out=((PCA_N, PCA_K), torch.float32)), call,
                ref=lambda i: ((i["y"].double() - i["mean"]) / i["scale"]) @ i["components"].t())


# the three kernel families of the spectral entry points (csrc/istft.hip: 1024; csrc/spectral2048.hip: 2048 and 4096; the general kernel: the rest)
SPECTRAL_N_FFT = (1024, 2048, 256)
SPECTRAL_FRAMES, SPECTRAL_CLIPS = 9, 2
MEL_BANDS = 8


def _spectral_signal(seed, n_fft, clips=SPECTRAL_CLIPS):
    hop = n_fft // 4
    return uni(gen(seed + n_fft), clips, n_fft + (SPECTRAL_FRAMES - 1) * hop)


def _stft_mag(n_fft, clips=SPECTRAL_CLIPS):
    hop, bins = n_fft // 4, n_fft // 2 + 1

    def build(seed):
        return dict(x=_spectral_signal(seed, n_fft, clips))

    def call(L, a, s):
        n = a["x"].shape[1]
        return L.mmk_stft_mag_f32(P(a["x"]), n, clips, n, n_fft, hop, 0, P(a["out"]), s)
    return Case("mmk_stft_mag_f32", build, lambda L, i: dict(out=((clips, SPECTRAL_FRAMES, bins), torch.float32)), call, tag=str(n_fft),
                ref=lambda i: B.stft_ref(i["x"].double(), n_fft, hop, False)[0].abs())


def _stft(n_fft):
    hop, bins = n_fft // 4, n_fft // 2 + 1

    def build(seed):
        return dict(x=_spectral_signal(seed, n_fft))

    def call(L, a, s):
        n = a["x"].shape[1]
        return L.mmk_stft_f32(P(a["x"]), n, SPECTRAL_CLIPS, n, n_fft, hop, 0, 0, 0, P(a["out"]), s)
    return Case("mmk_stft_f32", build, lambda L, i: dict(out=((SPECTRAL_CLIPS, SPECTRAL_FRAMES, bins, 2), torch.float32)), call, tag=str(n_fft),
                ref=lambda i: torch.view_as_real(B.stft_ref(i["x"].double(), n_fft, hop, False)[0]))


def _stft_energy(n_fft):
    hop = n_fft // 4

    def build(seed):
        return dict(x=_spectral_signal(seed, n_fft))

    def call(L, a, s):
        n = a["x"].shape[1]
        return L.mmk_stft_energy_f32(P(a["x"]), n, SPECTRAL_CLIPS, n, n_fft, hop, 0, 0, P(a["out"]), s)
    return Case("mmk_stft_energy_f32", build, lambda L, i: dict(out=((SPECTRAL_CLIPS, SPECTRAL_FRAMES), torch.float32)), call, tag=str(n_fft),
                ref=lambda i: B.stft_ref(i["x"].double(), n_fft, hop, False)[0].abs().sum(-1))


def _bank():
    """a banded filter bank of MEL_BANDS bands of five bins, four apart (include/mmk.h: MelSpec): fits any frame of 37 bins or more"""
    band = torch.tensor([[4 * m, 5, 5 * m] for m in range(MEL_BANDS)], dtype=torch.int32)
    return band, uni(gen(11), 5 * MEL_BANDS, lo=0.0)


def _band_host(band):
    flat = [int(v) for v in band.reshape(-1)]
    return (C.c_int32 * len(flat))(*flat)


def _melbank():
    rows, bins = 5, 37

    def build(seed):
        band, weights = _bank()
        return dict(s=uni(gen(seed), rows, bins, lo=0.0), band=band, weights=weights)

    def call(L, a, s):
        host = _band_host(_bank()[0])
        return L.mmk_melbank_f32(P(a["s"]), bins, rows, bins, bins, MEL_BANDS, host, P(a["band"]), P(a["weights"]), 5 * MEL_BANDS, None, 0, P(a["out"]), s)
    return Case("mmk_melbank_f32", build, lambda L, i: dict(out=((rows, MEL_BANDS), torch.float32)), call)


def _stft_mel(n_fft):
    hop, bins = n_fft // 4, n_fft // 2 + 1

    def build(seed):
        band, weights = _bank()
        return dict(x=_spectral_signal(seed, n_fft), band=band, weights=weights)

    def call(L, a, s):
        n = a["x"].shape[1]
        host = _band_host(_bank()[0])
        return L.mmk_stft_mel_f32(P(a["x"]), n, SPECTRAL_CLIPS, n, n_fft, hop, 0, 0, bins, MEL_BANDS, host, P(a["band"]), P(a["weights"]),
                                  5 * MEL_BANDS, None, 0, P(a["out"]), s)
    return Case("mmk_stft_mel_f32", build, lambda L, i: dict(out=((SPECTRAL_CLIPS, SPECTRAL_FRAMES, MEL_BANDS), torch.float32)), call, tag=str(n_fft))


def _istft(n_fft):
    hop, bins = n_fft // 4, n_fft // 2 + 1

    def build(seed):
        return dict(spec=uni(gen(seed + n_fft), SPECTRAL_CLIPS, SPECTRAL_FRAMES, bins, 2))

    def call(L, a, s):
        return L.mmk_istft_f32(P(a["spec"]), 0, SPECTRAL_CLIPS, SPECTRAL_FRAMES, n_fft, hop, P(a["ws"]), P(a["out"]), s)
    return Case("mmk_istft_f32", build, lambda L, i: dict(out=((SPECTRAL_CLIPS, hop * (SPECTRAL_FRAMES - 1)), torch.float32)), call, tag=str(n_fft),
                work=lambda L, i: dict(ws=4 * L.mmk_istft_workspace_floats(SPECTRAL_CLIPS, SPECTRAL_FRAMES, n_fft)),
                ref=lambda i: B.istft_ref(torch.view_as_complex(i["spec"].double().contiguous()), n_fft, hop)[0])


def _gla():
    n_fft, hop, n_iter = 1024, 256, 3
    bins = n_fft // 2 + 1

    def build(seed):
        g = gen(seed)
        return dict(mag=uni(g, SPECTRAL_CLIPS, SPECTRAL_FRAMES, bins, lo=0.0), init=uni(g, SPECTRAL_CLIPS, SPECTRAL_FRAMES, bins, 2, lo=0.0))

    def call(L, a, s):
        return L.mmk_gla_f32(P(a["mag"]), P(a["init"]), SPECTRAL_CLIPS, SPECTRAL_FRAMES, n_fft, hop, n_iter, 0.99, P(a["ws"]), P(a["out"]), s)
    return Case("mmk_gla_f32", build, lambda L, i: dict(out=((SPECTRAL_CLIPS, hop * (SPECTRAL_FRAMES - 1)), torch.float32)), call,
                work=lambda L, i: dict(ws=4 * L.mmk_gla_workspace_floats(SPECTRAL_CLIPS, SPECTRAL_FRAMES, n_fft, hop)))


def _interp1d():
    batch, n, n_out = 2, 100, 257

    def build(seed):
        return dict(x=uni(gen(seed), batch, n))
    return Case("mmk_interp1d_f32", build, lambda L, i: dict(y=((batch, n_out), torch.float32)),
                lambda L, a, s: L.mmk_interp1d_f32(P(a["x"]), n, batch, n, P(a["y"]), n_out, n_out, 0, 1, s))


def _derivative():
    batch, n, lag = 2, native.DERIV_TILE + 6, 3      # two tiles

    def build(seed):
        return dict(x=uni(gen(seed), batch, n))
    return Case("mmk_derivative_f32", build, lambda L, i: dict(y=((batch, n), torch.float32)),
                lambda L, a, s: L.mmk_derivative_f32(P(a["x"]), n, batch, n, lag, P(a["y"]), n, s))


HPSS_SHAPE = (1, native.HPSS_TILE_FRAMES + 1, native.HPSS_TILE_BINS + 1)


def _hpss(seed0=0):
    clips, frames, bins = HPSS_SHAPE
    names = ("harmonic", "percussive", "harm_median", "perc_median")

    def build(seed):
        return dict(s=uni(gen(seed + seed0), clips, frames, bins, lo=0.0))

    def call(L, a, s):
        return L.mmk_hpss_f32(P(a["s"]), frames * bins, bins, clips, frames, bins, 31, 31, 1.0, 1.0, 1.0, *[P(a[k]) for k in names],
                              frames * bins, bins, s)

    def ref(i):
        from tests import hpss_refs as HR
        return torch.from_numpy(HR.hpss64(i["s"].numpy(), 31)[0])
    return Case("mmk_hpss_f32", build, lambda L, i: {k: (HPSS_SHAPE, torch.float32) for k in names}, call, ref=ref)


def _packed(n, k):
    return lambda L, i: dict(packed=floats(L.mmk_packed_weight_floats(n, k)))


def _pack(n, k):
    def setup(L, a, s):
        return L.mmk_pack_weight_f32(P(a["w"]), k, n, k, P(a["packed"]), s)
    return setup


def _pack_weight():
    n, k = 33, 20

    def build(seed):
        return dict(w=uni(gen(seed), n, k))
    return Case("mmk_pack_weight_f32", build, lambda L, i: dict(packed=floats(L.mmk_packed_weight_floats(n, k))),
                lambda L, a, s: L.mmk_pack_weight_f32(P(a["w"]), k, n, k, P(a["packed"]), s))


def _linear():
    m, n, k = 5, 33, 20

    def build(seed):
        return dict(x=uni(gen(seed), m, k), w=uni(gen(12), n, k), bias=uni(gen(13), n))
    return Case("mmk_linear_f32", build, lambda L, i: dict(y=((m, n), torch.float32)),
                lambda L, a, s: L.mmk_linear_f32(P(a["x"]), k, m, P(a["packed"]), P(a["bias"]), n, k, P(a["y"]), n, 1, s),
                const=_packed(n, k), setup=_pack(n, k), ref=lambda i: torch.tanh(i["x"].double() @ i["w"].double().t() + i["bias"].double()))


def _gemm():
    batch, m, n, k = 2, 70, 33, 48

    def build(seed):
        return dict(a=uni(gen(seed), batch, m, k), w=uni(gen(14), n, k))

    def call(L, a, s):
        return L.mmk_gemm_f32(P(a["a"]), k, m * k, P(a["packed"]), n, k, P(a["c"]), n, m * n, m, batch, s)
    return Case("mmk_gemm_f32", build, lambda L, i: dict(c=((batch, m, n), torch.float32)), call, const=_packed(n, k), setup=_pack(n, k),
                ref=lambda i: i["a"].double() @ i["w"].double().t())


GEMM_K_SPLIT = 2


def _gemm_bias_act():
    m, n, k = 130, 33, 128          # two 64-column stages of K, split two ways: the partial launch and the one that adds them up

    def build(seed):
        return dict(a=uni(gen(seed), m, k), w=uni(gen(15), n, k), bias=uni(gen(16), n))

    def call(L, a, s):
        return L.mmk_gemm_bias_act_f32(P(a["a"]), k, m, P(a["packed"]), P(a["bias"]), n, k, P(a["c"]), n, 1, 0, 0, 0, 0, P(a["partial"]),
                                       a["partial"].numel() // 4, GEMM_K_SPLIT, s)
    return Case("mmk_gemm_bias_act_f32", build, lambda L, i: dict(c=((m, n), torch.float32)), call, const=_packed(n, k), setup=_pack(n, k),
                work=lambda L, i: dict(partial=4 * L.mmk_gemm_partial_floats(m, n, k, GEMM_K_SPLIT)),
                ref=lambda i: torch.tanh(i["a"].double() @ i["w"].double().t() + i["bias"].double()))


def _skinny_linear():
    m, n, k = 5, 33, 128

    def build(seed):
        return dict(a=uni(gen(seed), m, k), w=uni(gen(17), n, k), bias=uni(gen(18), n))
    return Case("mmk_skinny_linear_f32", build, lambda L, i: dict(c=((m, n), torch.float32)),
                lambda L, a, s: L.mmk_skinny_linear_f32(P(a["a"]), k, m, P(a["packed"]), P(a["bias"]), n, k, P(a["c"]), n, 3, s),
                const=_packed(n, k), setup=_pack(n, k))


def _tr_attention():
    batch, n_q, n_keys, heads, hd = 2, 5, 9, 2, 8
    D = heads * hd

    def build(seed):
        g = gen(seed)
        return dict(q=uni(g, batch, n_q, D), k=uni(g, batch, n_keys, D), v=uni(g, batch, n_keys, D))

    def call(L, a, s):
        return L.mmk_tr_attention_f32(P(a["q"]), D, n_q * D, P(a["k"]), P(a["v"]), D, n_keys * D, P(a["out"]), D, n_q * D, n_q, n_keys - n_q, n_keys,
                                      heads, hd, 1.0 / math.sqrt(hd), batch, s)

    def ref(i):
        q, k, v = (i[n].double().reshape(batch, -1, heads, hd) for n in "qkv")
        return B.attention_ref(q, k, v, n_keys - n_q, 1.0 / math.sqrt(hd))[0]
    return Case("mmk_tr_attention_f32", build, lambda L, i: dict(out=((batch, n_q, D), torch.float32)), call, ref=ref)


def _tr_add_ln():
    rows, d = 7, 70

    def build(seed):
        g = gen(seed)
        return dict(y=uni(g, rows, d), res=uni(g, rows, d), w=uni(gen(19), d), b=uni(gen(20), d))
    return Case("mmk_tr_add_ln_f32", build, lambda L, i: dict(out=((rows, d), torch.float32)),
                lambda L, a, s: L.mmk_tr_add_ln_f32(P(a["y"]), d, P(a["res"]), d, P(a["w"]), P(a["b"]), P(a["out"]), d, rows, d, s),
                ref=lambda i: B.ln_ref(i["y"].double() + i["res"].double(), i["w"].double(), i["b"].double())[0])


def _categorical_sample():
    rows, classes = 9, 256

    def build(seed):
        g = gen(seed)
        return dict(logits=uni(g, rows, classes + 1, lo=-3.0, hi=3.0), temperature=uni(gen(21), rows, lo=0.5, hi=1.5), uniforms=uni(g, rows, lo=0.0))

    def call(L, a, s):
        return L.mmk_categorical_sample_f32_i64(P(a["logits"]), classes + 1, rows, classes, 1, 0.9, P(a["temperature"]), P(a["uniforms"]), P(a["out"]), 1, s)
    return Case("mmk_categorical_sample_f32_i64", build, lambda L, i: dict(out=((rows,), torch.int64)), call)


# the integer inputs of the cases: every value lies in [0, INT_BELOW[name]) in the real and in the stale draw
INT_BELOW = dict(codes=256, items=7, nearest=300, src=300, dst=300, order=20, offsets=21, band=5 * MEL_BANDS)

CASES = [_fingerprint(), _fingerprint_buffers(), _mulaw_compress(), _mulaw_expand(), _resample(), _lfilter1(), _row_normalize(), _inv_row_norm(),
         _cosine_cost(), _dtw_subseq(), _nn_cosine(), _cum_entropy(), _nn_cosine_self(), _nn_components(), _segment_mean(), _nn_topk(),
         _half_neg_sqnorm(), _edge_components(), _novelty(), _novelty_finish(), _pick_peaks(), _pca_colstats(), _pca_cov(), _pca_eig(), _pca_project(),
         *[_stft_mag(n) for n in SPECTRAL_N_FFT], *[_stft(n) for n in SPECTRAL_N_FFT], *[_stft_energy(n) for n in SPECTRAL_N_FFT], _interp1d(),
         _derivative(), _hpss(), _melbank(), *[_stft_mel(n) for n in SPECTRAL_N_FFT], *[_istft(n) for n in SPECTRAL_N_FFT], _gla(), _pack_weight(),
         _linear(), _gemm(), _gemm_bias_act(), _skinny_linear(), _tr_attention(), _tr_add_ln(), _categorical_sample()]
BY_ID = {c.id: c for c in CASES}
ASYNC_CASES = [c for c in CASES if ENTRY_POINTS[c.entry].rule == "ASYNC"]
WAITS_CASES = [c for c in CASES if ENTRY_POINTS[c.entry].rule == "WAITS"]
# the stateless functions two streams run side by side, and the two whose null-stream launch the method must be able to see
TWO_STREAM_CASES = ("mmk_stft_mag_f32[1024]", "mmk_lfilter1_f32", "mmk_nn_topk_f32", "mmk_hpss_f32")
NULL_STREAM_CASES = ("mmk_lfilter1_f32", "mmk_stft_mag_f32[1024]")


# ====================================================================================================================== the plans
class PlanCase:
    """network: 'wavenet' | 'srnn' | 's2s' | 'tr'; ref: the id of the case in net_refs (WAVENET_CASES, SRNN_CASES, S2S_ALL) or
    transformer_refs.CASES; n: steps of the block (below the graph threshold unless `graph`; a resident SampleRNN block is the case's
    own first block, a resident launch has no graph); sampled: temperatures and uniforms are passed in"""

    def __init__(self, network, ref, n=None, sampled=False, graph=False):
        self.network, self.ref, self.n, self.sampled, self.graph = network, ref, n, sampled, graph

    @property
    def id(self):
        return f"{self.network}-{self.ref}" + ("-sampled" if self.sampled else "") + ("-graph" if self.graph else "")


GRAPH_STEPS = 8           # csrc/wavenet_plan.hip, csrc/transformer_plan.hip: kGraphSteps
SHORT_BLOCK = 9           # < 2 * GRAPH_STEPS: nothing is captured
PLAN_CASES = (
    [PlanCase("wavenet", r) for r in ("launches", "persist", "chain", "lpipe-4_3-13", "spipe-5", "spipe-pair-24", "bpipe-20", "frames-g4")]
    + [PlanCase("srnn", r) for r in ("launches", "bottom-one_clip", "bottom-four_clips-321", "resident-gru")]
    + [PlanCase("s2s", r) for r in ("resident-128-2-3", "per_frame", "launches", "classes")]
    + [PlanCase("tr", "one_layer_rf9")]
    + [PlanCase("wavenet", "chain", sampled=True), PlanCase("srnn", "bottom-one_clip", sampled=True), PlanCase("tr", "one_layer_rf9", sampled=True)]
    + [PlanCase("wavenet", "launches", n=2 * GRAPH_STEPS + 3, graph=True)])
ERROR_WORD_CASES = [PlanCase("srnn", "resident-gru"), PlanCase("wavenet", "persist"), PlanCase("s2s", "resident-128-2-3")]


def plan_ref(pc):
    """the net_refs / transformer_refs case a PlanCase stands on"""
    if pc.network == "tr":
        from tests import transformer_refs as TR
        return TR.BY_TAG[pc.ref]
    from tests import net_refs as R
    pool = {"wavenet": R.WAVENET_CASES, "srnn": R.SRNN_CASES, "s2s": R.S2S_ALL}[pc.network]
    return next(c for c in pool if c.id == pc.ref)


# ====================================================================================================================== the method
_cycles_per_ms = None


def cycles_per_ms():
    """torch.cuda._sleep's cycles per millisecond on this device: SLEEP_PROBE_CYCLES timed between two events, once per process"""
    global _cycles_per_ms
    if _cycles_per_ms is None:
        torch.cuda._sleep(1000)                      # (code loading)
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        start.record()
        torch.cuda._sleep(SLEEP_PROBE_CYCLES)
        stop.record()
        stop.synchronize()
        _cycles_per_ms = SLEEP_PROBE_CYCLES / max(start.elapsed_time(stop), 1e-3)
    return _cycles_per_ms


def delay(stream, ms):
    """keep `stream` busy for about `ms` (one wave spinning in torch.cuda._sleep)"""
    cycles = int(cycles_per_ms() * ms)
    with torch.cuda.stream(stream):
        torch.cuda._sleep(cycles)


NOT_ORDERED = ("the side stream and the null stream are ordered on this machine after all: the stream tests cannot see a null-stream launch")
_side_streams = []


def null_stream_overtakes(stream, ms=20.0):
    """a small fill on the null stream completes while `stream` is still held by a delay.  The runtime maps its streams onto a few
    hardware queues (four here, round robin) and a queue takes its packets in order, so a side stream that shares the null stream's
    queue IS ordered against it whatever its flags say - behind such a stream a null-stream launch computes from the late input like
    any other, and the method sees nothing.  One of eight side streams did on the first run (tests/test_gpu_streams.py: records)."""
    probe = torch.zeros(64, device="cuda")
    done = torch.cuda.Event()
    torch.cuda.synchronize()
    delay(stream, ms)
    probe.fill_(1.0)
    done.record()
    t0 = time.perf_counter()
    while not done.query() and time.perf_counter() - t0 < ms / 4000.0:
        pass
    overtook = done.query() and not stream.query()
    stream.synchronize()
    torch.cuda.synchronize()
    return overtook


def side_streams(device, count=1):
    """`count` distinct side streams that the null stream is SEEN to overtake (null_stream_overtakes), found once per process among
    the streams torch hands out and kept: every test of the method runs behind one of them"""
    cycles_per_ms()
    tried = 0
    while len(_side_streams) < count and tried < 16:
        tried += 1
        s = torch.cuda.Stream(device)
        if all(s.cuda_stream != t.cuda_stream for t in _side_streams) and null_stream_overtakes(s):
            _side_streams.append(s)
    assert len(_side_streams) >= count, NOT_ORDERED + f" ({len(_side_streams)} of {tried} side streams were overtaken by a null-stream fill)"
    return _side_streams[:count]


def side_stream(device):
    return side_streams(device, 1)[0]


def same_bits(a, b):
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.dtype == torch.float32:
        return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))
    if a.dtype == torch.float64:
        return torch.equal(a.contiguous().view(torch.int64), b.contiguous().view(torch.int64))
    return torch.equal(a, b)


_FILL = {torch.float32: float("nan"), torch.float64: float("nan"), torch.int64: -7777, torch.int32: -7777, torch.uint8: 0xA5}


class Bound:
    """a Case on a device: the real and the stale inputs, the input buffers the entry point reads, every output in the middle of a buffer
    with PAD elements of surround (NaN for floats, as f64_bounds.check_written expects; a sentinel for integers), zero-filled workspaces"""

    def __init__(self, case, device, seed=0):
        self.case, self.L = case, native.lib()
        host = case.build(seed)
        self.real = {k: v.to(device) for k, v in host.items()}
        self.stale = {k: v.to(device) for k, v in case.build(seed + STALE).items()}
        self.inp = {k: torch.empty_like(v) for k, v in self.real.items()}
        self.bufs, self.out = {}, {}
        for k, (shape, dtype) in case.outs(self.L, host).items():
            n = math.prod(shape)
            self.bufs[k] = torch.empty(n + 2 * PAD, dtype=dtype, device=device)
            self.out[k] = self.bufs[k][PAD:PAD + n].view(shape)
        self.work = {k: torch.zeros(max(int(b), 16), dtype=torch.uint8, device=device) for k, b in (case.work(self.L, host) if case.work else {}).items()}
        self.const = {k: torch.zeros(shape, dtype=dtype, device=device) for k, (shape, dtype) in (case.const(self.L, host) if case.const else {}).items()}
        if case.setup:
            rc = case.setup(self.L, {**self.real, **self.const}, native.stream_ptr(device))
            assert rc == 0, (case.id, "setup", rc, self.L.mmk_last_error())
        torch.cuda.synchronize()

    def fill(self, which, keep_work=False):
        """put the real or the stale inputs in place, clear the outputs and the workspaces (default stream); keep_work: leave the workspaces
        as the previous call left them (tests/graph_cases.py: what a replayed graph finds)"""
        for k, v in (self.real if which == "real" else self.stale).items():
            self.inp[k].copy_(v)
        for k, b in self.bufs.items():
            b.fill_(_FILL[b.dtype])
        if not keep_work:
            for w in self.work.values():
                w.zero_()

    def late_copy(self):
        for k, v in self.real.items():
            self.inp[k].copy_(v, non_blocking=True)

    def call(self, stream_ptr):
        rc = self.case.call(self.L, {**self.inp, **self.out, **self.work, **self.const}, stream_ptr)
        assert rc == 0, (self.case.id, rc, self.L.mmk_last_error())

    def outputs(self):
        return {k: v.clone().cpu() for k, v in self.out.items()}

    def check_surround(self, what):
        for k, b in self.bufs.items():
            n = b.numel() - 2 * PAD
            if b.dtype.is_floating_point:
                mask = torch.zeros(b.numel(), dtype=torch.bool)
                mask[PAD:PAD + n] = True
                B.check_written(b, mask, f"{what} {k}")
            else:
                edge = torch.cat([b[:PAD], b[PAD + n:]]).cpu()
                assert bool((edge == _FILL[b.dtype]).all()), f"{what} {k}: written outside the output"

    def run_default(self, which):
        """one call on torch's current (default) stream with the real or the stale input in place -> outputs on the host"""
        self.fill(which)
        self.call(native.stream_ptr(self.inp_device))
        torch.cuda.synchronize()
        return self.outputs()

    @property
    def inp_device(self):
        return next(iter(self.inp.values())).device


def differs(a, b):
    """two output sets differ somewhere, bit for bit"""
    return any(not same_bits(a[k], b[k]) for k in a)


def late_input(bound, stream, ms=None, call_stream=None):
    """the driver (module docstring) -> (outputs on the host, busy, host seconds of the call).  call_stream: the stream the entry point
    is GIVEN when it is not `stream` (0: the null stream - how the tests show that the method sees a launch that left its stream)"""
    cycles_per_ms()
    bound.fill("stale")                                                     # 1
    torch.cuda.synchronize()                                                # 2
    delay(stream, bound.case.delay_ms if ms is None else ms)                # 3
    with torch.cuda.stream(stream):
        bound.late_copy()                                                   # 4
    t0 = time.perf_counter()
    bound.call(stream.cuda_stream if call_stream is None else call_stream)  # 5
    busy = not stream.query()                                               # 6
    host = time.perf_counter() - t0
    stream.synchronize()                                                    # 7
    torch.cuda.synchronize()
    return bound.outputs(), busy, host                                      # 8


# ====================================================================================================================== the child
def first_call():
    """the first library call of this process is mmk_stft_mag_f32 (1024 / 256) on a side stream behind the delay and a late input, then at
    once mmk_istft_f32 on a second side stream; both again on the default stream; 0 if the bits agree"""
    device = torch.device("cuda", 0)
    torch.set_grad_enabled(False)
    mag, inv = Bound(BY_ID["mmk_stft_mag_f32[1024]"], device), Bound(BY_ID["mmk_istft_f32[1024]"], device)
    s1, s2 = side_streams(device, 2)       # (torch only: no library call yet)
    mag.fill("stale")
    inv.fill("real")
    torch.cuda.synchronize()
    delay(s1, DELAY_MS)
    with torch.cuda.stream(s1):
        mag.late_copy()
    mag.call(s1.cuda_stream)               # the first library call of the process: builds the tables on s1 and waits
    inv.call(s2.cuda_stream)               # reads the tables from another stream at once
    s1.synchronize()
    s2.synchronize()
    torch.cuda.synchronize()
    got = (mag.outputs(), inv.outputs())
    want = (mag.run_default("real"), inv.run_default("real"))
    bad = [f"{b.case.id} {k}: {int((g[k] != w[k]).sum())} of {g[k].numel()} elements differ from the default-stream run"
           for b, g, w in zip((mag, inv), got, want) for k in g if not same_bits(g[k], w[k])]
    for b in (mag, inv):
        b.check_surround(b.case.id)
    for line in bad:
        print(line)
    return 1 if bad else 0


if __name__ == "__main__":
    if sys.argv[1:] == ["first-call"]:
        sys.exit(first_call())
    sys.exit(f"usage: python -m tests.stream_cases first-call (got {sys.argv[1:]})")
