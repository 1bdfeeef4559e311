"""float64 references of the SimpleTransformer step outputs and the tolerance that derives from them, shared by test_transformer_refs.py
(CPU: the references against each other) and test_gpu_transformer_f64.py (the device against them).  The part tests/net_refs.py plays for
WaveNet, SampleRNN and Seq2Seq, and its rule: for a history (the classes or frames a run produced) the network is run teacher-forced three times

  R64   the walk below in float64 (float64 weights and arithmetic)
  R32   the network's own fp32 modules on the CPU: what the reference project computes
  R32k  the walk in fp32 with the head's activation in the step kernels' formula (net_refs.KERNEL_FORMULAS, csrc/mmk_common.h)

E = max(|R32 - R64|, |R32k - R64|) element by element is the reference's own fp32 error on THIS history; tol_max = 4 max(E), tol_rms = 4 rms(E)
over exactly the compared elements (net_refs.FACTOR, tolerance, check_outputs, check_picks, check_near_miss, ratios: used as they are).

The walk is a plain restatement of one step: X0 = embedding (or the input Linear) of the rf-long window + pe[0:rf]; every decoder layer
(post-norm: causal self-attention, add + LN1, causal cross-attention on memory = X0, add + LN2, Linear - ReLU - Linear, add + LN3); the last
window position; the final LayerNorm (with_layer_norm); the head (MLP: the raw outputs of its last Linear, q classes and the temperature
column; frames: Linear + Abs).  In float64 it is the network's own modules to 1e-12 x scale (torch_outputs_f64), asserted for every case.
With bound=True the same walk carries, next to every activation, the bound derived from the kernels' bounds (tests/f64_bounds.py): the
derived-bound test of test_gpu_transformer.py, whose looseness test_transformer_refs.py prints per case.

Defects are variants of the float64 walk, one at a time; each must leave tol_max somewhere among the compared elements, for every case it
applies to.  Where one cannot apply, the rule says why:
  (a) the median-magnitude entry of the last layer's self_attn.out_proj.bias dropped
  (b) the middle layer's (num_layers // 2) multihead_attn.in_proj_weight scaled by 1 + 1e-4: its query rows and the key / value rows the plan
      gathers into the all-layers cross-attention GEMM
  (c) the last clip's rows replaced by the second-to-last clip's (a ragged tile that reads its neighbour)
  (d) clip 0's window one step stale (the graph's step counter)
  (e) a causal mask leaking one key.  num_layers >= 2 only: with one layer the only query the outputs depend on is the last row's, which
      sees every key - the defect moves nothing there
  (f) the last layer's query and LN1 residual taken at window position rf - 2 (it still sees every key).  rf >= 2 only: at rf 1 there is no such row
  (g) pe[1:rf + 1] added instead of pe[0:rf]
  (h) the cross-attention keys and values of every layer l >= 1 made from that layer's input instead of X0.  num_layers >= 2 only: layer 0's
      input is X0
  (i) the final LayerNorm skipped.  with_layer_norm cases only: the others have none
"""
import functools
import math
from typing import NamedTuple

import torch

import mimikit_amd as mmk
from mimikit_amd import native
from oracle.weights import recipe_state_dict
from tests import net_refs as N
from tests.f64_bounds import ACT_F, ACT_LIP, U, attention_bound, gemm_bound, ln_bound, ln_ref
from tests.net_refs import FACTOR, Envelope, check_near_miss, check_outputs, check_picks, ratios, rms, tolerance  # noqa: F401

GAIN = 1.5              # the gain of the golden vectors and of test_gpu_transformer.py
# The cases' weights.  The recipe (oracle/weights.py) draws every 1-D `weight` as U(+-gain / sqrt(D)) - LayerNorm weights around ZERO.  A
# LayerNorm of such weights passes about a twentieth of what reaches it, three of them per layer: measured on the default network (recipe seed 97,
# gain 1.5), the cross-attention in_proj_weight of layer l scaled by 1 + 1e-4 moves the outputs by 1.2, 6e-2, 1e-3, 6e-5, 2e-6, 3e-8, 1e-9,
# 3e-10 tol_max for l = 7 .. 0: defect (b) of the middle layer cannot leave the envelope, and neither could a kernel's mistake in any layer
# but the last two.  And the greedy picks of every case are ONE class from the first step on, whatever the prompt.  So the cases add 1 to the
# LayerNorm weights the recipe drew (weights around one, as a trained network has them) and take gain 2.5: the same scaling then moves the
# default network's outputs by 0.47, 1.1, 1.3, 3.3, 3.7, 8.2, 11 and 16 tol_max for l = 0 .. 7 - every layer counts - and the picks depend on
# the prompt (test_transformer_refs.py asserts both).
CASE_GAIN = 2.5
CASE_LN_OFFSET = 1.0


# ---- the cases -----------------------------------------------------------------------------------------------------------------------------------------
class Case(NamedTuple):
    """net_kw: SimpleTransformer.Config keywords; io_kw: build()'s; parts: the lengths of the consecutive generate_block calls; seed: the recipe's
    (the prompt's is seed + clips); reaches: the plan branch the case is there for (csrc/transformer_plan.hip)"""
    tag: str
    net_kw: dict
    io_kw: dict
    clips: int
    parts: tuple
    seed: int
    reaches: str

    @property
    def rf(self):
        return self.net_kw.get("rf", 64)

    @property
    def prompt(self):
        return self.rf + 3

    @property
    def n(self):
        return sum(self.parts)

    @property
    def classes(self):
        return self.io_kw["kind"] == "mulaw"

    @property
    def layers(self):
        return self.net_kw.get("num_layers", 8)

    def ends(self):
        """the steps after which a block ends: the rows last_logits hands back"""
        out, t = [], 0
        for nb in self.parts:
            t += nb
            out.append(t - 1)
        return out

    def inputs(self, seed=None):
        """the prompt (clips, rf + 3[, bins]) on the host"""
        g = torch.Generator().manual_seed(self.seed + self.clips if seed is None else seed)
        if self.classes:
            return torch.randint(0, 256, (self.clips, self.prompt), generator=g)
        return torch.rand(self.clips, self.prompt, self.io_kw["n_fft"] // 2 + 1, generator=g)


# 19 steps: two replays of the 8-step graph and three plain steps; 16 at another t0: a new key, captured again; 5: below 2 x 8, no graph
PARTS = (19, 16, 5)
_RF65 = dict(model_dim=48, n_heads=4, feedforward_dim=96, num_layers=2, rf=65, with_layer_norm=True)
CASES = [
    Case("one_layer_rf9", dict(model_dim=32, n_heads=4, feedforward_dim=64, num_layers=1, rf=9), dict(kind="mulaw", n_mlp_layers=1), 3, PARTS, 90,
         "the only layer is the last-row branch: its query and LN1 residual read out of X0 at row stride rf D"),
    Case("clips130_rf2", dict(model_dim=48, n_heads=2, feedforward_dim=48, num_layers=2, rf=2, with_layer_norm=True),
         dict(kind="mulaw", n_mlp_layers=2), 130, PARTS, 91, "M = B = 130: the tiled GEMM in the last layer and the head, N = 257 ragged"),
    Case("ff24_rf33", dict(model_dim=48, n_heads=4, feedforward_dim=24, num_layers=2, rf=33), dict(kind="mulaw", n_mlp_layers=0), 4, PARTS, 92,
         "M = 132 tiled, ff2 with K = 24: no multiple of 16"),
    Case("ff8_rf33", dict(model_dim=48, n_heads=4, feedforward_dim=8, num_layers=2, rf=33), dict(kind="mulaw", n_mlp_layers=0), 4, PARTS, 93,
         "ff2 with K = 8 < 16 falls back to the row-tile kernel between tiled GEMMs"),
    Case("frames130_rf2", dict(model_dim=32, n_heads=2, feedforward_dim=48, num_layers=1, rf=2), dict(kind="magspec", n_fft=32), 130, (19,), 94,
         "frames in and out, the input Linear at M = 260 tiled, the output Linear at M = 130"),
    Case("layer_norm_rf65", _RF65, dict(kind="mulaw", n_mlp_layers=1), 2, PARTS, 95,
         "the window across the 64-row workgroup and the 64-key tile, M = 130 tiled, split K"),
    Case("head_dim128", dict(model_dim=512, n_heads=4, feedforward_dim=512, num_layers=2, rf=32), dict(kind="mulaw", n_mlp_layers=1), 2, (16, 3), 96,
         "the largest head"),
    Case("default", dict(), dict(kind="mulaw", n_mlp_layers=1, mlp_dim=128), 2, (16, 3), 97, "the network people run: D 256, 8 heads, FF 1024, 8 layers, rf 64"),
]
BY_TAG = {c.tag: c for c in CASES}


class Life(Case):
    """One generation among several that a case's network runs on ONE plan (net_refs.lives, test_gpu_plan_lives.py): the case with its own
    clips, prompt length, blocks and draw of the prompt; the tag - and with it the networks of nets() - is the case's."""

    @property
    def prompt(self):
        return self._prompt

    def inputs(self, seed=None):
        return Case.inputs(self, self.seed + self.clips + 7919 * self.draw if seed is None else seed)

    def reached(self):
        """the steps whose window still holds prompt positions"""
        return list(range(min(self.n, self.rf)))


def _life(case, index, clips, prompt, parts, draw):
    life = Life(*Case._replace(case, clips=clips, parts=tuple(parts)))
    life.index, life._prompt, life.draw = index, prompt, draw
    return life


def of_clips(life, n):
    """the life as the envelope of `n` selected clips of its history takes it"""
    return _life(life, life.index, n, life.prompt, life.parts, life.draw)


def lives(case):
    """the four lives of net_refs.lives: the case; its clips behind a prompt 5 longer with another prompt; max(1, clips // 2 - 1) clips (130 ->
    64, 4 -> 1, 3 -> 1, 2 -> 1) behind the shortest prompt, rf (generate_block takes it: the first window starts at position 0); the case again.
    The blocks of lives 2 and 3 are the case's first five, which is all of them here (at most three)"""
    B, P = case.clips, case.prompt
    return [_life(case, 1, B, P, case.parts, 0), _life(case, 2, B, P + 5, case.parts[:5], 1),
            _life(case, 3, max(1, B // 2 - 1), case.rf, case.parts[:5], 2), _life(case, 4, B, P, case.parts, 0)]
CACHE_HIT_CASES = ("one_layer_rf9", "clips130_rf2")
SAMPLED_CASE = "clips130_rf2"


# ---- networks ------------------------------------------------------------------------------------------------------------------------------------------
def build(net_kw, io_kw, seed, gain=GAIN, device="cuda", ln_offset=0.0):
    if io_kw["kind"] == "mulaw":
        io = mmk.IOSpec.mulaw_io(mmk.IOSpec.MuLawIOConfig(input_module_type="embedding", mlp_dim=io_kw.get("mlp_dim", 32),
                                                          n_mlp_layers=io_kw["n_mlp_layers"]))
    else:
        io = mmk.IOSpec.magspec_io(mmk.IOSpec.MagSpecIOConfig(n_fft=io_kw["n_fft"], hop_length=io_kw["n_fft"] // 4))
    net = mmk.SimpleTransformer.from_config(mmk.SimpleTransformer.Config(io_spec=io, **net_kw)).eval()
    fill(net, seed, gain, ln_offset)
    return net.to(device)


def fill(net, seed, gain=GAIN, ln_offset=0.0):
    """tests/golden/make_golden_transformer.py: the recipe for every parameter, the positional-encoding table as the network made it;
    ln_offset is added to every LayerNorm weight the recipe drew"""
    sd = net.state_dict()
    shapes = {k: tuple(v.shape) for k, v in sd.items() if torch.is_floating_point(v) and v.dim() > 0 and k != "pe.pe"}
    with torch.no_grad():
        for k, v in recipe_state_dict(shapes, seed, gain).items():
            sd[k].copy_(v.to(sd[k].device))
        for k, v in sd.items():
            if ln_offset and k.startswith("model.") and ".norm" in k[5:] and k.endswith(".weight"):
                v.add_(ln_offset)


def build_case(case, device="cuda"):
    return build(case.net_kw, case.io_kw, case.seed, CASE_GAIN, device, CASE_LN_OFFSET)


@functools.lru_cache(maxsize=None)
def nets(tag):
    """(the case's network in fp32, its float64 copy), on the host"""
    case = BY_TAG[tag]
    net = build_case(case, "cpu")
    net64 = build_case(case, "cpu").double()
    net64.load_state_dict(net.state_dict())
    return net, net64


def windows_of(hist, t0, n, rf):
    """(B, T[, bins]) -> the (B n, rf[, bins]) windows ending before t0 .. t0 + n - 1"""
    w = hist.unfold(1, rf, 1)[:, t0 - rf:t0 - rf + n]          # (B, n, [bins,] rf)
    w = w.movedim(-1, 2) if hist.dim() == 3 else w
    return w.reshape(-1, rf, *hist.shape[2:]).contiguous()


def torch_outputs(net, windows, chunk=512):
    """the network's own modules, all windows of (N, rf[, bins]) in batched forwards: the raw MLP outputs (N, q + 1) or frames"""
    rf = net.rf
    mask = net._generate_square_subsequent_mask(rf).to(windows.device)
    outs = []
    with torch.no_grad():
        for w in windows.split(chunk):
            src = net.pe(net.input_module((w,)).permute(1, 0, 2).contiguous())
            h = net.model(tgt=src, memory=src, tgt_mask=mask, memory_mask=mask)[-1]
            head = net.output_modules[0]
            outs.append(head.estimator[0].fc(h) if hasattr(head, "estimator") else head(h))
    return torch.cat(outs)


def torch_outputs_f64(net64, windows):
    """torch_outputs of a float64 copy of the network on the CPU, with the mask in float64 too: given a float32 mask, torch's CPU attention
    on float64 queries is wrong from 16 keys on (off by O(1) at rf 16 and 65)"""
    mask = net64._generate_square_subsequent_mask(net64.rf).double()
    with torch.no_grad():
        src = net64.pe(net64.input_module((windows,)).permute(1, 0, 2).contiguous())
        h = net64.model(tgt=src, memory=src, tgt_mask=mask, memory_mask=mask)[-1]
        head = net64.output_modules[0]
        return head.estimator[0].fc(h) if hasattr(head, "estimator") else head(h)


# ---- the walk ------------------------------------------------------------------------------------------------------------------------------------------
# Every primitive returns (values, bound); the bound is None unless the walk carries one.  The derived bound (bound=True, float64 only): a walk
# of the network carries, next to every activation X, an elementwise bound E on |X_plan - X64|: the bound of the kernel that made X (its own
# roundings), plus the errors of its inputs carried through the first-order sensitivity of the operation.  The kernel bounds treat roundings
# as independent (u sqrt(K) for K of them); the carried errors are treated the same way, summed in quadrature (rss) rather than in magnitude -
# added in magnitude, the bound of a two-layer network is 1e8 times the error a float32 run of it shows:
#   X0         embedding + pe: one fp32 add, u |X0|;  frames: the input Linear's bound, then that add
#   Linear     E_y = Lip(act) rss_k(W_nk E_k) + gemm_bound(x, W, b)
#   attention  E_o = attention_bound(q, k, v)                                    (the kernel's own)
#                  + rss_j(w_ij (ds_ij + sum_k w_ik ds_ik) (|v_j| + |o_i|)) + rss_j(w_ij E_v_j)   (the softmax's first-order sensitivity)
#              ds_ij = scale rss_d(E_q |k_j|, |q_i| E_k) + u |x_ij|         (x = scale q.k; scale = 1/sqrtf(hd) is one rounding off)
#   add + LN   E_out = ln_bound(v) + |w| rstd (E_v + rss(E_v) / D + |d| rstd^2 rss(d E_v) / D),  v = y + res, E_v = E_y + E_res
#                                                                              (|Jacobian| of LayerNorm, d = v - mean)
def _rss_mm(E, W):
    """rss_k(W_nk E_k): E (..., K) @ W^T in quadrature"""
    return torch.sqrt((E * E) @ (W * W).t())


def _linear(x, E, W, b, act=0, acts=ACT_F):
    y = acts[act](x @ W.t() + b)
    if E is None:
        return y, None
    return y, ACT_LIP[act] * _rss_mm(E, W) + gemm_bound(x, W, b, W.shape[1], act, y)


def _attention(q, k, v, Eq, Ek, Ev, shift=0):
    """(N, rf, H, hd) causal attention over the window; shift 1 lets every row see one key too many"""
    n, hd = q.shape[1], q.shape[3]
    scale = 1.0 / math.sqrt(hd)
    vis = torch.arange(n)[None, :] <= torch.arange(n)[:, None] + shift
    x = (torch.einsum("bihd,bjhd->bhij", q, k) * scale).masked_fill(~vis, -math.inf)
    wts = torch.softmax(x, -1)
    out = torch.einsum("bhij,bjhd->bihd", wts, v)
    if Eq is None:
        return out, None
    own = attention_bound(q, k, v, out, wts, x, vis, scale)
    xv = torch.where(vis, x, torch.zeros_like(x))
    sq = lambda t: t * t   # noqa: E731
    ds = scale * torch.sqrt(torch.einsum("bihd,bjhd->bhij", sq(Eq), sq(k)) + torch.einsum("bihd,bjhd->bhij", sq(q), sq(Ek))) + U * xv.abs()
    ds = torch.where(vis, ds, torch.zeros_like(ds))
    coef = wts * (ds + (wts * ds).sum(-1, keepdim=True))
    # rss_j(coef_ij (|v_jd| + |o_id|)) <= rss_j(coef_ij |v_jd|) + rss_j(coef_ij) |o_id|
    carried = (torch.sqrt(torch.einsum("bhij,bjhd->bihd", sq(coef), sq(v))) + torch.sqrt(sq(coef).sum(-1)).permute(0, 2, 1)[..., None] * out.abs()
               + torch.sqrt(torch.einsum("bhij,bjhd->bihd", sq(wts), sq(Ev))))
    return out, own + carried


def _add_ln(y, Ey, res, Eres, w, b):
    with_res = res is not None
    v = y + res if with_res else y
    out, mean, d, var, rstd = ln_ref(v, w, b)
    if Ey is None:
        return out, None
    Ev = Ey + Eres if with_res else Ey
    own = ln_bound(v, w, with_res, out, mean, d, var, rstd)
    D = v.shape[-1]
    rss = lambda t: torch.sqrt((t * t).sum(-1, keepdim=True))   # noqa: E731
    carried = w.abs() * rstd * (Ev + rss(Ev) / D + d.abs() * rstd ** 2 * rss(d * Ev) / D)
    return out, own + carried


def _mha(P, base, xq, Exq, kv, Ekv, H, shift):
    """nn.MultiheadAttention `base` of the decoder: queries from xq, keys and values from kv"""
    D = xq.shape[-1]
    W, b = P(base + "in_proj_weight"), P(base + "in_proj_bias")
    q, Eq = _linear(xq, Exq, W[:D], b[:D])
    k, Ek = _linear(kv, Ekv, W[D:2 * D], b[D:2 * D])
    v, Ev = _linear(kv, Ekv, W[2 * D:], b[2 * D:])
    heads = lambda t: None if t is None else t.reshape(*t.shape[:2], H, D // H)   # noqa: E731
    o, Eo = _attention(heads(q), heads(k), heads(v), heads(Eq), heads(Ek), heads(Ev), shift)
    return _linear(o.reshape(xq.shape), None if Eo is None else Eo.reshape(xq.shape), P(base + "out_proj.weight"), P(base + "out_proj.bias"))


DEFECTS_IN_THE_WALK = ("leak", "query_row", "pe_shift", "kv_from_input", "no_final_norm")


def walk(net, windows, defect=None, bound=False, head_formulas=None, weights=None):
    """the network on (N, rf[, bins]) windows in the dtype of `net`: (the head's raw outputs of the last position, their derived bound or None).
    defect: one of DEFECTS_IN_THE_WALK; weights: state-dict entries that replace the network's (the weight defects); head_formulas: the
    MLP head's activation by another formula, {'mish': f, ..}"""
    assert defect is None or defect in DEFECTS_IN_THE_WALK, defect
    sd = net.state_dict()
    P = lambda name: weights[name] if weights and name in weights else sd[name]   # noqa: E731
    cfg = net.config
    rf, H, L = cfg.rf, cfg.n_heads, cfg.num_layers
    shift = 1 if defect == "leak" else 0
    first = 1 if defect == "pe_shift" else 0
    pe = P("pe.pe")[first:first + rf, 0]
    zeros = (lambda t: torch.zeros_like(t)) if bound else (lambda t: None)
    if windows.dtype == torch.int64:
        x0 = P("input_module.heads.0.0.weight")[windows] + pe
        E0 = U * x0.abs() if bound else None
    else:
        pre, E0 = _linear(windows, zeros(windows), P("input_module.heads.0.0.weight"), P("input_module.heads.0.0.bias"))
        x0 = pre + pe
        E0 = E0 + U * x0.abs() if bound else None
    x, E = x0, E0
    for l in range(L):
        base = f"model.layers.{l}."
        ln = lambda k: (P(f"{base}norm{k}.weight"), P(f"{base}norm{k}.bias"))   # noqa: E731
        xq, Exq = x, E
        if defect == "query_row" and l == L - 1:      # (the last row is the only one the outputs depend on; it sees every key either way)
            xq = x.clone()
            xq[:, -1] = x[:, -2]
            if bound:
                Exq = E.clone()
                Exq[:, -1] = E[:, -2]
        mem, Emem = (x, E) if defect == "kv_from_input" and l >= 1 else (x0, E0)
        y, Ey = _mha(P, base + "self_attn.", xq, Exq, x, E, H, shift)
        x, E = _add_ln(y, Ey, xq, Exq, *ln(1))
        y, Ey = _mha(P, base + "multihead_attn.", x, E, mem, Emem, H, shift)
        x, E = _add_ln(y, Ey, x, E, *ln(2))
        h, Eh = _linear(x, E, P(base + "linear1.weight"), P(base + "linear1.bias"), native.ACT["ReLU"])
        y, Ey = _linear(h, Eh, P(base + "linear2.weight"), P(base + "linear2.bias"))
        x, E = _add_ln(y, Ey, x, E, *ln(3))
    h, Eh = x[:, -1], (E[:, -1] if bound else None)
    if net.model.norm is not None and defect != "no_final_norm":
        h, Eh = _add_ln(h, Eh, None, None, P("model.norm.weight"), P("model.norm.bias"))
    head = net.output_modules[0]
    if hasattr(head, "estimator"):                 # MLP: Linear, act, [Linear, act] * n, Linear (the plan's raw outputs)
        acts = dict(ACT_F)
        for name, f in (head_formulas or {}).items():
            acts[native.ACT[name.capitalize()]] = f
        fc = list(head.estimator[0].fc)
        for i, m in enumerate(fc):
            if isinstance(m, torch.nn.Linear):
                nxt = fc[i + 1] if i + 1 < len(fc) else None
                key = f"output_modules.0.estimator.0.fc.{i}."
                h, Eh = _linear(h, Eh, P(key + "weight"), P(key + "bias"), 0 if nxt is None else native.ACT[type(nxt).__name__], acts)
    else:                                          # magspec: Linear, Chunk, Abs
        h, Eh = _linear(h, Eh, P("output_modules.0.0.weight"), P("output_modules.0.0.bias"), native.ACT["Abs"])
    return h, Eh


def f64_walk(net64, windows, shift=0):
    """the float64 walk with its derived bound: (the head's raw outputs of the last position, the bound); shift 1: the leaking mask"""
    return walk(net64, windows, defect="leak" if shift else None, bound=True)


# ---- the three runs --------------------------------------------------------------------------------------------------------------------------------------
def _steps(case, history):
    n = history.size(1) - case.prompt
    assert history.size(0) == case.clips and n >= 1
    return n


def reference32(case, history):
    """R32: the network's own fp32 modules, teacher-forced on `history` (clips, prompt + n[, bins]) -> (clips, n, columns)"""
    n = _steps(case, history)
    return torch_outputs(nets(case.tag)[0], windows_of(history, case.prompt, n, case.rf)).reshape(case.clips, n, -1)


def reference64(case, history, windows=None, **kw):
    """the float64 walk on `history`; kw: the walk's defect / weights"""
    n = _steps(case, history)
    w = windows_of(history, case.prompt, n, case.rf) if windows is None else windows
    w = w if case.classes else w.double()
    return walk(nets(case.tag)[1], w, **kw)[0].reshape(case.clips, n, -1)


def envelope(history, case):
    """the three teacher-forced runs on `history`: Envelope(R64, E, R32, R32k), every generated step, (clips, n, columns)"""
    n = _steps(case, history)
    R64 = reference64(case, history)
    R32 = reference32(case, history)
    R32k = walk(nets(case.tag)[0], windows_of(history, case.prompt, n, case.rf), head_formulas=N.KERNEL_FORMULAS)[0].reshape(case.clips, n, -1)
    assert R64.dtype == torch.float64 and R32.dtype == torch.float32 and R32k.dtype == torch.float32
    return Envelope(R64, torch.maximum((R32.double() - R64).abs(), (R32k.double() - R64).abs()), R32, R32k)


def walk_is_the_network(case, history):
    """the float64 walk against the network's own modules in float64: (largest difference, the outputs' scale)"""
    n = _steps(case, history)
    w = windows_of(history, case.prompt, n, case.rf)
    w = w if case.classes else w.double()
    net64 = nets(case.tag)[1]
    want = torch_outputs_f64(net64, w)
    return float((walk(net64, w)[0] - want).abs().max()), float(want.abs().max())


def derived_bound(case, history, steps=2):
    """the largest element of the bound the walk derives from the kernels' bounds, over the first `steps` steps"""
    w = windows_of(history, case.prompt, steps, case.rf)
    return float(f64_walk(nets(case.tag)[1], w if case.classes else w.double())[1].max())


def free_run(case, prompt=None):
    """the fp32 modules' own free-running history: greedy (argmax of R32 fed back), or the frames fed back"""
    net = nets(case.tag)[0]
    prompt = case.inputs() if prompt is None else prompt
    hist = torch.cat([prompt, torch.zeros(case.clips, case.n, *prompt.shape[2:], dtype=prompt.dtype)], 1)
    for t in range(case.prompt, case.prompt + case.n):
        out = torch_outputs(net, hist[:, t - case.rf:t])
        hist[:, t] = out[:, :-1].argmax(-1) if case.classes else out
    return hist


# ---- defects ---------------------------------------------------------------------------------------------------------------------------------------------
def defects(case, history, R64):
    """(name, the float64 outputs with that one defect) for every defect of the module docstring that applies to the case"""
    sd = nets(case.tag)[1].state_dict()
    L, rf = case.layers, case.rf
    n = _steps(case, history)
    key = f"model.layers.{L - 1}.self_attn.out_proj.bias"
    b = sd[key].clone()
    entry = int(b.abs().argsort()[b.numel() // 2])
    b[entry] = 0.0
    yield f"(a) entry {entry} of {key} dropped", reference64(case, history, weights={key: b})
    key = f"model.layers.{L // 2}.multihead_attn.in_proj_weight"
    yield f"(b) {key} scaled by 1 + 1e-4", reference64(case, history, weights={key: sd[key] * (1 + 1e-4)})
    swapped = R64.clone()
    swapped[-1] = R64[-2]
    yield "(c) the last clip's rows are the second-to-last clip's", swapped
    w = windows_of(history, case.prompt, n, rf).reshape(case.clips, n, rf, *history.shape[2:]).clone()
    w[0] = windows_of(history[:1], case.prompt - 1, n, rf)
    yield "(d) clip 0's window one step stale", reference64(case, history, windows=w.reshape(case.clips * n, rf, *history.shape[2:]))
    if L >= 2:
        yield "(e) a causal mask leaking one key", reference64(case, history, defect="leak")
    if rf >= 2:
        yield f"(f) the last layer's query and LN1 residual at window position {rf - 2}", reference64(case, history, defect="query_row")
    yield "(g) pe[1:rf + 1] instead of pe[0:rf]", reference64(case, history, defect="pe_shift")
    if L >= 2:
        yield "(h) cross-attention keys / values of layers >= 1 from the layer's input", reference64(case, history, defect="kv_from_input")
    if case.net_kw.get("with_layer_norm"):
        yield "(i) the final LayerNorm skipped", reference64(case, history, defect="no_final_norm")


def life_defects(life, history, R64, prev_history, prev_R64):
    """(name, the float64 outputs with that one defect, the steps it is checked on) for defects (e) and (f) of net_refs.life_defects: clip
    0's prompt is the previous life's, position by position (the steps whose window still holds prompt positions); the last clip's rows are
    the previous life's rows of the same clip index and the same steps (every step)"""
    stale = history.clone()
    stale[0, :life.prompt] = prev_history[0, :life.prompt]
    assert not torch.equal(stale, history)
    yield "(e) clip 0's prompt is the previous life's", reference64(life, stale), life.reached()
    skipped = R64.clone()
    skipped[-1] = prev_R64[life.clips - 1, :life.n]
    yield "(f) the last clip's rows are the previous life's", skipped, list(range(life.n))


def applicable(case):
    """the letters of the defects defects() yields for the case"""
    L = case.layers
    return "abcd" + ("e" if L >= 2 else "") + ("f" if case.rf >= 2 else "") + "g" + ("h" if L >= 2 else "") + ("i" if case.net_kw.get("with_layer_norm") else "")


# ---- sampled decode on the host ------------------------------------------------------------------------------------------------------------------------
def sampled_run(case, temps, uniforms, min_temp=1e-4):
    """a free run that draws every class from the FLOAT64 walk's logits by inverting the CDF of softmax(logits / T) at `uniforms` (clips, n):
    the picks an exact device would make; tests hold them against R32 under the device test's conditions"""
    from oracle import torch_ref as O
    net64 = nets(case.tag)[1]
    n = uniforms.size(1)
    prompt = case.inputs()
    hist = torch.cat([prompt, torch.zeros(case.clips, n, dtype=prompt.dtype)], 1)
    for s in range(n):
        t = case.prompt + s
        raw = walk(net64, hist[:, t - case.rf:t])[0]
        hist[:, t] = O.categorical(O.mlp_logits(raw, min_temp), temps.double(), uniforms[:, s].double())
    return hist
