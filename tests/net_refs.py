"""float64 references of the WaveNet, SampleRNN and Seq2Seq step outputs and the tolerance that derives from them, shared by
test_net_refs.py (CPU: the references against each other) and test_gpu_networks_f64.py (the device against them).

A case is one (site, geometry) pair: a network, the plan switches that select a kernel, the clips, the generate blocks.  For a history
(the classes or frames a run produced) the oracle (oracle/torch_ref.py) is run teacher-forced on it three times:

  R64   float64 weights and arithmetic
  R32   fp32, torch's (libm) activations: what the reference project computes
  R32k  fp32 with the step kernels' formulas for sigmoid, tanh and Mish (csrc/mmk_common.h: sigmoid_fast, tanh_fast, mish_fast)
        restated in plain torch - a reference-side measurement of what those formulas cost, never the device's output

E = max(|R32 - R64|, |R32k - R64|) element by element is the reference's own fp32 error on THIS history.  The tolerance of a case is
  tol_max = 4 max(E),  tol_rms = 4 rms(E)
over exactly the compared elements: twice the reference's own worst error is the project's rule for a measured constant (C_FFT in
f64_bounds.py), the second factor of two covers what the device does differently and nobody has measured (v_exp_f32 / v_rcp_f32 are
~1 ulp operations where torch.exp2 and a division stand here; the MFMA chains add in another order).

Defects are variants of the float64 run, one at a time; each must leave tol_max somewhere among the compared elements
(check_near_miss), or the envelope is too loose to see what a kernel really gets wrong:
  (a) one bias entry dropped (the one of median magnitude: a typical entry, neither tame nor extreme): a recurrent bias_hh for SampleRNN and
      Seq2Seq, a conv_skip.bias for WaveNet
  (b) the weights of one layer scaled by 1 + 1e-4
  (c) the last clip's rows replaced by the second-to-last clip's (a ragged tile that reads its neighbour)
  (d) one clip's window one step stale
"""
import functools
from typing import NamedTuple

import numpy as np
import torch

import mimikit_amd as mmk
from oracle import torch_ref as O
from oracle.weights import load_recipe
from tests import helpers as H

FACTOR = 4.0
LOG2E = 1.4426950408889634


# ---- the kernels' formulas in plain torch (csrc/mmk_common.h) ---------------------------------------------------------------------------------------
def k_sigmoid(x):
    """sigmoid_fast: 1 / (1 + 2^(-x log2 e))"""
    return 1.0 / (1.0 + torch.exp2(x * -LOG2E))


def k_tanh(x):
    """tanh_fast: 2 sigmoid(2 x) - 1"""
    return 2.0 * (1.0 / (1.0 + torch.exp2(x * (-2.0 * LOG2E)))) - 1.0


def k_mish(x):
    """mish_fast: x n / (n + 2), n = e (e + 2), e = exp(min(x, 20)); x beyond 20"""
    e = torch.exp(torch.clamp(x, max=20.0))
    n = e * (e + 2.0)
    return torch.where(x > 20.0, x, x * (n / (n + 2.0)))


KERNEL_FORMULAS = dict(sigmoid=k_sigmoid, tanh=k_tanh, mish=k_mish)


# ---- networks ------------------------------------------------------------------------------------------------------------------------------------------
def _wavenet(C, blocks, mlp_dim, seed, cond_dims=()):
    io = H.mu_emb(mlp_dim=mlp_dim)
    kw = {}
    if cond_dims:
        ext = mmk.Extractor("signal", mmk.FileToSignal(16000))
        extra = tuple(mmk.InputSpec("signal", mmk.MagSpec(22, 4, center=False), mmk.LinearIO()).bind_to(ext) for _ in cond_dims)
        io = mmk.IOSpec(inputs=(io.inputs[0], *extra), targets=io.targets)
        kw["dims_1x1"] = tuple(cond_dims)
    net = mmk.WaveNet.from_config(mmk.WaveNet.Config(io_spec=io, blocks=blocks, dims_dilated=(C,), residuals_dim=C, skips_dim=C, **kw)).eval()
    sd = load_recipe(net, seed=seed, gain=2.0)
    dil = [2 ** i for b in blocks for i in range(b)]
    return net, sd, dict(kernels=[2] * len(dil), dilations=dil, has_skips=True, residuals=True)


def _srnn(kind, hidden, frame_sizes, seed, q=256, mlp_dim=128, n_rnn=1):
    net = mmk.SampleRNN.from_config(mmk.SampleRNN.Config(io_spec=H.mu_lin(mlp_dim=mlp_dim, q_levels=q), frame_sizes=frame_sizes, hidden_dim=hidden,
                                                         rnn_class=kind, n_rnn=n_rnn)).eval()
    sd = load_recipe(net, seed=seed, gain=2.0)
    return net, sd, dict(frame_sizes=frame_sizes, hidden_dim=hidden, rnn_class=kind, q_levels=q, n_rnn=n_rnn)


def _s2s(dim, hop, layers, seed, res=False, ds="edge_sum", us="linear_resample"):
    io = mmk.IOSpec.magspec_io(mmk.IOSpec.MagSpecIOConfig(n_fft=128, hop_length=32))
    cfg = mmk.Seq2SeqLSTMNetwork.Config(io_spec=io, model_dim=dim, hop=hop, enc_n_lstm=layers, dec_n_lstm=layers, enc_apply_residuals=res,
                                        dec_apply_residuals=res, enc_downsampling=ds, dec_upsampling=us)
    net = mmk.Seq2SeqLSTMNetwork.from_config(cfg).eval()
    sd = load_recipe(net, seed=seed, gain=1.5)
    return net, sd, dict(downsampling=ds, upsampling=us, enc_residuals=res, dec_residuals=res)


def _s2s_classes():
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        net, sd, hop, arch = H.s2s_mulaw("mlp0", model_dim=128, mlp_dim=128)
    assert hop == 4
    return net, sd, arch


# ---- what the plan must report after every block: the kernel the case means to cover ran ----------------------------------------------------
ONE_CLIP, FOUR_CLIPS, LAUNCHES = 1, 2, 3      # mmk_srnn_bottom_kernel (include/mmk.h)


def _wn_launches(p, k):
    return not p.persistent


def _wn_persist(p, k):
    return p.persistent and not p.chain and not p.layer_pipelined and not p.stage_pipelined


def _wn_chain(p, k):
    return p.chain


def _wn_lpipe(p, k):
    return p.layer_pipelined


def _wn_spipe(p, k):
    return p.stage_pipelined and not p.batch_pipelined and not p.pair_visits


def _wn_spipe_pair(p, k):
    return p.stage_pipelined and not p.batch_pipelined and p.pair_visits


def _wn_bpipe(p, k):
    return p.stage_pipelined and p.batch_pipelined


def _bottom(kernel):
    return lambda p, k: p.resident_blocks() == 0 and p.bottom_kernel() == kernel


def _resident(warmups=None):
    return lambda p, k: p.resident_blocks() == k and (warmups is None or p.resident_warmups() == warmups)


def _s2s_resident(layers):
    return lambda p, k: p.resident_launches() == k * 2 * layers


def _s2s_per_frame(p, k):
    return p.resident_launches() == 0


class Case:
    """kind: 'wavenet' | 'wavenet_frames' | 'srnn' | 's2s' | 's2s_classes'; make() -> (net, state dict, the oracle's keywords); env: the plan
    switches; parts: the lengths of the consecutive generate_block calls (Seq2Seq: steps of `hop` frames per call); ran(plan, blocks so far)"""

    def __init__(self, id, kind, make, clips, parts, env, ran, cond=0, hop=None, seed=0, forced_split=None):
        self.id, self.kind, self._make, self.clips, self.parts, self.env, self.ran = id, kind, make, clips, tuple(parts), dict(env), ran
        self.cond, self.hop, self.seed = cond, hop, seed
        # split-K cases: (rows, columns, K, forced split) of the tiled GEMM the switch reaches; the plan reports nothing about it, so the
        # device test also runs the case without the switch and requires other bits in the first step's frames
        self.forced_split = forced_split

    def make(self):
        return self._make()

    @functools.cached_property
    def host(self):
        """(state dict, the oracle's keywords) - the recipe's weights are the same in every network make() builds"""
        _, sd, arch = self._make()
        return sd, arch

    sd = property(lambda self: self.host[0])
    arch = property(lambda self: self.host[1])

    @property
    def n(self):
        return sum(self.parts) * (self.hop or 1)

    @property
    def classes(self):
        return self.kind in ("wavenet", "srnn", "s2s_classes")

    def rows(self):
        """the steps whose outputs the device hands back: every frame of a frame network, every step of the Seq2Seq class path (last_logits holds
        the `hop` rows of a step), the last step of each block otherwise"""
        if self.kind in ("wavenet", "srnn"):
            ends, t = [], 0
            for nb in self.parts:
                t += nb
                ends.append(t - 1)
            return ends
        return list(range(self.n))

    @property
    def P(self):
        arch = self.arch
        if self.kind in ("wavenet", "wavenet_frames"):
            return O.wavenet_rf(arch["kernels"], arch["dilations"]) + 3
        if self.kind == "srnn":
            return 2 * arch["frame_sizes"][0] + 3
        return self.hop

    def inputs(self):
        """the prompt and the conditioning inputs of the case (fp32 / int64, on the host)"""
        g = torch.Generator().manual_seed(1000 + self.seed + self.clips)
        P = self.P
        if self.kind == "wavenet_frames":
            return torch.rand(self.clips, P, 33, generator=g), ()
        if self.kind == "s2s":
            return torch.rand(self.clips, P, 65, generator=g), ()
        prompt = torch.randint(0, 256, (self.clips, P), generator=g)
        return prompt, tuple(torch.rand(self.clips, P + self.n, 12, generator=g) for _ in range(self.cond))


WN_PARTS = (1, 2, 3, 4, 5, 6, 7, 8, 9)                        # 45 steps, nine rows per clip, block ends on every small ring phase
SRNN_PARTS = (1, 2, 3, 4, 5, 6, 7, 8, 9, 17, 16)              # outside resident mode: 78 steps
# resident mode: every block at least two periods long (a head of up to fs0 - 1 steps runs with the kernels in turns, the launch takes over at the
# next multiple of fs0), block ends (absolute position, prompt 2 fs0 + 3) on the residues 15, 0, 1, 2 mod 16 and 31, 0, 1, 2 mod 32
RES_PARTS_16 = (44, 33, 33, 33)                               # from 35: 79, 112, 145, 178
RES_PARTS_32 = (92, 65, 65, 65)                               # from 67: 159, 224, 289, 354
_SP = {"MMK_WN_SPIPE": "1", "MMK_WN_BPIPE": "0"}
_NR = {"MMK_SRNN_RESIDENT": "0"}

WAVENET_CASES = [
    Case("launches", "wavenet", lambda: _wavenet(32, (3, 2), 32, 21), 5, WN_PARTS, {"MMK_WN_PERSISTENT": "0"}, _wn_launches),
    Case("persist", "wavenet", lambda: _wavenet(32, (3, 2), 32, 21), 5, WN_PARTS, {"MMK_WN_CHAIN": "0"}, _wn_persist),
    Case("chain", "wavenet", lambda: _wavenet(32, (3, 2), 32, 21), 5, WN_PARTS, {}, _wn_chain),
    Case("chain-cond", "wavenet", lambda: _wavenet(32, (3, 2), 32, 22, (16,)), 5, WN_PARTS, {}, _wn_chain, cond=1),
    Case("chain-step_warmup", "wavenet", lambda: _wavenet(32, (3, 2), 32, 21), 5, WN_PARTS, {"MMK_WN_PREFILL": "0"}, _wn_chain),
    Case("lpipe-4_3-13", "wavenet", lambda: _wavenet(64, (4, 3), 128, 62), 13, WN_PARTS, {}, _wn_lpipe),
    Case("lpipe-10-8", "wavenet", lambda: _wavenet(64, (10,), 128, 61), 8, WN_PARTS, {}, _wn_lpipe),
    Case("lpipe-cond", "wavenet", lambda: _wavenet(64, (4, 3), 128, 72, (16,)), 13, WN_PARTS, {}, _wn_lpipe, cond=1),
    Case("spipe-5", "wavenet", lambda: _wavenet(256, (3,), 128, 306), 5, WN_PARTS, _SP, _wn_spipe),
    Case("spipe-cond", "wavenet", lambda: _wavenet(256, (3,), 128, 307, (16,)), 5, WN_PARTS, _SP, _wn_spipe, cond=1),
    Case("spipe-pair-24", "wavenet", lambda: _wavenet(256, (3,), 128, 306), 24, WN_PARTS, {**_SP, "MMK_WN_SPIPE_PAIR": "1"}, _wn_spipe_pair),
    Case("bpipe-20", "wavenet", lambda: _wavenet(256, (3,), 128, 306), 20, WN_PARTS, {"MMK_WN_SPIPE": "1", "MMK_WN_BPIPE": "1"}, _wn_bpipe),
    # (real-valued frames in and out: no persistent kernel takes them, csrc/wavenet_plan.hip)
    Case("frames-g4", "wavenet_frames", lambda: H.freqnet("g4"), 5, WN_PARTS, {}, _wn_launches),
]

SRNN_CASES = [
    Case("launches", "srnn", lambda: _srnn("gru", 128, (16, 4, 1), 78), 21, SRNN_PARTS, {**_NR, "MMK_SRNN_FUSED": "0"}, _bottom(LAUNCHES)),
    Case("bottom-one_clip", "srnn", lambda: _srnn("gru", 128, (16, 4, 1), 78), 21, SRNN_PARTS, {**_NR, "MMK_SRNN_FUSED": "1"}, _bottom(ONE_CLIP)),
    Case("bottom-four_clips-321", "srnn", lambda: _srnn("gru", 128, (16, 4, 1), 78, q=321, mlp_dim=64), 21, SRNN_PARTS,
         {**_NR, "MMK_SRNN_FUSED": "1"}, _bottom(FOUR_CLIPS)),
    Case("tier-up_apart", "srnn", lambda: _srnn("lstm", 128, (16, 4, 1), 77), 21, SRNN_PARTS,
         {**_NR, "MMK_SRNN_FUSED": "1", "MMK_SRNN_FUSED_UP": "0"}, _bottom(ONE_CLIP)),
    Case("rnn_tanh", "srnn", lambda: _srnn("rnn", 128, (16, 4, 1), 80), 5, SRNN_PARTS, {"MMK_SRNN_FUSED": "1"}, _bottom(ONE_CLIP)),
    Case("n_rnn_2", "srnn", lambda: _srnn("gru", 128, (16, 4, 1), 81, n_rnn=2), 5, SRNN_PARTS, {"MMK_SRNN_FUSED": "1"}, _bottom(ONE_CLIP)),
    Case("resident-gru", "srnn", lambda: _srnn("gru", 128, (16, 4, 1), 83), 21, RES_PARTS_16, {"MMK_SRNN_FUSED": "1"}, _resident()),
    Case("resident-lstm", "srnn", lambda: _srnn("lstm", 128, (16, 4, 1), 83), 21, RES_PARTS_16, {"MMK_SRNN_FUSED": "1"}, _resident()),
    Case("resident-32_8_2-33", "srnn", lambda: _srnn("gru", 128, (32, 8, 2), 91), 33, RES_PARTS_32, {"MMK_SRNN_FUSED": "1"}, _resident()),
    Case("resident-gru-512-40", "srnn", lambda: _srnn("gru", 512, (16, 4, 1), 79), 40, RES_PARTS_16, {"MMK_SRNN_FUSED": "1"}, _resident()),
    Case("resident-warmup_1", "srnn", lambda: _srnn("lstm", 128, (16, 4, 1), 85), 21, RES_PARTS_16,
         {"MMK_SRNN_FUSED": "1", "MMK_SRNN_RESIDENT_WARMUP": "1"}, _resident(1)),
    Case("resident-warmup_0", "srnn", lambda: _srnn("lstm", 128, (16, 4, 1), 85), 21, RES_PARTS_16,
         {"MMK_SRNN_FUSED": "1", "MMK_SRNN_RESIDENT_WARMUP": "0"}, _resident(0)),
]


def _s2s_case(tag, dim, hop, clips, layers, env, ran, forced_split=None, **kw):
    return Case(tag, "s2s", lambda: _s2s(dim, hop, layers, 7 + dim + hop, **kw), clips, (1, 1, 1), env, ran, hop=hop, forced_split=forced_split)


def gemm_k_split(M, N, K, forced=0):
    """csrc/gemm.hip, gemm_bias_act_k_split, restated: (the K split a launch of the tiled GEMM takes, its pipeline stages).  Tiles of 64 x 64,
    stages of 4 K-chunks of 16; unforced, K is halved while the grid stays within 512 workgroups; a forced split is clamped to the stages"""
    n_tiles, k_chunks = -(-N // 16), -(-K // 16)
    wgs = -(-n_tiles // 4) * -(-M // 64)
    stages = -(-k_chunks // 4)
    ks = 1
    while ks * 2 <= stages and wgs * ks * 2 <= 512 and ks < 8:
        ks *= 2
    return (min(forced, stages) if forced > 0 else ks), stages


S2S_CASES = [
    _s2s_case("resident-128-2-3", 128, 2, 3, 1, {}, _s2s_resident(1)),
    _s2s_case("resident-256-5-17", 256, 5, 17, 1, {}, _s2s_resident(1)),
    _s2s_case("resident-512-3-33", 512, 3, 33, 1, {}, _s2s_resident(1)),
    _s2s_case("resident-128-7-128", 128, 7, 128, 1, {}, _s2s_resident(1)),
    _s2s_case("resident-128-8-16-2layers", 128, 8, 16, 2, {}, _s2s_resident(2)),
    _s2s_case("resident-128-8-16-2layers-residuals", 128, 8, 16, 2, {}, _s2s_resident(2), res=True),
    _s2s_case("per_frame", 128, 8, 16, 2, {"MMK_S2S_SEQ": "0"}, _s2s_per_frame),
    _s2s_case("launches", 128, 8, 16, 2, {"MMK_S2S_FUSED": "0"}, _s2s_per_frame),
    # split K: in resident mode the bi-LSTM input projections have a kernel of their own, the switch reaches the output projection
    # (batch x hop = 128 rows, 65 columns, K = model_dim).  At model_dim 256 that GEMM has four stages and splits four ways by itself, so a
    # forced 2 and a forced 3 (uneven: 2 + 1 + 1 stages) are both honoured and both differ from the default - at model_dim 128 (two stages)
    # a forced 3 would be clamped to 2, which is the default there (test_net_refs.py asserts this arithmetic)
    _s2s_case("ksplit-2", 256, 8, 16, 1, {"MMK_GEMM_KSPLIT": "2"}, _s2s_resident(1), forced_split=(128, 65, 256, 2)),
    _s2s_case("ksplit-3", 256, 8, 16, 1, {"MMK_GEMM_KSPLIT": "3"}, _s2s_resident(1), forced_split=(128, 65, 256, 3)),
    _s2s_case("mean-repeat", 128, 8, 16, 1, {}, _s2s_resident(1), ds="mean", us="repeat"),
    Case("classes", "s2s_classes", _s2s_classes, 24, (1, 1, 1), {}, _s2s_resident(1), hop=4),
]

ALL_CASES = [("wavenet", c) for c in WAVENET_CASES] + [("srnn", c) for c in SRNN_CASES] + [("s2s", c) for c in S2S_CASES]


# ---- the oracle, teacher-forced ----------------------------------------------------------------------------------------------------------------------
def to64(sd):
    return {k: (v.double() if torch.is_floating_point(v) else v) for k, v in sd.items()}


def reference(case, sd, hist, conds=()):
    """the oracle's outputs of the case's n generated steps on the history `hist` (prompt + n steps), in the dtype of `sd`: raw head outputs
    (clips, n, classes + 1) or frames (clips, n, bins)"""
    n, P, arch = case.n, case.P, case.arch
    sd = O.fold_weight_norm(sd)                    # (in the dtype of `sd`; the Seq2Seq decoder with residuals is weight-normed)
    if case.kind in ("wavenet", "wavenet_frames"):
        rf = P - 3
        lo, hi = P - rf, P + n - 1                 # ONE forward over the n windows: output j belongs to the window that starts at lo + j
        kw = dict(arch, embedding=False) if case.kind == "wavenet_frames" else arch
        return O.wavenet_window_forward(sd, (hist[:, lo:hi], *[c[:, lo:hi] for c in conds]), n_cond=len(conds), every_position=True, **kw)
    if case.kind == "srnn":
        return O.SampleRNNOracle(sd, **arch).generate(hist[:, :P], n, keep_logits=True, forced=hist)[1]
    outs = []
    for t in range(P, P + n, case.hop):
        x = hist[:, t - case.hop:t]
        outs.append(O.s2s_step(sd, x, case.hop, return_raw=True, **arch)[1] if case.kind == "s2s_classes" else O.s2s_step(sd, x, case.hop, **arch))
    return torch.cat(outs, 1)


def free_run(case, prompt, conds=()):
    """the fp32 oracle's own free-running history"""
    sd, arch = O.fold_weight_norm(case.sd), case.arch
    if case.kind == "wavenet":
        return O.wavenet_generate(sd, prompt, conds, case.n, **arch)
    if case.kind == "wavenet_frames":
        return O.wavenet_generate_frames(sd, prompt, case.n, **arch)
    if case.kind == "srnn":
        return O.SampleRNNOracle(sd, **arch).generate(prompt, case.n)
    out = O.s2s_generate(sd, prompt, case.n, case.hop, **arch)
    return out.long() if case.kind == "s2s_classes" else out


class Envelope(NamedTuple):
    R64: torch.Tensor
    E: torch.Tensor
    R32: torch.Tensor
    R32k: torch.Tensor


def envelope(history, case, conds=()):
    """the three teacher-forced runs on `history`: (R64, E, R32, R32k), every generated step"""
    sd = case.sd
    R64 = reference(case, to64(sd), history, conds)
    R32 = reference(case, sd, history, conds)
    with O.activation_formulas(**KERNEL_FORMULAS):
        R32k = reference(case, sd, history, conds)
    assert R64.dtype == torch.float64 and R32.dtype == torch.float32 and R32k.dtype == torch.float32
    return Envelope(R64, torch.maximum((R32.double() - R64).abs(), (R32k.double() - R64).abs()), R32, R32k)


def rms(x):
    return float(x.double().pow(2).mean().sqrt())


def tolerance(E):
    """(tol_max, tol_rms) of the compared elements' E"""
    return FACTOR * float(E.max()), FACTOR * rms(E)


def ratios(dev, R64, E):
    """max|dev - R64| / max(E) and rms(dev - R64) / rms(E): records (the margin allows FACTOR), never tolerances"""
    err = dev.double() - R64
    return float(err.abs().max()) / float(E.max()), rms(err) / rms(E)


def check_outputs(dev, R64, tol_max, tol_rms, what):
    err = (dev.double() - R64).abs()
    bad = ~(err <= tol_max)
    if bool(bad.any()):
        i = tuple(int(v) for v in np.unravel_index(int(torch.where(bad, err.nan_to_num(nan=float("inf")), -torch.ones_like(err)).argmax()), err.shape))
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} elements outside the envelope; worst at {i}: got {float(dev[i]):.9g}, want "
                             f"{float(R64[i]):.9g}, error {float(err[i]):.3e} > tol_max {tol_max:.3e}")
    assert rms(err) <= tol_rms, f"{what}: rms error {rms(err):.3e} > tol_rms {tol_rms:.3e} (largest error {float(err.max()):.3e}, tol_max {tol_max:.3e})"


def check_picks(picks, R64, tol_max, what="picks"):
    """a greedy pick p of a step is right iff R64[p] >= max(R64 over the classes) - 2 tol_max (both ends of the comparison may be off by
    tol_max); the temperature column is no class (helpers.margin_ok).  Every step of every clip, no excluded share."""
    cls = R64[..., :-1]
    picks = picks.long()
    inside = (picks >= 0) & (picks < cls.shape[-1])
    assert bool(inside.all()), f"{what}: {int((~inside).sum())} picks are no class"
    gap = cls.max(-1).values - cls.gather(-1, picks.unsqueeze(-1)).squeeze(-1)
    bad = ~(gap <= 2 * tol_max)
    if bool(bad.any()):
        i = tuple(int(t[0]) for t in bad.nonzero(as_tuple=True))
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} picks are not the float64 argmax within 2 tol_max; at {i}: class {int(picks[i])} lies "
                             f"{float(gap[i]):.3e} below the best, 2 tol_max = {2 * tol_max:.3e}")


def check_near_miss(defect, R64, tol_max, what):
    """the float64 run with one defect must leave tol_max somewhere among the compared elements (NaN counts as leaving it)"""
    assert bool((~((defect - R64).abs() <= tol_max)).any()), \
        f"{what}: the defect moves the outputs by at most {float((defect - R64).abs().max()):.3e}, inside tol_max {tol_max:.3e} - the envelope is too loose"


def _keys(case, sd):
    arch = case.arch
    if case.kind in ("wavenet", "wavenet_frames"):
        L = len(arch["kernels"])
        bias = "layers.0.conv_skip.bias" if "layers.0.conv_skip.bias" in sd else \
            next(k for k in sd if k.startswith("layers.0.conv_dil") and k.endswith("bias"))
        return bias, next(k for k in sd if k.startswith(f"layers.{L // 2}.conv_dil") and k.endswith("weight"))
    if case.kind == "srnn":
        return "tiers.0.rnn.bias_hh_l0", "tiers.0.rnn.weight_hh_l0"
    return "dec.lstm.0.bias_hh_l0_reverse", "dec.lstm.0.weight_hh_l0"


def bias_dropped(case, history, conds, entry=None):
    """defect (a): (name, the float64 outputs) with entry `entry` of the case's bias vector zeroed - by default the one of median magnitude"""
    sd64 = O.fold_weight_norm(to64(case.sd))
    bias_key, _ = _keys(case, sd64)
    b = sd64[bias_key].clone()
    entry = int(b.abs().argsort()[b.numel() // 2]) if entry is None else entry
    b.view(-1)[entry] = 0.0
    return f"(a) entry {entry} of {bias_key} dropped", reference(case, {**sd64, bias_key: b}, history, conds)


def defects(case, history, conds, R64):
    """(name, the float64 outputs with that one defect) for the four defects of the module docstring"""
    sd64 = O.fold_weight_norm(to64(case.sd))
    _, weight_key = _keys(case, sd64)
    yield bias_dropped(case, history, conds)
    yield f"(b) {weight_key} scaled by 1 + 1e-4", reference(case, {**sd64, weight_key: sd64[weight_key] * (1 + 1e-4)}, history, conds)
    c = R64.clone()
    c[-1] = R64[-2]
    yield "(c) the last clip's rows are the second-to-last clip's", c
    stale = history.clone()
    stale[0, 1:] = history[0, :-1]
    yield "(d) clip 0's window one step stale", reference(case, sd64, stale, conds)
