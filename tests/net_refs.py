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
  (b) the weights of one layer scaled by 1 + 1e-4: the dilated convolution of the middle layer (WaveNet), the decoder's first recurrent
      matrix (Seq2Seq); for SampleRNN, by one rule for every case, the recurrent matrix weight_hh of the LAST stacked layer of the tier right
      above the bottom - the tier that steps most often and the layer whose state the up-sampler reads, so the scaled product is taken once per
      frame of that tier and reaches the compared row through one up-sampler only (tier 0's first layer, the choice before the option cases,
      steps fs0 / fs[-2] times less often and, under stacked layers, is damped by every layer above it: at frame sizes 16, 8, 8 with three
      stacked LSTM layers it moved the compared rows by 0.15 tol_max, the rule's choice moves them by 7 tol_max)
  (c) the last clip's rows replaced by the second-to-last clip's (a ragged tile that reads its neighbour)
  (d) one clip's window one step stale

The option cases (WAVENET_OPTION_CASES, WAVENET_HEAD_CASES, MULTI_CASES, SRNN_OPTION_CASES, S2S_OPTION_CASES: every network option the plans
branch on, on the per-layer launch path or the padded heads of the pipelines) add option defects, one per option of the case (the opt_*
generators below; each says which device mistake it stands for).  They too are float64 variants, expressed through the state dict, the inputs
or the oracle's keywords only, and each must leave tol_max.  A network of several targets has one output tensor, one E and one tolerance per
target; a defect has left the envelope when it leaves tol_max of any one target.

Lives (Life, lives, life_defects): the generations test_gpu_plan_lives.py runs on ONE plan - the case, then its clips behind a prompt 5
longer with other inputs, then fewer clips behind the shortest prompt, then the case again.  A life is a view of its case with its own clips,
prompt length, blocks and draw of the inputs; every function here that takes a case takes a life.  Their defects - (e) a prompt, (f) a ragged
group's rows, (g) SampleRNN tier states of the life BEFORE - stand for what a reused workspace can do, and each must leave tol_max too.
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
def _wavenet(C, blocks, mlp_dim, seed, cond_dims=(), q=256):
    io = H.mu_emb(mlp_dim=mlp_dim, q_levels=q)
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


def _s2s_classes(tag="mlp0", hop=4):
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        net, sd, got, arch = H.s2s_mulaw(tag, model_dim=128, mlp_dim=128)
    assert got == hop
    return net, sd, arch


def _s2s_stack(tag, dim, hop, seed, inputs=1):
    """a network of helpers.S2S_STACKS (or the plain one, tag None) at another width and hop, with `inputs` magnitude-frame inputs added up"""
    import warnings
    kw = dict(H.S2S_STACKS[tag]) if tag else {}
    io = mmk.IOSpec.magspec_io(mmk.IOSpec.MagSpecIOConfig(n_fft=128, hop_length=32))
    io = mmk.IOSpec(inputs=(io.inputs[0],) * inputs, targets=io.targets)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        net = mmk.Seq2SeqLSTMNetwork.from_config(mmk.Seq2SeqLSTMNetwork.Config(io_spec=io, model_dim=dim, hop=hop, **kw)).eval()
    sd = load_recipe(net, seed=seed, gain=1.5)
    return net, sd, dict(downsampling=kw.get("enc_downsampling", "edge_sum"), enc_residuals=kw.get("enc_apply_residuals", False),
                         dec_residuals=kw.get("dec_apply_residuals", False))


def _no_n_cond(made):
    """the helpers' (net, state dict, keywords) with the `n_cond` the oracle's callers pass themselves taken out of the keywords"""
    net, sd, arch = made
    arch = dict(arch)
    arch.pop("n_cond", None)
    return net, sd, arch


def _mlp_head(tag):
    net, sd, _, arch = H.mlp_head_case(tag)
    return net, sd, arch


def _multi_io(tag):
    """helpers.multi_io with the oracle's keywords as one dict: a WaveNet's kernels and dilations beside the others"""
    net, sd, arch, _ = H.multi_io(tag)
    if not isinstance(arch, dict):
        ks, ds, kw = arch
        arch = dict(kw, kernels=ks, dilations=ds)
    return net, sd, arch


# ---- what the plan must report after every block: the kernel the case means to cover ran ----------------------------------------------------
ONE_CLIP, FOUR_CLIPS, LAUNCHES = 1, 2, 3      # mmk_srnn_bottom_kernel (include/mmk.h)


# ran(plan, k, w=1): k counts the generate blocks (Seq2Seq: steps) the plan has run in its whole life; w the generations among them whose
# warm-up was whole periods long (SampleRNN: the only ones a resident warm-up launch can take) - one generation, as in test_gpu_networks_f64.py: 1
def _wn_launches(p, k, w=1):
    return not p.persistent


def _wn_persist(p, k, w=1):
    return p.persistent and not p.chain and not p.layer_pipelined and not p.stage_pipelined


def _wn_chain(p, k, w=1):
    return p.chain


def _wn_lpipe(p, k, w=1):
    return p.layer_pipelined


def _wn_spipe(p, k, w=1):
    return p.stage_pipelined and not p.batch_pipelined and not p.pair_visits


def _wn_spipe_pair(p, k, w=1):
    return p.stage_pipelined and not p.batch_pipelined and p.pair_visits


def _wn_bpipe(p, k, w=1):
    return p.stage_pipelined and p.batch_pipelined


def _bottom(kernel):
    return lambda p, k, w=1: p.resident_blocks() == 0 and p.bottom_kernel() == kernel


def _resident(warmups=None):
    return lambda p, k, w=1: p.resident_blocks() == k and (warmups is None or p.resident_warmups() == warmups * w)


def _s2s_resident(layers, dec=None):
    """every bi-LSTM layer of every step as one resident launch: `layers` per side, or `layers` in the encoder and `dec` in the decoder"""
    return lambda p, k, w=1: p.resident_launches() == k * (layers + (layers if dec is None else dec))


def flags(case, p):
    """what the plan reports about the kernels it took, for the record a test prints"""
    if case.kind in ("wavenet", "wavenet_frames"):
        return {n: bool(getattr(p, n)) for n in ("persistent", "chain", "layer_pipelined", "stage_pipelined", "batch_pipelined", "pair_visits")}
    if case.kind == "srnn":
        return dict(bottom_kernel=p.bottom_kernel(), resident_blocks=p.resident_blocks(), resident_warmups=p.resident_warmups())
    return dict(resident_launches=p.resident_launches())


def streams(x):
    """a tuple of tensors as it is, one tensor as a tuple of one"""
    return tuple(x) if isinstance(x, (tuple, list)) else (x,)


def _s2s_per_frame(p, k, w=1):
    return p.resident_launches() == 0


class Case:
    """kind: 'wavenet' | 'wavenet_frames' | 'srnn' | 's2s' | 's2s_classes'; make() -> (net, state dict, the oracle's keywords); env: the plan
    switches; parts: the lengths of the consecutive generate_block calls (Seq2Seq: steps of `hop` frames per call); ran(plan, blocks so far);
    cond: real-valued inputs beside the first (WaveNet: conditioning features, Seq2Seq: further frame inputs the network adds up), given for
    the whole length; q: the class count of every class stream (one entry: the prompt's; several: a network of several class inputs, the
    first `targets` of which the loop writes and the others of which are given for the whole length); options: the case's option defects"""

    def __init__(self, id, kind, make, clips, parts, env, ran, cond=0, hop=None, seed=0, forced_split=None, q=(256,), targets=1, options=()):
        self.id, self.kind, self._make, self.clips, self.parts, self.env, self.ran = id, kind, make, clips, tuple(parts), dict(env), ran
        self.cond, self.hop, self.seed = cond, hop, seed
        self.q, self.targets, self.options = tuple(q), targets, tuple(options)
        self.multi = len(self.q) > 1              # histories and outputs are tuples: one stream per class input, one output per target
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

    draw = 0          # which draw of the inputs (a Life: its own)

    @property
    def shortest_prompt(self):
        """the shortest prompt the network takes: the receptive field (the WaveNet warm-up then starts at position 0), frame_sizes[0], or
        the `hop` frames a Seq2Seq step reads.  The oracle and the networks accept it for every case: no life needed another length."""
        arch = self.arch
        if self.kind in ("wavenet", "wavenet_frames"):
            return O.wavenet_rf(arch["kernels"], arch["dilations"])
        return arch["frame_sizes"][0] if self.kind == "srnn" else self.hop

    def inputs(self, life=None):
        """the prompt and the conditioning inputs of the case - or of `life`, a Life of it - (fp32 / int64, on the host)"""
        if life is not None:
            assert life.case is self
            return life.inputs()
        g = torch.Generator().manual_seed(1000 + self.seed + self.clips + 7919 * self.draw)
        P = self.P
        if self.kind == "wavenet_frames":
            return torch.rand(self.clips, P, 33, generator=g), ()
        if self.kind == "s2s":
            return torch.rand(self.clips, P, 65, generator=g), tuple(torch.rand(self.clips, P + self.n, 65, generator=g) for _ in range(self.cond))
        if self.multi:
            return tuple(torch.randint(0, q, (self.clips, P if k < self.targets else P + self.n), generator=g) for k, q in enumerate(self.q)), ()
        prompt = torch.randint(0, self.q[0], (self.clips, P), generator=g)
        return prompt, tuple(torch.rand(self.clips, P + self.n, 12, generator=g) for _ in range(self.cond))


def spipe_pair_form(clips, forced=True):
    """csrc/wavenet_spipe.h, wn_spipe_pair_form, restated for a forced MMK_WN_SPIPE_PAIR=1: the ring takes two clips per visit for an even
    count of 24 .. 128 clips - of the CALL, not of the plan: a plan made for 24 clips serves 11 of them one clip per visit"""
    return forced and clips % 2 == 0 and 24 <= clips <= 128


class Life(Case):
    """One generation among several that a case's network runs on ONE plan (test_gpu_plan_lives.py): a view of the case with its own clips,
    prompt length P, blocks and draw of the inputs.  The network, the state dict, the oracle's keywords, `env` and `ran` are the case's - but
    for the one flag that follows the call's batch instead of the plan's (spipe_pair_form).  inputs(), reference(), free_run(), envelope()
    and defects() take a life wherever they take a case."""

    def __init__(self, case, index, clips, P, parts, draw):
        vars(self).update({k: v for k, v in vars(case).items() if k != "host"})
        self.case, self.index, self.clips, self.parts, self.draw, self._P = case, index, clips, tuple(parts), draw, P
        if case.ran is _wn_spipe_pair and not spipe_pair_form(clips):
            self.ran = _wn_spipe

    host = property(lambda self: self.case.host)
    P = property(lambda self: self._P)

    @property
    def whole_period_warmup(self):
        """SampleRNN: the warm-up runs the tiers over [fs0, P - P % fs0): at least one whole period, which a resident warm-up launch can take"""
        fs0 = self.arch["frame_sizes"][0]
        return self.P - self.P % fs0 - fs0 >= fs0

    def reached(self):
        """the indices into rows() of the steps a teacher-forced reference still computes from the prompt: the window of step j holds prompt
        positions while j < rf; a Seq2Seq step reads the `hop` frames before it; a SampleRNN tier state carries the prompt without end"""
        if self.kind == "srnn":
            return list(range(len(self.rows())))
        return [i for i, r in enumerate(self.rows()) if r < self.shortest_prompt]


def life_parts(case):
    """the blocks of lives 2 and 3: the first five (15 steps); in SampleRNN resident mode the first two, which are two resident launches; two
    steps of `hop` frames for Seq2Seq - the oracle's cost per life stays near that of the case itself"""
    if case.kind in ("s2s", "s2s_classes"):
        return case.parts[:2]
    return case.parts[:2] if case.parts in (RES_PARTS_16, RES_PARTS_32) else case.parts[:5]


def lives(case):
    """the four lives of a case on one plan:
      1  the case itself
      2  the case's clips, a prompt 5 longer (it starts below where life 1 ended: the tags and ring slots of life 1 lie ahead of it, on
         other ring phases; the WaveNet warm-up starts at position 8, the SampleRNN warm-up offset is (P + 5) % fs0; Seq2Seq has no prompt
         beyond `hop`: only the content changes), a prefix of the blocks, other inputs
      3  max(1, clips // 2 - 1) clips - ragged against the groups of 2, 4 and 16 the kernels work in -, the shortest prompt, other inputs
      4  life 1 again, bit for bit"""
    B, P, short = case.clips, case.P, life_parts(case)
    longer = P if case.kind in ("s2s", "s2s_classes") else P + 5
    return [Life(case, 1, B, P, case.parts, 0), Life(case, 2, B, longer, short, 1),
            Life(case, 3, max(1, B // 2 - 1), case.shortest_prompt, short, 2), Life(case, 4, B, P, case.parts, 0)]


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


def _s2s_case(tag, dim, hop, clips, layers, env, ran, forced_split=None, options=(), **kw):
    return Case(tag, "s2s", lambda: _s2s(dim, hop, layers, 7 + dim + hop, **kw), clips, (1, 1, 1), env, ran, hop=hop, forced_split=forced_split,
                options=options)


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

#   (the option cases and ALL_CASES: at the end of the module, behind the option defects they name)


# ---- the oracle, teacher-forced ----------------------------------------------------------------------------------------------------------------------
def to64(sd):
    return {k: (v.double() if torch.is_floating_point(v) else v) for k, v in sd.items()}


def reference(case, sd, hist, conds=(), arch=None):
    """the oracle's outputs of the case's n generated steps on the history `hist` (prompt + n steps; a tuple of streams for a network of several
    class inputs), in the dtype of `sd`: raw head outputs (clips, n, classes + 1) or frames (clips, n, bins) - for a network of several class
    inputs the tuple of its targets' raw outputs.  `arch`: other keywords for the oracle than the case's own (an option defect)"""
    n, P = case.n, case.P
    arch = case.arch if arch is None else arch
    sd = O.fold_weight_norm(sd)                    # (in the dtype of `sd`; the Seq2Seq decoder with residuals is weight-normed)
    if case.kind in ("wavenet", "wavenet_frames"):
        rf = O.wavenet_rf(arch["kernels"], arch["dilations"])
        lo, hi = P - rf, P + n - 1                 # ONE forward over the n windows: output j belongs to the window that starts at lo + j
        kw = dict(arch, embedding=False) if case.kind == "wavenet_frames" else arch
        inputs = tuple(x[:, lo:hi] for x in (*streams(hist), *conds))
        return O.wavenet_window_forward(sd, inputs, n_cond=len(inputs) - 1, every_position=True, **kw)
    if case.kind == "srnn":
        if case.multi:
            return O.SampleRNNOracle(sd, **arch).generate(tuple(x[:, :P] for x in hist), n, keep_logits=True, forced=tuple(hist))[1]
        return O.SampleRNNOracle(sd, **arch).generate(hist[:, :P], n, keep_logits=True, forced=hist)[1]
    outs = []
    for t in range(P, P + n, case.hop):
        x = hist[:, t - case.hop:t]
        for c in conds:                            # (further frame inputs: the network adds them up in front of the encoder)
            x = x + c[:, t - case.hop:t]
        outs.append(O.s2s_step(sd, x, case.hop, return_raw=True, **arch)[1] if case.kind == "s2s_classes" else O.s2s_step(sd, x, case.hop, **arch))
    return torch.cat(outs, 1)


def free_run(case, prompt, conds=()):
    """the fp32 oracle's own free-running history"""
    sd, arch = O.fold_weight_norm(case.sd), case.arch
    if case.kind == "wavenet" and case.multi:
        return (*O.wavenet_generate_streams(sd, prompt, case.n, **arch), *prompt[case.targets:])
    if case.kind == "wavenet":
        return O.wavenet_generate(sd, prompt, conds, case.n, **arch)
    if case.kind == "wavenet_frames":
        return O.wavenet_generate_frames(sd, prompt, case.n, **arch)
    if case.kind == "srnn":
        return O.SampleRNNOracle(sd, **arch).generate(prompt, case.n)
    if conds:
        hop, P = case.hop, case.P
        frames = torch.cat([prompt, torch.zeros(case.clips, case.n, 65)], 1)
        for t in range(P, P + case.n, hop):
            frames[:, t:t + hop] = O.s2s_step(sd, frames[:, t - hop:t] + sum(c[:, t - hop:t] for c in conds), hop, **arch)
        return frames
    out = O.s2s_generate(sd, prompt, case.n, case.hop, **arch)
    return out.long() if case.kind == "s2s_classes" else out


class Envelope(NamedTuple):
    R64: torch.Tensor
    E: torch.Tensor
    R32: torch.Tensor
    R32k: torch.Tensor


def envelope(history, case, conds=()):
    """the three teacher-forced runs on `history`: (R64, E, R32, R32k), every generated step - one Envelope, or for a network of several class
    inputs the list of its targets' Envelopes"""
    sd = case.sd
    R64 = reference(case, to64(sd), history, conds)
    R32 = reference(case, sd, history, conds)
    with O.activation_formulas(**KERNEL_FORMULAS):
        R32k = reference(case, sd, history, conds)
    envs = []
    for r64, r32, r32k in zip(streams(R64), streams(R32), streams(R32k)):
        assert r64.dtype == torch.float64 and r32.dtype == torch.float32 and r32k.dtype == torch.float32
        envs.append(Envelope(r64, torch.maximum((r32.double() - r64).abs(), (r32k.double() - r64).abs()), r32, r32k))
    assert len(envs) == case.targets
    return envs if case.multi else envs[0]


def per_target(x):
    """the per-target list of a case's envelopes, outputs or defect outputs (one target: a list of one)"""
    return list(x) if isinstance(x, (tuple, list)) and not isinstance(x, Envelope) else [x]


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
    """the float64 run with one defect must leave tol_max somewhere among the compared elements (NaN counts as leaving it).  Several targets:
    lists with one entry per target, each target with its own tol_max; the defect has to leave one of them"""
    defect, R64 = per_target(defect), per_target(R64)
    tol_max = list(tol_max) if isinstance(tol_max, (tuple, list)) else [tol_max]
    assert len(defect) == len(R64) == len(tol_max)
    moved = [float((d - r).abs().max()) for d, r in zip(defect, R64)]
    assert any(bool((~((d - r).abs() <= t)).any()) for d, r, t in zip(defect, R64, tol_max)), \
        f"{what}: the defect moves the outputs by at most {moved}, inside tol_max {tol_max} - the envelope is too loose"


def _keys(case, sd):
    arch = case.arch
    if case.kind in ("wavenet", "wavenet_frames"):
        L = len(arch["kernels"])
        bias = "layers.0.conv_skip.bias" if "layers.0.conv_skip.bias" in sd else \
            next(k for k in sd if k.startswith("layers.0.conv_dil") and k.endswith("bias"))
        return bias, next(k for k in sd if k.startswith(f"layers.{L // 2}.conv_dil") and k.endswith("weight"))
    if case.kind == "srnn":
        # (b): the last stacked layer of the tier right above the bottom, for every case (the module docstring says why)
        return "tiers.0.rnn.bias_hh_l0", f"tiers.{len(arch['frame_sizes']) - 2}.rnn.weight_hh_l{arch.get('n_rnn', 1) - 1}"
    return "dec.lstm.0.bias_hh_l0_reverse", "dec.lstm.0.weight_hh_l0"


def _drop(sd, key, entry=None):
    """(entry, the vector sd[key] with that entry zeroed) - by default the entry of median magnitude"""
    b = sd[key].clone()
    entry = int(b.abs().argsort()[b.numel() // 2]) if entry is None else entry
    b.view(-1)[entry] = 0.0
    return entry, b


def _stale(x, clip=0):
    """x with one clip's rows one step late"""
    y = x.clone()
    y[clip, 1:] = x[clip, :-1]
    return y


def bias_dropped(case, history, conds, entry=None):
    """defect (a): (name, the float64 outputs) with entry `entry` of the case's bias vector zeroed - by default the one of median magnitude"""
    sd64 = O.fold_weight_norm(to64(case.sd))
    bias_key, _ = _keys(case, sd64)
    entry, b = _drop(sd64, bias_key, entry)
    return f"(a) entry {entry} of {bias_key} dropped", reference(case, {**sd64, bias_key: b}, history, conds)


def defects(case, history, conds, R64):
    """(name, the float64 outputs with that one defect) for the four defects of the module docstring, then the case's option defects.
    `R64`: the float64 outputs, or the list of them per target - the defects' outputs come in the same form"""
    sd64 = O.fold_weight_norm(to64(case.sd))
    _, weight_key = _keys(case, sd64)
    yield bias_dropped(case, history, conds)
    yield f"(b) {weight_key} scaled by 1 + 1e-4", reference(case, {**sd64, weight_key: sd64[weight_key] * (1 + 1e-4)}, history, conds)
    swapped = []
    for r in per_target(R64):
        c = r.clone()
        c[-1] = r[-2]
        swapped.append(c)
    yield "(c) the last clip's rows are the second-to-last clip's", swapped if case.multi else swapped[0]
    stale = (_stale(history[0]), *history[1:]) if case.multi else _stale(history)
    yield "(d) clip 0's window one step stale", reference(case, sd64, stale, conds)
    for option in case.options:
        yield from option(case, sd64, history, conds)


def life_defects(life, history, conds, R64, prev_history, prev_R64, prev=None):
    """(name, the float64 outputs with that one defect, the indices into rows() it is checked on) for the defects of a plan's later lives.
    `prev_history` / `prev_R64`: the history and the float64 outputs (per target) of the life before, `prev` that life (for (g)):
      (e) clip 0's prompt is the previous life's, position by position (the rings are addressed by absolute position): a queue, a ring or
          a state the warm-up did not rewrite - on the rows the prompt still reaches (Life.reached)
      (f) the last clip's rows are the previous life's rows of the same clip index and the same steps: a ragged group that was skipped
      (g) SampleRNN, life 2: the tiers start from the previous life's final hidden states instead of h0 (the oracle keeps its tier states
          in `hidden` and puts them back through reset_hidden(): with that method stubbed on the one instance it runs on from where the
          generation before ended - nothing of the oracle is rewritten)"""
    sd64 = O.fold_weight_norm(to64(life.sd))
    P, n = life.P, life.n
    first, prev_first = streams(history)[0], streams(prev_history)[0]
    stale = first.clone()
    stale[0, :P] = prev_first[0, :P]
    assert not torch.equal(stale, first)
    stale = (stale, *history[1:]) if life.multi else stale
    yield "(e) clip 0's prompt is the previous life's", reference(life, sd64, stale, conds), life.reached()
    every = list(range(len(life.rows())))
    skipped = []
    for r, pr in zip(per_target(R64), per_target(prev_R64)):
        c = r.clone()
        c[-1] = pr[life.clips - 1, :n]
        skipped.append(c)
    yield "(f) the last clip's rows are the previous life's", skipped if life.multi else skipped[0], every
    if life.kind == "srnn" and prev is not None and prev.clips == life.clips:
        oracle = O.SampleRNNOracle(sd64, **life.arch)
        oracle.reset_hidden = lambda: None
        if life.multi:
            oracle.generate(tuple(x[:, :prev.P] for x in prev_history), prev.n, forced=tuple(prev_history))
            out = oracle.generate(tuple(x[:, :P] for x in history), n, keep_logits=True, forced=tuple(history))[1]
        else:
            oracle.generate(prev_history[:, :prev.P], prev.n, forced=prev_history)
            out = oracle.generate(history[:, :P], n, keep_logits=True, forced=history)[1]
        yield "(g) the tiers start from the previous life's final hidden states", out, every


# ---- option defects: generators of (name, the float64 outputs with the option subtly off) over (case, folded float64 state dict, history, conds) --
def _layer_key(case, sd, leaf):
    """the key of the middle layer's dilated convolution (gated or not) that ends in `leaf`"""
    L = len(case.arch["kernels"])
    return next(k for k in sd if k.startswith(f"layers.{L // 2}.conv_dil") and k.endswith(leaf))


def _head_biases(case, sd, k=0):
    """the bias keys of target k's MLP head, in the order of its Linears (dropout modules between them shift the indices)"""
    p = f"output_module.heads.{k}.estimator.0.fc." if case.kind.startswith("s2s") else f"output_modules.{k}.estimator.0.fc."
    ns = sorted(int(key[len(p):].split(".")[0]) for key in sd if key.startswith(p) and key.endswith(".bias"))
    return [f"{p}{n}.bias" for n in ns]


def opt_oldest_tap(case, sd, hist, conds):
    """kernel size 3 or 4: the oldest tap's slice of the middle layer's weight zeroed - a launch path that walks a kernel's taps in the wrong
    order, or stops one short, as a kernel written for two taps would"""
    key = _layer_key(case, sd, "weight")
    w = sd[key].clone()
    assert w.shape[2] > 2
    w[:, :, 0] = 0.0
    yield f"[kernel size] the oldest tap of {key} zeroed", reference(case, {**sd, key: w}, hist, conds)


def opt_conditioning(case, sd, hist, conds):
    """conditioning: clip 0's conditioning input one step stale (a conditioning row read at t - 1: the row of the step before, or of the ragged
    clip's neighbour in time); with two inputs, also the two raw inputs swapped (their projections laid side by side in the wrong order)"""
    yield "[conditioning] clip 0's conditioning input one step stale", reference(case, sd, hist, (_stale(conds[0]), *conds[1:]))
    if len(conds) == 2:
        yield "[conditioning] the two raw inputs swapped", reference(case, sd, hist, conds[::-1])


def opt_affine_bias(case, sd, hist, conds):
    """affine residuals: the median entry of a middle layer's aff_res.params.bias dropped - one of the three chunks (x_hat, a, b) of the
    1x1 convolution packed without its bias"""
    key = f"layers.{len(case.arch['kernels']) // 2}.aff_res.params.bias"
    entry, b = _drop(sd, key)
    yield f"[affine residuals] entry {entry} of {key} dropped", reference(case, {**sd, key: b}, hist, conds)


def opt_hidden_bias(case, sd, hist, conds):
    """a deeper head: the median bias entry of the hidden Linear dropped (the hidden blocks share ONE Linear, so in every copy of it) - a
    head kernel that applies the hidden layer's bias only where the one-layer head has one"""
    keys = _head_biases(case, sd)[1:-1]
    assert keys and all(torch.equal(sd[k], sd[keys[0]]) for k in keys)
    entry, b = _drop(sd, keys[0])
    yield f"[deeper head] entry {entry} of {keys[0]} dropped", reference(case, {**sd, **{k: b for k in keys}}, hist, conds)


def opt_narrow_head(case, sd, hist, conds):
    """a head narrower than the pipelines' 128 x 256: the bias of the last real class q - 1 dropped, then that of the temperature column q -
    the two columns that border the padding: a padded column (bias -inf) that leaks into its neighbour, or a temperature read from column 256"""
    key, q = _head_biases(case, sd)[-1], case.q[0]
    assert sd[key].numel() == q + 1 and q < 256
    for entry, what in ((q - 1, "the last class"), (q, "the temperature column")):
        yield f"[narrow head] the bias of {what} ({entry} of {key}) dropped", reference(case, {**sd, key: _drop(sd, key, entry)[1]}, hist, conds)


def opt_targets(case, sd, hist, conds):
    """several inputs and targets: for every target k > 0, the last bias entry of head k dropped (a second head that reads the first one's
    bias vector, whose length differs); and the last stream one step stale for clip 0 (a class stream of the step before, or read at the first
    stream's position)"""
    for k in range(1, case.targets):
        key = _head_biases(case, sd, k)[-1]
        entry = sd[key].numel() - 1
        yield f"[several targets] the last bias entry of head {k} ({key}) dropped", reference(case, {**sd, key: _drop(sd, key, entry)[1]}, hist, conds)
    k = len(hist) - 1
    yield f"[several inputs] stream {k} of clip 0 one step stale", reference(case, sd, (*hist[:k], _stale(hist[k])), conds)


def opt_stacked_bias(case, sd, hist, conds):
    """stacked recurrent layers: the median bias_hh entry of the LAST stacked layer of tier 0 dropped - a loop over the stack that binds layer
    0's operands for every layer, or stops one layer short"""
    key = f"tiers.0.rnn.bias_hh_l{case.arch['n_rnn'] - 1}"
    entry, b = _drop(sd, key)
    yield f"[stacked layers] entry {entry} of {key} dropped", reference(case, {**sd, key: b}, hist, conds)


def _keyword(option, what, **kw):
    def run(case, sd, hist, conds):
        yield f"[{option}] {what}", reference(case, sd, hist, conds, arch=dict(case.arch, **kw))
    return run


# h0_init ones run from zeros: a warm-up that clears the state it was told to fill with ones
opt_h0_zeros = _keyword("h0_init", "the hidden state starts from zeros", h0="zeros")
# inputs_mode mean run as sum: the 1 / M of the mean left out where the inputs' projections are added up
opt_mean_as_sum = _keyword("inputs_mode", "mean run as sum", inputs_mode="sum")
# inputs_mode static_mix run as mean: the learned mixing weights never bound, every input weighted alike
opt_mix_as_mean = _keyword("inputs_mode", "static_mix run as mean", inputs_mode="mean")
# layerwise_inputs left out: the embedded input not added to every layer's output
opt_not_layerwise = _keyword("layerwise_inputs", "the embedded input is not added to the layers' outputs", layerwise_inputs=False)


def opt_layer_order(case, sd, hist, conds):
    """reverse_layer_order: the layers' dilations in build order instead of run order (which layer has its residual 1x1 is fixed by the
    weights) - a plan that reverses the weights but not the ring geometry"""
    yield "[reverse_layer_order] the dilations in build order", reference(case, sd, hist, conds, arch=dict(case.arch, dilations=case.arch["dilations"][::-1]))


def opt_no_gate(case, sd, hist, conds):
    """act_g=None: the one activation of a layer evaluated by the gate's function instead of the filter's - a launch path that picks the
    gate's slot of the activation pair.  (Running the gate itself cannot be expressed: the ungated convolution has half the channels.)"""
    arch = dict(case.arch, act_f=case.arch.get("act_g", "Sigmoid"))
    yield f"[no gate] the layers' activation is {arch['act_f']}", reference(case, sd, hist, conds, arch=arch)


def opt_gate_swapped(case, sd, hist, conds):
    """act_f / act_g: the two activations swapped between the filter half and the gate half of a layer's channels"""
    arch = dict(case.arch, act_f=case.arch["act_g"], act_g=case.arch["act_f"])
    yield "[activations] act_f and act_g swapped", reference(case, sd, hist, conds, arch=arch)


def opt_pooling(case, sd, hist, conds):
    """Seq2Seq pooling: edge_mean run as mean, edge_sum as sum, sum as edge_sum - they differ only in which frames of the window count: a
    pooling kernel that takes every frame where it should take the two at the edges, or the reverse"""
    other = {"edge_mean": "mean", "edge_sum": "sum", "sum": "edge_sum"}[case.arch["downsampling"]]
    yield f"[pooling] {case.arch['downsampling']} run as {other}", reference(case, sd, hist, conds, arch=dict(case.arch, downsampling=other))


def opt_interp(case, sd, hist, conds):
    """Seq2Seq upsampling interp run as repeat: the encoder's two final states not spread over the decoder's frames (interp has no
    up-sampling weights, so linear_resample cannot be run on its state dict)"""
    assert "dec.fc.fc.weight" not in sd
    yield "[upsampling] interp run as repeat", reference(case, sd, hist, conds, arch=dict(case.arch, upsampling="repeat"))


def opt_deepest_bias(case, sd, hist, conds):
    """asymmetric stacks: the median bias_hh entry of the deepest layer of the longer side dropped - a plan that sizes both stacks by one
    side's depth never binds that layer's operands"""
    depth = {side: 1 + max(int(k.split(".")[2]) for k in sd if k.startswith(side + ".lstm.")) for side in ("enc", "dec")}
    assert depth["enc"] != depth["dec"]
    side = max(depth, key=depth.get)
    key = f"{side}.lstm.{depth[side] - 1}.bias_hh_l0"
    entry, b = _drop(sd, key)
    yield f"[stacks] entry {entry} of {key} dropped", reference(case, {**sd, key: b}, hist, conds)


def opt_second_input(case, sd, hist, conds):
    """several continuous inputs: clip 0's second input one step stale (swapping the inputs of a sum changes nothing) - the second input read
    at another frame than the first"""
    yield "[several inputs] clip 0's second input one step stale", reference(case, sd, hist, (_stale(conds[0]),))


# ---- the option cases -----------------------------------------------------------------------------------------------------------------------------------
def _wn_option_defects(kw):
    """the option defects of a helpers.WAVENET_OPTIONS / WAVENET_ACTS entry"""
    out = []
    if kw.get("kernel_sizes", (2,))[0] > 2:
        out.append(opt_oldest_tap)
    if kw.get("cond"):
        out.append(opt_conditioning)
    if kw.get("with_affine_residuals"):
        out.append(opt_affine_bias)
    if kw.get("io", {}).get("n_mlp_layers"):
        out.append(opt_hidden_bias)
    if "act_g" in kw and kw["act_g"] is None:
        out.append(opt_no_gate)
    elif "act_f" in kw:
        out.append(opt_gate_swapped)
    if kw.get("layerwise_inputs"):
        out.append(opt_not_layerwise)
    if kw.get("reverse_layer_order"):
        out.append(opt_layer_order)
    return tuple(out)


def _wn_stage(batched):
    return lambda p, k, w=1: p.stage_pipelined and p.batch_pipelined == batched


_BP = {"MMK_WN_SPIPE": "1", "MMK_WN_BPIPE": "1"}
# 16 channels, 5 layers (freqnet: 32 channels, 3 layers), 9 clips: past a row group of 8, short of 16, odd; all on the per-layer launch path
# (`tied` - tie_io_weights - and the dropout head change where the weights come from, not what is computed: the four standing defects only)
WAVENET_OPTION_CASES = [
    *[Case(f"opt-{tag}", "wavenet", lambda tag=tag: _no_n_cond(H.wavenet_option(tag)), 9, WN_PARTS, {}, _wn_launches, cond=int(bool(kw.get("cond"))),
           options=_wn_option_defects(kw)) for tag, kw in H.WAVENET_OPTIONS.items()],
    *[Case(f"act-{tag}", "wavenet", lambda tag=tag: _no_n_cond(H.wavenet_act(tag)), 9, WN_PARTS, {}, _wn_launches, cond=int(bool(kw.get("cond"))),
           options=_wn_option_defects(kw)) for tag, kw in H.WAVENET_ACTS.items()],
    Case("head-wn_relu_dp", "wavenet", lambda: _mlp_head("wn_relu_dp"), 9, WN_PARTS, {}, _wn_launches),
    Case("head-wn_tanh_2", "wavenet", lambda: _mlp_head("wn_tanh_2"), 9, WN_PARTS, {}, _wn_launches, options=(opt_hidden_bias,)),
    Case("frames-g1", "wavenet_frames", lambda: H.freqnet("g1"), 9, WN_PARTS, {}, _wn_launches),
    Case("frames-g2abs", "wavenet_frames", lambda: H.freqnet("g2abs"), 9, WN_PARTS, {}, _wn_launches),
]

# the pipelines' padded heads: (q, mlp_dim, cond_dims, blocks, clips) of test_wavenet_stage_pipeline_takes_narrower_heads_and_two_conditioning_inputs
# and (q, mlp_dim, blocks, clips) of test_wavenet_layer_pipeline_takes_narrower_heads (tests/test_gpu_networks.py), with their seeds
WAVENET_HEAD_CASES = [
    Case("spipe-narrow-200-100-33", "wavenet", lambda: _wavenet(256, (2, 2, 1), 100, 500 + 200 + 33, (32, 16), q=200), 33, WN_PARTS, _SP, _wn_stage(False),
         cond=2, q=(200,), options=(opt_narrow_head, opt_conditioning)),
    Case("bpipe-narrow-200-100-33", "wavenet", lambda: _wavenet(256, (2, 2, 1), 100, 500 + 200 + 33, (32, 16), q=200), 33, WN_PARTS, _BP, _wn_stage(True),
         cond=2, q=(200,), options=(opt_narrow_head, opt_conditioning)),
    Case("spipe-narrow-64-40-9", "wavenet", lambda: _wavenet(256, (4,), 40, 500 + 64 + 9, (16,), q=64), 9, WN_PARTS, _SP, _wn_stage(False),
         cond=1, q=(64,), options=(opt_narrow_head, opt_conditioning)),
    Case("lpipe-narrow-200-112-40", "wavenet", lambda: _wavenet(64, (4,), 112, 700 + 200, q=200), 40, WN_PARTS, {}, _wn_lpipe, q=(200,),
         options=(opt_narrow_head,)),
    Case("lpipe-narrow-64-32-13", "wavenet", lambda: _wavenet(64, (4, 3), 32, 700 + 64, q=64), 13, WN_PARTS, {}, _wn_lpipe, q=(64,),
         options=(opt_narrow_head,)),
]


def _multi_case(tag):
    kind, classes, heads, kw = H.MULTI_IO[tag]
    options = (opt_targets,) + {"mean": (opt_mean_as_sum,), "static_mix": (opt_mix_as_mean,)}.get(kw.get("inputs_mode"), ())
    if kind == "wavenet":      # (class conditioning streams and further targets: the launch path, csrc/wavenet_plan.hip)
        return Case(f"multi-{tag}", "wavenet", lambda: _multi_io(tag), 9, WN_PARTS, {}, _wn_launches, q=classes, targets=len(heads), options=options)
    # (several class streams: the kernels in turns, one launch per op, csrc/srnn_plan.hip)
    return Case(f"multi-{tag}", "srnn", lambda: _multi_io(tag), 9, SRNN_PARTS, {}, _bottom(LAUNCHES), q=classes, targets=len(heads), options=options)


MULTI_CASES = [_multi_case(tag) for tag in H.MULTI_IO]
WAVENET_MULTI_CASES = [c for c in MULTI_CASES if c.kind == "wavenet"]
SRNN_MULTI_CASES = [c for c in MULTI_CASES if c.kind == "srnn"]


def _srnn_option_defects(kw):
    out = []
    if kw.get("n_rnn", 1) > 1:
        out.append(opt_stacked_bias)
    if kw.get("io", {}).get("n_mlp_layers"):
        out.append(opt_hidden_bias)
    if kw.get("h0_init") == "ones":
        out.append(opt_h0_zeros)
    return tuple(out)


# hidden 32, 11 clips: the tier and bottom kernels take 128 hidden units and up, so every one of these runs one launch per op and never
# resident (bottom_kernel 3, resident_blocks 0).  inputs_mode mean / static_mix of ONE input weight it by 1 (ZipReduceVariables): `gru_mean`
# has no option defect, and `lstm_mix_ones` only the one of h0_init; weight norm and the heads' activations are held by the standing defects
SRNN_OPTION_CASES = [
    *[Case(f"opt-{tag}", "srnn", lambda tag=tag: H.srnn_option(tag), 11, SRNN_PARTS, {}, _bottom(LAUNCHES), options=_srnn_option_defects(kw))
      for tag, kw in H.SRNN_OPTIONS.items()],
    Case("weight_norm-gru", "srnn", lambda: H.srnn("gru", weight_norm=True), 11, SRNN_PARTS, {}, _bottom(LAUNCHES)),
    Case("weight_norm-lstm", "srnn", lambda: H.srnn("lstm", weight_norm=True), 11, SRNN_PARTS, {}, _bottom(LAUNCHES)),
    Case("head-srnn_softplus_dp1d", "srnn", lambda: _mlp_head("srnn_softplus_dp1d"), 11, SRNN_PARTS, {}, _bottom(LAUNCHES)),
    Case("head-srnn_sigmoid", "srnn", lambda: _mlp_head("srnn_sigmoid"), 11, SRNN_PARTS, {}, _bottom(LAUNCHES)),
]


def _s2s_variant(ds, us):
    options = ((opt_pooling,) if ds in ("edge_mean", "edge_sum", "sum") else ()) + ((opt_interp,) if us == "interp" else ())
    return _s2s_case(f"{ds}-{us}", 128, 8, 16, 1, {}, _s2s_resident(1), ds=ds, us=us, options=options)


def _s2s_stack_case(tag, enc, dec):
    return Case(f"stack-{tag}", "s2s", lambda: _s2s_stack(tag, 128, 8, 143), 16, (1, 1, 1), {}, _s2s_resident(enc, dec), hop=8, options=(opt_deepest_bias,))


# model_dim 128, hop 8, 16 clips: the smallest resident width, 128 rows (the tiled GEMM); every bi-LSTM layer of every step is one resident launch
S2S_OPTION_CASES = [
    *[_s2s_variant(ds, us) for ds, us in H.S2S_VARIANTS if (ds, us) != ("mean", "repeat")],      # (mean-repeat: S2S_CASES)
    _s2s_stack_case("e2d1", 2, 1), _s2s_stack_case("e1d3", 1, 3), _s2s_stack_case("e3d1res_sum", 3, 1),
    Case("classes-mlp2_stack", "s2s_classes", lambda: _s2s_classes("mlp2_stack", 2), 16, (1, 1, 1), {}, _s2s_resident(2), hop=2, options=(opt_hidden_bias,)),
    # (two frame inputs: the network adds them up and has no block path - the device test goes step by step)
    Case("two_inputs", "s2s", lambda: _s2s_stack(None, 128, 8, 141, inputs=2), 16, (1, 1, 1), {}, _s2s_resident(1), hop=8, cond=1, options=(opt_second_input,)),
]

WAVENET_ALL = WAVENET_CASES + WAVENET_OPTION_CASES + WAVENET_HEAD_CASES + WAVENET_MULTI_CASES
SRNN_ALL = SRNN_CASES + SRNN_OPTION_CASES + SRNN_MULTI_CASES
S2S_ALL = S2S_CASES + S2S_OPTION_CASES
ALL_CASES = [("wavenet", c) for c in WAVENET_ALL] + [("srnn", c) for c in SRNN_ALL] + [("s2s", c) for c in S2S_ALL]


