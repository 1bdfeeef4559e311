"""WaveNet, SampleRNN and Seq2Seq step outputs on the device against the float64 oracle, inside the envelope of tests/net_refs.py: every
execution mode the plans know (the cases and the plan flags that prove the intended kernel ran are in net_refs.py: WAVENET_CASES,
SRNN_CASES, S2S_CASES), greedy, in consecutive generate_block calls.  Three switches leave no trace in a plan's flags: `chain-step_warmup`
(MMK_WN_PREFILL=0 is read at warm-up; the case asserts the chain kernel only), Seq2Seq `per_frame` against `launches` (both report no resident
launch; nothing tells the fused per-frame cell from one launch per op) and the split-K cases, which are proven otherwise: the expected split
is derived from the GEMM's geometry (net_refs.gemm_k_split, test_net_refs.py) and the frames must differ bitwise from the unforced run's.

Class networks: last_logits after every block against R64 of the device's own history (check_outputs: 4 max(E) and 4 rms(E)), the class of
EVERY step against R64's argmax within 2 tol_max (check_picks), and the four defects of net_refs.py on the same rows (check_near_miss).
Frame networks (Seq2Seq on magnitude frames, WaveNet on magnitude frames): every generated frame, the reference of each step run on the
device's own preceding frames.

First run on an MI355X, per case: max|dev - R64| / max(E) and rms(dev - R64) / rms(E) over the compared elements (the margin allows 4).  Records, not
tolerances - the tolerance is recomputed from the reference on every run:

  network     case                                 outputs  scale   max ratio  rms ratio    max(E)     rms(E)
  wavenet     launches                               11565  1.89         0.77       0.72  7.434e-07  1.515e-07
  wavenet     persist                                11565  1.89         0.81       0.75  7.434e-07  1.515e-07
  wavenet     chain                                  11565  1.89         0.62       0.69  7.434e-07  1.515e-07
  wavenet     chain-cond                             11565  4.29         0.74       0.71  1.140e-06  2.665e-07
  wavenet     chain-step_warmup                      11565  1.89         0.79       0.71  7.434e-07  1.515e-07
  wavenet     lpipe-4_3-13                           30069  1.85         0.50       0.61  1.295e-06  2.438e-07
  wavenet     lpipe-10-8                             18504  3.42         0.74       0.65  1.775e-06  4.124e-07
  wavenet     lpipe-cond                             30069  5.53         0.47       0.51  3.002e-06  5.853e-07
  wavenet     spipe-5                                11565  0.626        0.49       0.52  4.369e-07  1.021e-07
  wavenet     spipe-cond                             11565  2.68         0.43       0.36  1.438e-06  3.645e-07
  wavenet     spipe-pair-24                          55512  0.661        0.47       0.53  4.603e-07  1.044e-07
  wavenet     bpipe-20                               46260  0.708        0.79       0.66  3.872e-07  1.044e-07
  wavenet     frames-g4                               7425  0.165        0.36       0.20  8.516e-08  2.075e-08
  sample_rnn  launches                               59367  4.04         0.45       0.47  2.245e-06  3.536e-07
  sample_rnn  bottom-one_clip                        59367  4.04         0.26       0.34  2.245e-06  3.536e-07
  sample_rnn  bottom-four_clips-321                  74382  3.89         0.46       0.43  1.644e-06  3.018e-07
  sample_rnn  tier-up_apart                          59367  2.93         0.33       0.34  1.260e-06  2.266e-07
  sample_rnn  rnn_tanh                               14135  4.93         0.41       0.46  2.647e-06  5.268e-07
  sample_rnn  n_rnn_2                                14135  3.31         0.27       0.39  1.844e-06  2.528e-07
  sample_rnn  resident-gru                           21588  3.57         0.32       0.32  1.703e-06  3.141e-07
  sample_rnn  resident-lstm                          21588  2.95         0.36       0.31  1.432e-06  2.136e-07
  sample_rnn  resident-32_8_2-33                     33924  3.21         0.32       0.32  1.804e-06  3.187e-07
  sample_rnn  resident-gru-512-40                    41120  3.65         0.27       0.33  2.144e-06  3.710e-07
  sample_rnn  resident-warmup_1                      21588  3.2          0.29       0.29  1.645e-06  3.162e-07
  sample_rnn  resident-warmup_0                      21588  3.2          0.29       0.29  1.645e-06  3.162e-07
  seq2seq     resident-128-2-3                        1170  0.313        1.01       1.00  1.230e-07  3.909e-08
  seq2seq     resident-256-5-17                      16575  0.484        0.75       0.83  2.235e-07  4.731e-08
  seq2seq     resident-512-3-33                      19305  0.428        0.86       0.83  2.070e-07  4.784e-08
  seq2seq     resident-128-7-128                    174720  0.647        0.76       0.87  2.722e-07  4.709e-08
  seq2seq     resident-128-8-16-2layers              24960  0.273        0.98       1.02  1.623e-07  3.809e-08
  seq2seq     resident-128-8-16-2layers-residuals    24960  1.01         0.57       0.74  6.951e-07  1.200e-07
  seq2seq     per_frame                              24960  0.273        0.88       0.94  1.623e-07  3.843e-08
  seq2seq     launches                               24960  0.273        0.46       0.24  1.623e-07  3.829e-08
  seq2seq     ksplit-2                               24960  0.45         1.19       0.89  2.011e-07  4.608e-08
  seq2seq     ksplit-3                               24960  0.45         1.12       0.88  2.011e-07  4.605e-08
  seq2seq     mean-repeat                            24960  0.4          0.93       0.91  2.302e-07  4.328e-08
  seq2seq     classes                                74016  0.219        0.78       0.92  1.029e-07  2.126e-08

The device lies inside the reference's own fp32 error, or at it, everywhere (ratios 0.2 .. 1.2): no case needed a finding.
Split K: 6331 (forced 2) and 5178 (forced 3) of the 8320 frames of the first step differ bitwise from the run with the launch's
own four-way split, by at most 1.341e-07 and 1.043e-07.
"""
import pytest
import torch

import mimikit_amd as mmk
from tests import net_refs as R

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

SWITCHES = ("MMK_WN_XCD_LOCAL", "MMK_WN_PERSISTENT", "MMK_WN_GROUPS", "MMK_WN_SMALL", "MMK_WN_PREFILL", "MMK_WN_CHAIN", "MMK_WN_LPIPE", "MMK_WN_SPIPE",
            "MMK_WN_BPIPE", "MMK_WN_PIPE", "MMK_WN_SPIPE_PAIR", "MMK_SRNN_FUSED", "MMK_SRNN_FUSED_UP", "MMK_SRNN_RESIDENT", "MMK_SRNN_RESIDENT_WARMUP",
            "MMK_SRNN_COMPOSED", "MMK_S2S_FUSED", "MMK_S2S_SEQ", "MMK_S2S_COMPOSED", "MMK_GEMM_KSPLIT")


def _switch(monkeypatch, case):
    for k in SWITCHES:
        monkeypatch.delitem(mmk.native.PLAN_TUNING, k, raising=False)
    for k, v in case.env.items():
        monkeypatch.setitem(mmk.native.PLAN_TUNING, k, v)


def _generate(case, device, what):
    """the case's blocks on the device -> (history on the host, the outputs the device hands back: (clips, compared steps, columns))"""
    net = case.make()[0].to(device)
    prompt, conds = case.inputs()
    B, P, n, hop = case.clips, case.P, case.n, case.hop or 1
    conds_d = tuple(c.to(device) for c in conds)
    data = torch.cat([prompt, torch.zeros(B, n, *prompt.shape[2:], dtype=prompt.dtype)], 1).to(device)
    if case.kind in ("srnn", "s2s", "s2s_classes"):
        net.before_generate((data[:, :P],), None)
        if case.kind == "srnn" and "MMK_SRNN_RESIDENT_WARMUP" in case.env:
            assert case.ran(net._plan, 0), (what, "the warm-up took another path", net._plan.resident_warmups())
    rows, t = [], P
    for k, nb in enumerate(case.parts, 1):
        assert net.generate_block((data, *conds_d), t, nb * hop)
        t += nb * hop
        plan = net._plan
        assert case.ran(plan, k), (what, f"block {k}: the plan took another kernel")
        waits = plan.persistent if case.kind in ("wavenet", "wavenet_frames") else plan.resident_blocks() if case.kind == "srnn" else plan.resident_launches()
        if waits:
            plan.sync_status()                     # (the workgroups of these kernels wait for each other: a timed-out wait is an error here)
        if case.classes:
            rows.append(plan.last_logits(B).cpu())
    net.after_generate((data,), None)
    hist = data.cpu()
    if not case.classes:
        return hist, hist[:, P:]
    return hist, torch.cat(rows, 1) if case.kind == "s2s_classes" else torch.stack(rows, 1)


def _against_float64(case, device, monkeypatch, what):
    _switch(monkeypatch, case)
    hist, dev = _generate(case, device, what)
    _, conds = case.inputs()
    env = R.envelope(hist, case, conds)
    rows = case.rows()
    R64, E = env.R64[:, rows], env.E[:, rows]
    assert dev.shape == R64.shape, (what, dev.shape, R64.shape)
    tol_max, tol_rms = R.tolerance(E)
    r_max, r_rms = R.ratios(dev, R64, E)
    print(f"[f64] {what}: {dev.numel()} outputs of scale {float(R64.abs().max()):.3g}; max|dev - R64| / max(E) = {r_max:.2f}, rms(dev - R64) / rms(E) = {r_rms:.2f} "
          f"(the margin allows {R.FACTOR:g}); max(E) {float(E.max()):.3e}, rms(E) {R.rms(E):.3e}")
    R.check_outputs(dev, R64, tol_max, tol_rms, what)
    if case.classes:
        R.check_picks(hist[:, case.P:], env.R64, tol_max, what)
    for name, out in R.defects(case, hist, conds, env.R64):
        R.check_near_miss(out[:, rows], R64, tol_max, f"{what} {name}")
    if case.forced_split:
        # the plan reports nothing about the split: the same case without the switch (the launch then splits K its own way, which
        # test_net_refs.py shows to be another one) must give other bits in the first step's frames, which both runs compute from the prompt
        monkeypatch.delitem(mmk.native.PLAN_TUNING, "MMK_GEMM_KSPLIT")
        _, unforced = _generate(case, device, what + " without the switch")
        first = slice(0, case.hop)
        differ = int((unforced[:, first] != dev[:, first]).sum())
        print(f"[f64] {what}: {differ} of {dev[:, first].numel()} frames of the first step differ bitwise from the unforced split's, by at most "
              f"{float((unforced[:, first] - dev[:, first]).abs().max()):.3e}")
        assert differ > 0, (what, "the forced split gave the bits of the launch's own split: the switch did not take effect")
        R.check_outputs(unforced[:, first], R64[:, first], tol_max, float("inf"), what + " without the switch")


@pytest.mark.parametrize("case", R.WAVENET_CASES, ids=[c.id for c in R.WAVENET_CASES])
def test_wavenet_steps_within_the_float64_envelope(device, monkeypatch, case):
    """launch path, wavenet_persist, wavenet_chain, wavenet_lpipe (a ragged group of eight; rf 1024: the long rings), wavenet_spipe (one clip and
    two clips per visit), wavenet_bpipe (16 + a ragged 4), conditioned variants, the per-step warm-up, a magnitude-frame net; prompt rf + 3,
    blocks of 1 .. 9 steps: nine rows per clip, ends on every small ring phase"""
    _against_float64(case, device, monkeypatch, f"wavenet {case.id}")


@pytest.mark.parametrize("case", R.SRNN_CASES, ids=[c.id for c in R.SRNN_CASES])
def test_sample_rnn_steps_within_the_float64_envelope(device, monkeypatch, case):
    """hidden 128 (one case 512): one launch per op, the one-clip and four-clip bottom kernels, the tier kernel with its up-sampler apart, tanh
    tiers and stacked layers, resident mode (GRU and LSTM, frames of 1 and 2 samples, ragged row tiles, both warm-ups); prompt 2 rf + 3; resident
    blocks at least two periods long that end on four residues of the period, each of them one resident launch"""
    _against_float64(case, device, monkeypatch, f"sample_rnn {case.id}")


@pytest.mark.parametrize("case", R.S2S_CASES, ids=[c.id for c in R.S2S_CASES])
def test_seq2seq_steps_within_the_float64_envelope(device, monkeypatch, case):
    """magspec n_fft 128: the resident bi-LSTM over its geometry (stacked layers with and without residuals), one launch per frame, one launch per
    op, the output projection split over K two and three ways (model_dim 256: four stages, batch x hop = 128) where the launch itself would split it
    four ways, another pooling / upsampling pair, and the class path; three chained steps each"""
    _against_float64(case, device, monkeypatch, f"seq2seq {case.id}")
