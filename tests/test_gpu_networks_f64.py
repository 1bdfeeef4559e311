"""WaveNet, SampleRNN and Seq2Seq step outputs on the device against the float64 oracle, inside the envelope of tests/net_refs.py: every
execution mode the plans know (the cases and the plan flags that prove the intended kernel ran are in net_refs.py: WAVENET_CASES,
SRNN_CASES, S2S_CASES), greedy, in consecutive generate_block calls.  Three switches leave no trace in a plan's flags: `chain-step_warmup`
(MMK_WN_PREFILL=0 is read at warm-up; the case asserts the chain kernel only), Seq2Seq `per_frame` against `launches` (both report no resident
launch; nothing tells the fused per-frame cell from one launch per op) and the split-K cases, which are proven otherwise: the expected split
is derived from the GEMM's geometry (net_refs.gemm_k_split, test_net_refs.py) and the frames must differ bitwise from the unforced run's.
And every network option the plans branch on (net_refs.py: WAVENET_OPTION_CASES, WAVENET_HEAD_CASES, MULTI_CASES, SRNN_OPTION_CASES,
S2S_OPTION_CASES): kernel sizes, gates and activations, layer order, layerwise inputs, affine residuals, deeper and narrower heads,
conditioning, several inputs and targets, stacked recurrent layers, h0_init, inputs_mode, weight norm, every pooling / upsampling pair and
asymmetric stacks - on the per-layer launch path or the pipelines' padded heads, asserted through the same flags.

Class networks: last_logits after every block against R64 of the device's own history (check_outputs: 4 max(E) and 4 rms(E)), the class of
EVERY step against R64's argmax within 2 tol_max (check_picks), and the four defects of net_refs.py and the case's option defects on the
same rows (check_near_miss).  A network of several targets: last_logits(B, target) of every target against that target's own reference, E
and tolerance, and that target's stream against check_picks.
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

The option cases (WAVENET_OPTION_CASES, WAVENET_HEAD_CASES, MULTI_CASES, SRNN_OPTION_CASES, S2S_OPTION_CASES), first run on an MI355X; a
network of several targets has one line per target (its own reference, E and tolerance):

  wavenet     opt-mlp2                               20817  1.62         0.83       0.68  6.371e-07  1.095e-07
  wavenet     opt-mlp3_cond                          20817  2.37         0.87       0.80  8.035e-07  1.691e-07
  wavenet     opt-nogate                             20817  7.09         1.20       0.77  2.113e-06  4.873e-07
  wavenet     opt-nogate_cond                        20817  6.46         1.09       0.80  2.222e-06  4.850e-07
  wavenet     opt-rev                                20817  1.44         0.69       0.63  5.337e-07  1.097e-07
  wavenet     opt-rev_noskip                         20817  1.67         1.19       0.61  5.005e-07  1.114e-07
  wavenet     opt-lw                                 20817  4.75         1.00       0.76  1.633e-06  2.283e-07
  wavenet     opt-lw_noskip_rev                      20817  5.98         0.84       0.79  1.539e-06  2.874e-07
  wavenet     opt-tied                               20817  2.38         0.65       0.74  7.813e-07  1.428e-07
  wavenet     opt-k3                                 20817  2.85         0.65       0.72  1.013e-06  1.672e-07
  wavenet     opt-k3_cond                            20817  4.12         0.90       0.75  1.454e-06  2.837e-07
  wavenet     opt-k4_noskip                          20817  0.996        0.67       0.65  3.903e-07  7.853e-08
  wavenet     opt-aff                                20817  4.72         0.93       0.79  5.545e-06  6.093e-07
  wavenet     opt-aff_nogate_noskip                  20817  3.75         0.91       0.85  2.305e-05  1.718e-06
  wavenet     act-mish_tanh                          20817  0.424        1.00       0.66  1.053e-07  1.968e-08
  wavenet     act-relu_nogate                        20817  0.822        1.11       0.93  2.165e-07  4.008e-08
  wavenet     act-sin_sig_cond                       20817  1.28         1.17       0.80  2.895e-07  5.827e-08
  wavenet     act-softplus_abs                       20817  0.769        0.86       0.92  2.632e-07  4.551e-08
  wavenet     act-id_cos_noskip                      20817  1.3          0.97       0.89  3.788e-07  6.509e-08
  wavenet     act-abs_nogate_cond                    20817  3            1.20       0.99  8.666e-07  1.746e-07
  wavenet     head-wn_relu_dp                        20817  3.13         0.88       0.71  7.356e-07  1.598e-07
  wavenet     head-wn_tanh_2                         20817  2.54         0.64       0.67  1.070e-06  1.980e-07
  wavenet     frames-g1                              13365  0.18         0.38       0.23  9.165e-08  2.204e-08
  wavenet     frames-g2abs                           13365  0.156        0.31       0.20  8.698e-08  2.207e-08
  wavenet     spipe-narrow-200-100-33                59697  4.39         0.43       0.37  2.423e-06  5.450e-07
  wavenet     bpipe-narrow-200-100-33                59697  4.39         0.72       0.61  2.423e-06  5.450e-07
  wavenet     spipe-narrow-64-40-9                    5265  1.99         0.60       0.43  1.196e-06  3.168e-07
  wavenet     lpipe-narrow-200-112-40                72360  1.32         0.55       0.58  6.633e-07  1.333e-07
  wavenet     lpipe-narrow-64-32-13                   7605  1.92         0.67       0.67  8.998e-07  2.112e-07
  wavenet     multi-wn_2x2 target 0                  20817  2.46         0.91       0.77  9.559e-07  1.958e-07
  wavenet     multi-wn_2x2 target 1                   5265  1.74         1.07       0.77  6.578e-07  1.485e-07
  wavenet     multi-wn_2x1 target 0                  20817  2.54         0.73       0.73  8.007e-07  1.630e-07
  wavenet     multi-wn_3x3_noskip target 0           10449  0.975        1.01       0.81  3.152e-07  6.948e-08
  wavenet     multi-wn_3x3_noskip target 1            5265  1.11         0.98       0.79  2.941e-07  7.076e-08
  wavenet     multi-wn_3x3_noskip target 2            1377  0.742        1.34       0.87  1.703e-07  4.980e-08
  sample_rnn  opt-gru_n2                             31097  3.9          0.76       0.83  1.575e-06  1.886e-07
  sample_rnn  opt-lstm_n3                            31097  4.51         0.95       0.85  8.359e-07  1.285e-07
  sample_rnn  opt-rnn_n2_mlp2                        31097  5.66         0.75       0.76  2.195e-06  3.200e-07
  sample_rnn  opt-gru_mean                           31097  3.15         0.85       0.83  1.037e-06  1.771e-07
  sample_rnn  opt-lstm_mix_ones                      31097  3.2          1.11       0.85  7.313e-07  1.320e-07
  sample_rnn  weight_norm-gru                        31097  6.81         0.75       0.81  2.325e-06  2.336e-07
  sample_rnn  weight_norm-lstm                       31097  5.72         1.04       0.83  1.321e-06  1.366e-07
  sample_rnn  head-srnn_softplus_dp1d                31097  385          0.92       0.87  1.231e-03  1.157e-04
  sample_rnn  head-srnn_sigmoid                      31097  14.8         0.57       0.73  1.191e-04  9.506e-06
  sample_rnn  multi-srnn_sum_2x2 target 0            25443  5.21         0.92       0.81  1.703e-06  2.671e-07
  sample_rnn  multi-srnn_sum_2x2 target 1             6435  4.1          1.17       0.80  1.198e-06  2.735e-07
  sample_rnn  multi-srnn_mix_2x1 target 0            25443  2.31         0.90       0.82  5.130e-07  9.772e-08
  sample_rnn  multi-srnn_mean_3x3 target 0           25443  3.87         0.73       0.79  1.882e-06  3.020e-07
  sample_rnn  multi-srnn_mean_3x3 target 1            6435  2.23         0.91       0.80  9.885e-07  1.898e-07
  sample_rnn  multi-srnn_mean_3x3 target 2            3267  3.69         0.54       0.76  2.264e-06  3.088e-07
  seq2seq     edge_mean-linear_resample              24960  0.362        0.60       0.95  2.341e-07  3.816e-08
  seq2seq     sum-linear_resample                    24960  0.941        0.50       0.56  6.226e-07  1.168e-07
  seq2seq     edge_sum-repeat                        24960  0.503        0.97       0.82  2.584e-07  5.870e-08
  seq2seq     linear_resample-interp                 24960  0.444        0.78       0.91  2.473e-07  4.791e-08
  seq2seq     edge_sum-interp                        24960  0.61         0.80       0.84  3.071e-07  6.101e-08
  seq2seq     linear_resample-linear_resample        24960  0.341        0.99       0.97  1.693e-07  3.857e-08
  seq2seq     stack-e2d1                             24960  0.265        1.06       0.98  1.627e-07  3.960e-08
  seq2seq     stack-e1d3                             24960  0.326        1.05       1.03  1.571e-07  3.813e-08
  seq2seq     stack-e3d1res_sum                      24960  0.937        0.58       0.66  6.921e-07  1.487e-07
  seq2seq     classes-mlp2_stack                     24672  0.165        0.79       0.69  6.113e-08  1.376e-08
  seq2seq     two_inputs                             24960  0.736        0.68       0.67  3.297e-07  7.021e-08

The option paths lie at the reference's own fp32 error too (ratios 0.3 .. 1.34, the rms ratios 0.2 .. 1.03): the launch path's libm gates
(tanhf / expf / log1pf / sinf) sit nearer R32 than the step kernels' fast formulas, as supposed, and no option case needed a finding.  The
head of scale 385 (gain-8 recipe, Softplus) has a max(E) of 1.2e-3, which is 3e-6 of its scale; the affine residuals' 2.3e-5 is the squared
terms of x_hat a + b layer after layer - both are the reference's own error, and the device sits at 0.9 of it.

"""
import pytest
import torch

import mimikit_amd as mmk
from tests import net_refs as R
from tests.plan_driver import generate as _generate, switch as _switch

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)


def _against_float64(case, device, monkeypatch, what):
    _switch(monkeypatch, case)
    hist, dev = _generate(case, device, what)
    _, conds = case.inputs()
    envs = R.envelope(hist, case, conds)
    rows = case.rows()
    tols, failed = [], []
    # a network of several targets: every target's outputs against its own reference, its own E and its own tolerance
    for k, (dev_k, env_k) in enumerate(zip(R.per_target(dev), R.per_target(envs))):
        what_k = f"{what} target {k}" if case.multi else what
        R64, E = env_k.R64[:, rows], env_k.E[:, rows]
        assert dev_k.shape == R64.shape, (what_k, dev_k.shape, R64.shape)
        tol_max, tol_rms = R.tolerance(E)
        tols.append(tol_max)
        r_max, r_rms = R.ratios(dev_k, R64, E)
        print(f"[f64] {what_k}: {dev_k.numel()} outputs of scale {float(R64.abs().max()):.3g}; max|dev - R64| / max(E) = {r_max:.2f}, rms(dev - R64) / rms(E) = {r_rms:.2f} "
              f"(the margin allows {R.FACTOR:g}); max(E) {float(E.max()):.3e}, rms(E) {R.rms(E):.3e}")
        try:
            R.check_outputs(dev_k, R64, tol_max, tol_rms, what_k)
            if case.classes:
                R.check_picks(R.streams(hist)[k][:, case.P:], env_k.R64, tol_max, what_k)
        except AssertionError as err:      # (every target's figures are printed before the first failure is raised)
            failed.append(err)
    if failed:
        raise failed[0]
    R64, tol_max = R.per_target(envs)[0].R64[:, rows], tols[0]      # (the split-K check below: one target)
    full = [e.R64 for e in R.per_target(envs)]
    for name, out in R.defects(case, hist, conds, full if case.multi else full[0]):
        R.check_near_miss([o[:, rows] for o in R.per_target(out)], [r[:, rows] for r in full], tols, f"{what} {name}")
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


@pytest.mark.parametrize("case", R.WAVENET_ALL, ids=[c.id for c in R.WAVENET_ALL])
def test_wavenet_steps_within_the_float64_envelope(device, monkeypatch, case):
    """launch path, wavenet_persist, wavenet_chain, wavenet_lpipe (a ragged group of eight; rf 1024: the long rings), wavenet_spipe (one clip and
    two clips per visit), wavenet_bpipe (16 + a ragged 4), conditioned variants, the per-step warm-up, a magnitude-frame net; prompt rf + 3,
    blocks of 1 .. 9 steps: nine rows per clip, ends on every small ring phase.  The option cases: 16 channels x 5 layers x 9 clips on the launch
    path (every tag of helpers.WAVENET_OPTIONS / WAVENET_ACTS, two MLP heads, two more magnitude-frame nets), the stage, batch and layer pipelines
    with heads narrower than their 128 x 256, and networks of several class inputs and targets"""
    _against_float64(case, device, monkeypatch, f"wavenet {case.id}")


@pytest.mark.parametrize("case", R.SRNN_ALL, ids=[c.id for c in R.SRNN_ALL])
def test_sample_rnn_steps_within_the_float64_envelope(device, monkeypatch, case):
    """hidden 128 (one case 512): one launch per op, the one-clip and four-clip bottom kernels, the tier kernel with its up-sampler apart, tanh
    tiers and stacked layers, resident mode (GRU and LSTM, frames of 1 and 2 samples, ragged row tiles, both warm-ups); prompt 2 rf + 3; resident
    blocks at least two periods long that end on four residues of the period, each of them one resident launch.  The option cases: hidden 32,
    11 clips, one launch per op: stacked layers, a deeper head, inputs_mode, h0_init ones, weight norm, two more head activations, and
    networks of several class inputs and targets"""
    _against_float64(case, device, monkeypatch, f"sample_rnn {case.id}")


@pytest.mark.parametrize("case", R.S2S_ALL, ids=[c.id for c in R.S2S_ALL])
def test_seq2seq_steps_within_the_float64_envelope(device, monkeypatch, case):
    """magspec n_fft 128: the resident bi-LSTM over its geometry (stacked layers with and without residuals), one launch per frame, one launch per
    op, the output projection split over K two and three ways (model_dim 256: four stages, batch x hop = 128) where the launch itself would split it
    four ways, another pooling / upsampling pair, and the class path; three chained steps each.  The option cases (model_dim 128, hop 8, 16
    clips): the other pooling / upsampling pairs, asymmetric stacks, the class path with a deeper head on a stacked decoder with residuals, and
    two frame inputs added up (step by step: that network has no block path)"""
    _against_float64(case, device, monkeypatch, f"seq2seq {case.id}")
