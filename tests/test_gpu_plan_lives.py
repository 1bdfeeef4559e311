"""A plan outlives a generation: every case of test_gpu_networks_f64.py and test_gpu_transformer_f64.py runs FOUR generations on one network
object and one plan (net_refs.lives, transformer_refs.lives), through the networks' own lifecycle (before_generate, generate_block,
after_generate - tests/plan_driver.py), the way GenerateLoopV2's further batches, EnsembleGenerator's events and every validation epoch do:

  life  clips                  prompt                    blocks                inputs
  1     B                      P                         the case's            the case's
  2     B                      P + 5                     a prefix of them      another draw
  3     max(1, B // 2 - 1)     the shortest allowed      the same prefix       a third draw
  4     B                      P                         the case's            the case's again

A fresh workspace is all zeros, which is the right start for hidden states, tier outputs, tags and counters: what a reset misses shows only
on a plan's second life.  Life 2 starts BELOW where life 1 ended, so the tags and ring slots of life 1 lie ahead of it, on other ring phases
(the WaveNet warm-up starts at position 8 instead of 3, the SampleRNN warm-up offset is 8; Seq2Seq has no prompt beyond `hop`: only the
content changes).  Life 3 is ragged against the groups of 2, 4 and 16 the kernels work in (5 -> 1, 8 -> 3, 9 -> 3, 11 -> 4, 13 -> 5, 16 -> 7,
17 -> 7, 20 -> 9, 21 -> 9, 24 -> 11, 33 -> 15, 40 -> 19, 128 -> 63, 130 -> 64, 2 / 3 / 4 -> 1) behind the shortest prompt (rf: the warm-up
starts at position 0; frame_sizes[0]: no warm-up step at all).  No geometry had to be substituted: the oracle and the four networks take
these lengths.  Held per case:

  same plan      after every life net._plan is the object life 1 made, net._plan_batch is B and native.pack_launch_count() has not moved;
                 case.ran(plan, k) after every block with k counted over the plan's whole life (the resident counters go on counting:
                 resident warm-ups 1, 2, 2, 3 after the four lives - life 3 has no warm-up step), sync_status after every block of a
                 plan whose kernels wait for each other
  life 2         bit for bit the history and every last_logits row of a FRESH network and plan that run life 2 alone (same clips, same
                 Bmax: the same kernels) - after two fresh networks gave each other's bits; and inside the float64 envelope of its own
                 history (R.envelope, R.tolerance, check_outputs, check_picks on every step; of more than five clips the first four
                 and the last: the bitwise leg covers all of them)
  life 3         inside the float64 envelope of its own history, every clip (a fresh plan of another Bmax takes another K split and
                 another bottom kernel: no bitwise leg); last_logits into a buffer of B rows of NaN leaves the rows from `clips` on NaN
  life 4         bit for bit life 1: same plan, same inputs - pure state isolation

The transformer's lives 2 and 3 also run every step teacher-forced (generate_step over the same windows, as test_gpu_transformer_f64.py
does), so that the steps whose window still holds the prompt are compared rows and not only picks.

One flag follows the call's batch, not the plan's: spipe-pair-24 runs two clips per visit in lives 1, 2 and 4 and ONE clip per visit in life
3 (11 clips: wn_spipe_pair_form wants an even count of 24 .. 128, csrc/wavenet_spipe.h; net_refs.spipe_pair_form restates it and
net_refs.Life asserts the other flag for that life).  Every other flag is the plan's and is asserted as the case states it.

What a defect of this kind does to the references alone - a prompt, a ragged group's rows or tier states of the life before - is in
test_net_refs.py / test_transformer_refs.py (defects (e), (f), (g)): each leaves tol_max.

First run on an MI355X, per case (and per target): the compared outputs, max|dev - R64| / max(E), rms(dev - R64) / rms(E) and max(E), for
life 2 (left) and life 3 (right).  Records, not tolerances - the tolerance is recomputed from the reference on every run, the margin allows 4:

                                                                  life 2                              life 3
  network     case                                                 outputs   max   rms     max(E)    outputs   max   rms     max(E)
  wavenet     launches                                                6425  0.76  0.74  6.465e-07       1285  0.66  0.59  7.258e-07
  wavenet     persist                                                 6425  0.82  0.75  6.465e-07       1285  0.62  0.65  7.258e-07
  wavenet     chain                                                   6425  0.55  0.68  6.465e-07       1285  0.67  0.75  7.258e-07
  wavenet     chain-cond                                              6425  0.78  0.67  1.079e-06       1285  0.64  0.66  1.266e-06
  wavenet     chain-step_warmup                                       6425  0.56  0.68  6.465e-07       1285  0.67  0.75  7.258e-07
  wavenet     lpipe-4_3-13                                            6425  0.69  0.60  9.502e-07       6425  0.80  0.60  8.087e-07
  wavenet     lpipe-10-8                                              6425  0.74  0.63  1.583e-06       3855  0.51  0.63  2.010e-06
  wavenet     lpipe-cond                                              6425  0.46  0.52  2.718e-06       6425  0.44  0.51  2.759e-06
  wavenet     spipe-5                                                 6425  0.63  0.53  3.471e-07       1285  0.77  0.55  2.975e-07
  wavenet     spipe-cond                                              6425  0.41  0.35  1.398e-06       1285  0.39  0.45  1.216e-06
  wavenet     spipe-pair-24                                           6425  0.51  0.51  4.255e-07      14135  0.66  0.51  3.669e-07
  wavenet     bpipe-20                                                6425  0.84  0.64  3.608e-07      11565  0.87  0.64  4.603e-07
  wavenet     frames-g4                                               2475  0.31  0.23  8.170e-08        495  0.38  0.26  6.721e-08
  wavenet     opt-mlp2                                                6425  0.62  0.71  5.875e-07       3855  1.00  0.95  7.121e-07
  wavenet     opt-mlp3_cond                                           6425  1.04  0.81  7.301e-07       3855  0.78  0.75  6.063e-07
  wavenet     opt-nogate                                              6425  1.04  0.82  1.833e-06       3855  0.59  0.74  2.592e-06
  wavenet     opt-nogate_cond                                         6425  0.80  0.77  2.060e-06       3855  0.93  0.81  2.125e-06
  wavenet     opt-rev                                                 6425  0.65  0.65  5.634e-07       3855  0.75  0.63  4.365e-07
  wavenet     opt-rev_noskip                                          6425  0.73  0.65  4.508e-07       3855  0.71  0.63  4.493e-07
  wavenet     opt-lw                                                  6425  1.11  0.80  8.633e-07       3855  0.99  0.83  8.891e-07
  wavenet     opt-lw_noskip_rev                                       6425  0.93  0.79  1.366e-06       3855  1.03  0.78  1.027e-06
  wavenet     opt-tied                                                6425  0.83  0.72  7.033e-07       3855  0.67  0.76  7.581e-07
  wavenet     opt-k3                                                  6425  0.69  0.75  8.096e-07       3855  0.88  0.68  6.109e-07
  wavenet     opt-k3_cond                                             6425  0.93  0.79  1.075e-06       3855  0.98  0.78  1.016e-06
  wavenet     opt-k4_noskip                                           6425  0.85  0.70  3.176e-07       3855  0.71  0.61  2.730e-07
  wavenet     opt-aff                                                 6425  0.97  0.81  4.605e-06       3855  1.44  0.91  1.944e-06
  wavenet     opt-aff_nogate_noskip                                   6425  0.57  0.72  1.512e-05       3855  0.68  0.81  2.413e-05
  wavenet     act-mish_tanh                                           6425  0.79  0.72  1.020e-07       3855  1.08  0.70  1.028e-07
  wavenet     act-relu_nogate                                         6425  0.82  0.81  2.078e-07       3855  0.92  0.92  2.099e-07
  wavenet     act-sin_sig_cond                                        6425  0.88  0.77  2.619e-07       3855  0.79  0.78  2.621e-07
  wavenet     act-softplus_abs                                        6425  1.05  0.90  2.074e-07       3855  0.91  0.93  1.841e-07
  wavenet     act-id_cos_noskip                                       6425  1.13  0.93  2.905e-07       3855  1.03  0.89  3.279e-07
  wavenet     act-abs_nogate_cond                                     6425  0.75  0.98  9.183e-07       3855  0.70  0.91  1.150e-06
  wavenet     head-wn_relu_dp                                         6425  1.25  0.76  6.034e-07       3855  1.16  0.76  4.713e-07
  wavenet     head-wn_tanh_2                                          6425  0.71  0.62  8.844e-07       3855  0.71  0.59  7.802e-07
  wavenet     frames-g1                                               2475  0.41  0.28  9.245e-08       1485  0.45  0.29  7.409e-08
  wavenet     frames-g2abs                                            2475  0.33  0.26  8.151e-08       1485  0.34  0.24  7.903e-08
  wavenet     spipe-narrow-200-100-33                                 5025  0.62  0.39  1.689e-06      15075  0.40  0.39  2.166e-06
  wavenet     bpipe-narrow-200-100-33                                 5025  1.01  0.63  1.689e-06      15075  0.83  0.61  2.166e-06
  wavenet     spipe-narrow-64-40-9                                    1625  0.54  0.42  1.047e-06        975  0.54  0.47  9.647e-07
  wavenet     lpipe-narrow-200-112-40                                 5025  0.60  0.56  5.280e-07      19095  0.49  0.57  6.362e-07
  wavenet     lpipe-narrow-64-32-13                                   1625  0.78  0.67  7.525e-07       1625  0.83  0.63  6.664e-07
  wavenet     multi-wn_2x2 target 0                                   6425  1.21  0.83  6.864e-07       3855  0.69  0.71  7.324e-07
  wavenet     multi-wn_2x2 target 1                                   1625  0.66  0.74  6.202e-07        975  1.05  0.79  4.711e-07
  wavenet     multi-wn_2x1 target 0                                   6425  0.84  0.73  6.394e-07       3855  0.98  0.72  5.136e-07
  wavenet     multi-wn_3x3_noskip target 0                            3225  0.85  0.85  2.559e-07       1935  0.87  0.79  2.665e-07
  wavenet     multi-wn_3x3_noskip target 1                            1625  0.87  0.81  2.522e-07        975  1.09  0.84  2.765e-07
  wavenet     multi-wn_3x3_noskip target 2                             425  0.78  0.80  1.895e-07        255  0.88  0.89  1.515e-07
  sample_rnn  launches                                                6425  0.42  0.51  1.732e-06      11565  0.54  0.48  1.149e-06
  sample_rnn  bottom-one_clip                                         6425  0.31  0.37  1.732e-06      11565  0.40  0.34  1.149e-06
  sample_rnn  bottom-four_clips-321                                   8050  0.49  0.44  1.184e-06      14490  0.48  0.44  1.370e-06
  sample_rnn  tier-up_apart                                           6425  0.31  0.34  1.216e-06      11565  0.29  0.34  1.169e-06
  sample_rnn  rnn_tanh                                                6425  0.32  0.44  2.671e-06       1285  1.02  0.77  7.855e-07
  sample_rnn  n_rnn_2                                                 6425  0.45  0.40  1.112e-06       1285  0.63  0.50  6.170e-07
  sample_rnn  resident-gru                                            2570  0.32  0.31  1.063e-06       4626  0.22  0.34  2.160e-06
  sample_rnn  resident-lstm                                           2570  0.25  0.32  1.235e-06       4626  0.36  0.34  1.010e-06
  sample_rnn  resident-32_8_2-33                                      2570  0.37  0.38  1.143e-06       7710  0.27  0.32  1.434e-06
  sample_rnn  resident-gru-512-40                                     2570  0.30  0.33  1.585e-06       9766  0.30  0.31  1.671e-06
  sample_rnn  resident-warmup_1                                       2570  0.39  0.32  1.070e-06       4626  0.32  0.28  1.631e-06
  sample_rnn  resident-warmup_0                                       2570  0.36  0.32  1.070e-06       4626  0.32  0.28  1.631e-06
  sample_rnn  opt-gru_n2                                              6425  1.33  0.90  7.412e-07       5140  0.93  0.84  8.765e-07
  sample_rnn  opt-lstm_n3                                             6425  1.27  0.83  4.983e-07       5140  1.05  0.83  6.671e-07
  sample_rnn  opt-rnn_n2_mlp2                                         6425  0.72  0.65  1.611e-06       5140  0.75  0.69  1.121e-06
  sample_rnn  opt-gru_mean                                            6425  0.76  0.88  1.052e-06       5140  1.00  0.83  7.040e-07
  sample_rnn  opt-lstm_mix_ones                                       6425  1.14  0.89  5.583e-07       5140  1.02  0.73  5.917e-07
  sample_rnn  weight_norm-gru                                         6425  0.88  0.89  1.296e-06       5140  1.00  0.83  1.303e-06
  sample_rnn  weight_norm-lstm                                        6425  1.31  0.81  7.394e-07       5140  1.14  0.88  6.859e-07
  sample_rnn  head-srnn_softplus_dp1d                                 6425  0.97  0.92  1.030e-03       5140  0.68  0.63  4.555e-04
  sample_rnn  head-srnn_sigmoid                                       6425  0.76  0.70  7.143e-05       5140  0.26  0.45  5.443e-05
  sample_rnn  multi-srnn_sum_2x2 target 0                             6425  1.07  0.89  1.046e-06       3855  2.14  1.12  6.547e-07
  sample_rnn  multi-srnn_sum_2x2 target 1                             1625  0.79  0.79  1.517e-06        975  1.31  1.04  7.930e-07
  sample_rnn  multi-srnn_mix_2x1 target 0                             6425  1.29  0.79  4.111e-07       3855  1.17  0.96  3.140e-07
  sample_rnn  multi-srnn_mean_3x3 target 0                            6425  0.54  0.87  1.832e-06       3855  1.26  1.02  7.715e-07
  sample_rnn  multi-srnn_mean_3x3 target 1                            1625  1.35  0.90  7.232e-07        975  1.16  0.92  5.045e-07
  sample_rnn  multi-srnn_mean_3x3 target 2                             825  0.81  0.78  1.068e-06        495  0.84  0.84  9.160e-07
  seq2seq     resident-128-2-3                                         780  1.22  0.92  1.305e-07        260  0.86  1.05  1.314e-07
  seq2seq     resident-256-5-17                                       3250  0.82  0.80  1.928e-07       4550  0.93  0.82  1.748e-07
  seq2seq     resident-512-3-33                                       1950  1.00  0.78  1.728e-07       5850  0.63  0.75  2.393e-07
  seq2seq     resident-128-7-128                                      4550  0.79  0.87  2.260e-07      57330  0.73  0.80  2.717e-07
  seq2seq     resident-128-8-16-2layers                               5200  0.85  1.02  1.668e-07       7280  0.79  1.01  1.926e-07
  seq2seq     resident-128-8-16-2layers-residuals                     5200  0.61  0.75  5.835e-07       7280  0.77  0.75  5.000e-07
  seq2seq     per_frame                                               5200  0.92  0.97  1.433e-07       7280  0.73  0.93  1.926e-07
  seq2seq     launches                                                5200  0.30  0.26  1.433e-07       7280  0.19  0.21  1.926e-07
  seq2seq     ksplit-2                                                5200  1.29  0.85  1.661e-07       7280  0.82  0.83  2.160e-07
  seq2seq     ksplit-3                                                5200  1.11  0.84  1.661e-07       7280  0.82  0.83  2.160e-07
  seq2seq     mean-repeat                                             5200  0.93  0.88  1.746e-07       7280  0.88  0.92  1.820e-07
  seq2seq     classes                                                10280  0.79  0.94  1.043e-07      22616  0.93  0.95  1.100e-07
  seq2seq     edge_mean-linear_resample                               5200  1.03  0.97  1.493e-07       7280  1.00  0.96  1.489e-07
  seq2seq     sum-linear_resample                                     5200  0.56  0.58  5.008e-07       7280  0.54  0.55  5.973e-07
  seq2seq     edge_sum-repeat                                         5200  0.78  0.81  2.536e-07       7280  0.70  0.81  3.005e-07
  seq2seq     linear_resample-interp                                  5200  0.92  0.89  2.329e-07       7280  1.04  0.86  1.914e-07
  seq2seq     edge_sum-interp                                         5200  0.79  0.76  2.983e-07       7280  0.70  0.79  2.838e-07
  seq2seq     linear_resample-linear_resample                         5200  0.87  0.95  1.607e-07       7280  0.77  0.94  1.710e-07
  seq2seq     stack-e2d1                                              5200  1.01  0.96  1.531e-07       7280  1.02  0.99  1.487e-07
  seq2seq     stack-e1d3                                              5200  0.98  1.02  1.559e-07       7280  0.98  1.01  1.510e-07
  seq2seq     stack-e3d1res_sum                                       5200  0.67  0.68  6.126e-07       7280  0.52  0.64  7.413e-07
  seq2seq     classes-mlp2_stack                                      5140  0.80  0.73  4.786e-08       7196  0.63  0.70  5.953e-08
  seq2seq     two_inputs                                              5200  0.60  0.70  3.651e-07       7280  0.59  0.69  3.687e-07
  transformer one_layer_rf9 last_logits after the blocks              2313  0.69  0.72  2.973e-06        771  0.88  0.81  2.089e-06
  transformer one_layer_rf9 every step                               30840  0.90  0.81  2.973e-06      10280  1.06  0.78  2.180e-06
  transformer clips130_rf2 last_logits after the blocks               3855  0.69  0.66  2.220e-06      49344  0.69  0.69  2.220e-06
  transformer clips130_rf2 every step                                51400  0.77  0.68  2.442e-06     657920  0.93  0.68  2.804e-06
  transformer ff24_rf33 last_logits after the blocks                  3084  0.66  0.85  2.144e-06        771  0.62  0.73  1.918e-06
  transformer ff24_rf33 every step                                   41120  0.99  0.84  2.577e-06      10280  0.99  0.81  2.138e-06
  transformer ff8_rf33 last_logits after the blocks                   3084  1.13  0.82  2.647e-06        771  0.65  0.58  3.098e-06
  transformer ff8_rf33 every step                                    41120  0.94  0.80  3.184e-06      10280  0.61  0.69  3.891e-06
  transformer frames130_rf2 every frame                               1615  0.94  0.83  1.433e-06      20672  0.75  0.80  2.068e-06
  transformer layer_norm_rf65 last_logits after the blocks            1542  1.18  0.78  2.391e-06        771  0.84  0.76  2.332e-06
  transformer layer_norm_rf65 every step                             20560  0.90  0.80  3.473e-06      10280  1.22  0.83  2.839e-06
  transformer head_dim128 last_logits after the blocks                1028  0.46  0.42  3.699e-06        514  0.64  0.43  2.464e-06
  transformer head_dim128 every step                                  9766  0.52  0.47  4.098e-06       4883  0.68  0.50  3.776e-06
  transformer default last_logits after the blocks                    1028  0.58  0.59  3.983e-06        514  0.50  0.49  2.784e-06
  transformer default every step                                      9766  0.58  0.53  4.022e-06       4883  0.78  0.54  3.561e-06

Every life of every case lies at the reference's own fp32 error, where the fresh plans of test_gpu_networks_f64.py lie (max ratios 0.19 ..
2.14, rms 0.21 .. 1.12; the largest, 2.14, is the one-launch-per-op SampleRNN of two targets on 3 clips, whose max(E) is taken over 3855
outputs only).  No life left the envelope, life 2 gave the fresh plan's bits and life 4 gave life 1's bits in all 100 cases: no reset, warm-up,
graph key or ragged group needed a fix.  With mmk_srnn_reset skipped (tried once beside the tests, on the launch-per-op SampleRNN cases) lives
2 and 3 lie 1e6 max(E) off and the bitwise legs fail: the test sees a carried state.

Bit-deterministic run to run (two fresh networks and plans, life 2), confirmed on that run for every case, so for every mode: WaveNet - the
per-layer launch path (classes and frames, every option), wavenet_persist, wavenet_chain (with the prefill and the per-step warm-up),
wavenet_lpipe, wavenet_spipe with one and with two clips per visit, wavenet_bpipe, the padded heads; SampleRNN - one launch per op, the
one-clip and four-clip bottom kernels, the tier kernel with its up-sampler apart, resident mode (GRU, LSTM, hidden 512, both warm-ups);
Seq2Seq - the resident bi-LSTM, one launch per frame, one launch per op, both forced K splits, the class path; the transformer - plain steps
and the replayed graph.  NOT_BIT_DETERMINISTIC is empty.
"""
import pytest
import torch

from mimikit_amd import native
from tests import net_refs as R
from tests import plan_driver as D
from tests import transformer_refs as T

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

# cases whose kernels turned out not to give equal bits run to run: their bitwise legs fall back to the envelope (none so far)
NOT_BIT_DETERMINISTIC = {}


def _bits(x):
    return x.contiguous().view(torch.int32) if x.dtype == torch.float32 else x


def _same_bits(a, b):
    a, b = [t for x in a for t in R.per_target(x)], [t for x in b for t in R.per_target(x)]
    return len(a) == len(b) and all(x.shape == y.shape and x.dtype == y.dtype and torch.equal(_bits(x), _bits(y)) for x, y in zip(a, b))


def _record(what, dev, R64, E):
    r_max, r_rms = R.ratios(dev, R64, E)
    print(f"[lives] {what}: {dev.numel()} outputs of scale {float(R64.abs().max()):.3g}; max|dev - R64| / max(E) = {r_max:.2f}, rms(dev - R64) / rms(E) = {r_rms:.2f} "
          f"(the margin allows {R.FACTOR:g}); max(E) {float(E.max()):.3e}, rms(E) {R.rms(E):.3e}")


def _some_clips(clips):
    """life 2: of more than five clips the first four and the last"""
    return None if clips <= 5 else [0, 1, 2, 3, clips - 1]


def _within_the_envelope(life, what, hist, dev, sel=None):
    """the float64 test's check of one generation: every target against its own reference, E and tolerance; every pick of every step"""
    _, conds = life.inputs()
    if sel is not None:
        hist = tuple(x[sel] for x in hist) if life.multi else hist[sel]
        dev = [d[sel] for d in dev] if life.multi else dev[sel]
        conds = tuple(c[sel] for c in conds)
    envs = R.envelope(hist, life, conds)
    rows = life.rows()
    failed = []
    for k, (dev_k, env_k) in enumerate(zip(R.per_target(dev), R.per_target(envs))):
        what_k = f"{what} target {k}" if life.multi else what
        R64, E = env_k.R64[:, rows], env_k.E[:, rows]
        assert dev_k.shape == R64.shape, (what_k, dev_k.shape, R64.shape)
        tol_max, tol_rms = R.tolerance(E)
        _record(what_k, dev_k, R64, E)
        try:
            R.check_outputs(dev_k, R64, tol_max, tol_rms, what_k)
            if life.classes:
                R.check_picks(R.streams(hist)[k][:, life.P:], env_k.R64, tol_max, what_k)
        except AssertionError as err:      # (every target's figures are printed before the first failure is raised)
            failed.append(err)
    if failed:
        raise failed[0]


def _nothing_behind_the_batch(life, B, what):
    """after every block of life 3: last_logits of its `clips` clips into B rows of NaN"""
    def look(plan):
        for target in range(life.targets):
            got = plan.last_logits(life.clips) if life.kind == "s2s_classes" else plan.last_logits(life.clips, target)
            out = torch.full((B, *got.shape[1:]), float("nan"), device=got.device)
            D.logits_into(life, plan, life.clips, out, target)
            out = out.cpu()
            assert _same_bits([out[:life.clips]], [got.cpu()]), (what, target, "the caller's buffer got other rows than last_logits hands back")
            assert bool(out[life.clips:].isnan().all()), (what, target, f"{int((~out[life.clips:].isnan()).sum())} elements behind the batch were written")
    return look


def _four_lives(case, device, monkeypatch, what):
    D.switch(monkeypatch, case)
    B = case.clips
    net = case.make()[0].to(device)
    ran, blocks, warmups, plan, packs = {}, 0, 0, None, None
    for life in R.lives(case):
        warmups += int(life.kind == "srnn" and life.whole_period_warmup)
        look = _nothing_behind_the_batch(life, B, f"{what} life 3") if life.index == 3 and life.classes else None
        ran[life.index] = D.generate(life, device, f"{what} life {life.index}", net=net, blocks_before=blocks, warmups=warmups, after_block=look)
        blocks += len(life.parts)
        if life.index == 1:
            plan, packs = net._plan, native.pack_launch_count()
        print(f"[lives] {what} life {life.index}: {life.clips} clips, prompt {life.P}, {life.n} steps; the plan reports {R.flags(life, net._plan)}")
        assert net._plan is plan and net._plan_batch == B, (what, life.index, "the plan was replaced", net._plan_batch)
        assert native.pack_launch_count() == packs, (what, life.index, "the weights were packed again")
    _, two, three, _ = R.lives(case)
    failed = []
    for life in (two, three):
        try:
            _within_the_envelope(life, f"{what} life {life.index}", *ran[life.index], sel=_some_clips(life.clips) if life.index == 2 else None)
        except AssertionError as err:      # (the figures of both lives and the bitwise legs are looked at before the first failure is raised)
            failed.append(err)
    fresh = [D.generate(two, device, f"{what} life 2 on a fresh plan", warmups=int(two.kind == "srnn" and two.whole_period_warmup)) for _ in range(2)]
    deterministic = _same_bits(fresh[0], fresh[1])
    print(f"[lives] {what}: two fresh plans give {'equal' if deterministic else 'OTHER'} bits in life 2")
    if case.id in NOT_BIT_DETERMINISTIC.get(case.kind, ()):
        for k, run in enumerate(fresh):    # (the fallback the module docstring describes: each run inside the envelope instead)
            _within_the_envelope(two, f"{what} life 2 on fresh plan {k}", *run, sel=_some_clips(two.clips))
    else:
        assert deterministic, (what, "two fresh networks and plans disagree bitwise in life 2: the mode is not deterministic")
        assert _same_bits(ran[2], fresh[0]), (what, "life 2 on the plan life 1 ran on differs bitwise from life 2 on a fresh plan")
        assert _same_bits(ran[4], ran[1]), (what, "life 4 differs bitwise from life 1: same plan, same inputs")
    if failed:
        raise failed[0]


@pytest.mark.parametrize("case", R.WAVENET_ALL, ids=[c.id for c in R.WAVENET_ALL])
def test_wavenet_plan_lives(device, monkeypatch, case):
    """dilation queues and private rings addressed by absolute position, which no hook clears (WaveNet._weights_checked): every slot a step
    reads must have been rewritten by the warm-up before it - from position 3, 8 and 0, for B, B and fewer clips"""
    _four_lives(case, device, monkeypatch, f"wavenet {case.id}")


@pytest.mark.parametrize("case", R.SRNN_ALL, ids=[c.id for c in R.SRNN_ALL])
def test_sample_rnn_plan_lives(device, monkeypatch, case):
    """tier states, counters and epoch-tagged granules that mmk_srnn_reset and the resident path's own clears put back (SampleRNN.
    _weights_checked, reset_hidden): warm-up offsets 3, 8 and 0, no warm-up step at all in life 3, resident launches behind heads of 13, 8 and
    0 steps"""
    _four_lives(case, device, monkeypatch, f"sample_rnn {case.id}")


@pytest.mark.parametrize("case", R.S2S_ALL, ids=[c.id for c in R.S2S_ALL])
def test_seq2seq_plan_lives(device, monkeypatch, case):
    """a step keeps no state between calls, but the workspace holds the states, exchange images and padded rows of Bmax clips: other frames,
    then fewer clips (1, 7, 8, 11, 15 or 63 of them), then the first ones again"""
    _four_lives(case, device, monkeypatch, f"seq2seq {case.id}")


# ---- the transformer -------------------------------------------------------------------------------------------------------------------------------------
def _tr_generate(life, net, device, look=None, every_step=False):
    """-> (history on the host, last_logits after every block or None, the plan's raw outputs of every step teacher-forced or None)"""
    B, P, rf = life.clips, life.prompt, life.rf
    prompt = life.inputs()
    data = torch.cat([prompt, torch.zeros(B, life.n, *prompt.shape[2:], dtype=prompt.dtype)], 1).to(device)
    net.before_generate((data[:, :P],), None)
    ends, t = [], P
    for nb in life.parts:
        assert net.generate_block((data,), t, nb) is True
        t += nb
        if life.classes:
            ends.append(net._plan.last_logits(B).cpu())
            if look is not None:
                look(net._plan)
    steps = None
    if every_step and life.classes:
        steps = []
        for t in range(P, P + life.n):
            net.generate_step((data[:, t - rf:t],), t=t)
            steps.append(net._plan.last_logits(B).cpu())
        steps = torch.stack(steps, 1)
    net.after_generate((data,), None)
    return data.cpu(), (torch.stack(ends, 1) if life.classes else None), steps


def _tr_within_the_envelope(life, what, hist, ends, steps, sel=None):
    if sel is not None:
        hist, ends, steps = hist[sel], (None if ends is None else ends[sel]), (None if steps is None else steps[sel])
        life = T.of_clips(life, len(sel))
    env = T.envelope(hist, life)
    failed = []
    for name, dev, at in (("last_logits after the blocks", ends, life.ends()), ("every step", steps, slice(None))) if life.classes else \
            (("every frame", hist[:, life.prompt:], slice(None)),):
        if dev is None:
            continue
        R64, E = env.R64[:, at], env.E[:, at]
        assert dev.shape == R64.shape, (what, name, dev.shape, R64.shape)
        _record(f"{what} {name}", dev, R64, E)
        tol_max, tol_rms = T.tolerance(E)
        try:
            T.check_outputs(dev, R64, tol_max, tol_rms, f"{what} {name}")
        except AssertionError as err:
            failed.append(err)
    if failed:
        raise failed[0]
    if life.classes:
        T.check_picks(hist[:, life.prompt:], env.R64, T.tolerance(env.E)[0], f"{what} picks")


def _tr_nothing_behind_the_batch(life, B, what):
    def look(plan):
        got = plan.last_logits(life.clips)
        out = torch.full((B, got.shape[1]), float("nan"), device=got.device)
        native.check(plan._lib.mmk_tr_last_logits(plan.handle, life.clips, native.ptr(out), out.stride(0), native.stream_ptr(plan.device)), "mmk_tr_last_logits")
        out = out.cpu()
        assert _same_bits([out[:life.clips]], [got.cpu()]), (what, "the caller's buffer got other rows than last_logits hands back")
        assert bool(out[life.clips:].isnan().all()), (what, f"{int((~out[life.clips:].isnan()).sum())} elements behind the batch were written")
    return look


@pytest.mark.parametrize("tag", [c.tag for c in T.CASES])
def test_transformer_plan_lives(device, tag):
    """KV rows, the step counter and a hipGraph keyed by the call's pointers and strides: four tensors of three shapes at three t0 on one plan"""
    case = T.BY_TAG[tag]
    what = f"transformer {tag}"
    net = T.build_case(case, device)
    B = case.clips
    ran, plan, packs = {}, None, None
    for life in T.lives(case):
        look = _tr_nothing_behind_the_batch(life, B, f"{what} life 3") if life.index == 3 else None
        ran[life.index] = _tr_generate(life, net, device, look, every_step=life.index in (2, 3))
        if life.index == 1:
            plan, packs = net._plan, native.pack_launch_count()
        print(f"[lives] {what} life {life.index}: {life.clips} clips, prompt {life.prompt}, {life.n} steps")
        assert net._plan is plan and net._plan_batch == B, (what, life.index, "the plan was replaced", net._plan_batch)
        assert native.pack_launch_count() == packs, (what, life.index, "the weights were packed again")
    _, two, three, _ = T.lives(case)
    failed = []
    for life in (two, three):
        try:
            _tr_within_the_envelope(life, f"{what} life {life.index}", *ran[life.index], sel=_some_clips(life.clips) if life.index == 2 else None)
        except AssertionError as err:
            failed.append(err)
    fresh = [_tr_generate(two, T.build_case(case, device), device)[:2] for _ in range(2)]
    deterministic = _same_bits([x for x in fresh[0] if x is not None], [x for x in fresh[1] if x is not None])
    print(f"[lives] {what}: two fresh plans give {'equal' if deterministic else 'OTHER'} bits in life 2")
    if tag in NOT_BIT_DETERMINISTIC.get("transformer", ()):
        for k, run in enumerate(fresh):
            _tr_within_the_envelope(two, f"{what} life 2 on fresh plan {k}", *run, None, sel=_some_clips(two.clips))
    else:
        assert deterministic, (what, "two fresh networks and plans disagree bitwise in life 2: the mode is not deterministic")
        assert _same_bits([x for x in ran[2][:2] if x is not None], [x for x in fresh[0] if x is not None]), \
            (what, "life 2 on the plan life 1 ran on differs bitwise from life 2 on a fresh plan")
        assert _same_bits([x for x in ran[4][:2] if x is not None], [x for x in ran[1][:2] if x is not None]), \
            (what, "life 4 differs bitwise from life 1: same plan, same inputs")
    if failed:
        raise failed[0]
