"""SimpleTransformer step outputs on the device against the float64 walk, inside the envelope of tests/transformer_refs.py (the regime
test_gpu_networks_f64.py holds WaveNet, SampleRNN and Seq2Seq to): the plan branches no other test reaches (transformer_refs.CASES says which
case is there for which), the graph path, every pick, no excused share.

Class cases: a random prompt of rf + 3, greedy, generate_block in consecutive calls of 19, 16 and 5 steps on the same tensor (two replays of the
8-step hipGraph plus three plain steps; another t0, so the graph is captured again; fewer than 2 x 8 steps, so no graph; the two large networks:
16 and 3).  Then, against the envelope built on the device's own history: last_logits after every block (check_outputs against that step's R64
row), the logits of EVERY step from teacher-forced generate_step over the same windows (check_outputs over all of them), every pick of every
step (check_picks) and every defect that applies to the case on the same rows (check_near_miss).
Frame cases: every generated frame of a 19-step block, the reference of each step run on the device's own preceding frames.
Graph cache hit: a second generate_block with the same tensor, t0 and n replays the stored graph on a history that has changed.
Sampled block: per-clip temperatures on the tiled head, every pick inside its CDF interval of R32 (the conditions of
test_gpu_transformer.py::test_sampled_decode_picks_lie_in_their_cdf_interval, which test_transformer_refs.py shows the references alone meet).

First run on an MI355X, per case: max|dev - R64| / max(E) and rms(dev - R64) / rms(E) over the compared elements (the margin allows 4).  Records,
not tolerances - the tolerance is recomputed from the reference on every run:

  case             compared                      outputs  scale   max ratio  rms ratio    max(E)     rms(E)
  one_layer_rf9    last_logits after the blocks     2313  5.16         0.88       0.81  2.101e-06  6.409e-07
  one_layer_rf9    every step                      30840  5.89         0.88       0.78  2.893e-06  6.831e-07
  clips130_rf2     last_logits after the blocks   100230  4.37         0.69       0.70  2.220e-06  5.674e-07
  clips130_rf2     every step                    1336400  5.17         0.69       0.68  3.555e-06  5.868e-07
  ff24_rf33        last_logits after the blocks     3084  4.65         1.07       0.82  1.562e-06  4.825e-07
  ff24_rf33        every step                      41120  5.19         1.01       0.80  2.641e-06  5.485e-07
  ff8_rf33         last_logits after the blocks     3084  4.55         1.02       0.80  2.962e-06  7.648e-07
  ff8_rf33         every step                      41120  4.87         0.96       0.79  3.536e-06  7.562e-07
  frames130_rf2    every frame                     41990  3.64         0.98       0.81  1.673e-06  3.931e-07
  layer_norm_rf65  last_logits after the blocks     1542  4.92         0.94       0.69  2.508e-06  7.753e-07
  layer_norm_rf65  every step                      20560  5.28         0.79       0.74  3.512e-06  7.800e-07
  head_dim128      last_logits after the blocks     1028  4.64         0.62       0.48  4.210e-06  1.104e-06
  head_dim128      every step                       9766  4.96         0.62       0.52  4.210e-06  1.132e-06
  default          last_logits after the blocks     1028  4.26         0.78       0.56  2.869e-06  1.076e-06
  default          every step                       9766  4.29         0.57       0.52  3.917e-06  1.097e-06
  one_layer_rf9    last_logits, replayed graph       771  4.89         0.69       0.62  2.128e-06  6.758e-07
  clips130_rf2     last_logits, replayed graph     33410  4.37         0.69       0.76  2.220e-06  5.313e-07

The device lies inside the reference's own fp32 error, or at it, in every case (max ratios 0.57 .. 1.07, rms 0.48 .. 0.82): every case could be
planned, none left the envelope, no finding on the device and no further reference-side run in E.  Sampled block: 2470 of 2470 picks inside
their interval.  Measured once beside the tests, the same cases with the recipe's own weights (gain 1.5, LayerNorm weights around zero, which
transformer_refs.py explains it does not use): max ratios 0.31 .. 1.03, rms 0.48 .. 0.87, every pick right - and every pick the same class.
"""
import pytest
import torch

from tests import helpers as H
from tests import transformer_refs as R

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)
TAGS = [c.tag for c in R.CASES]


def _blank(case, prompt, n, device):
    return torch.cat([prompt, torch.zeros(case.clips, n, *prompt.shape[2:], dtype=prompt.dtype)], 1).to(device)


def _record(what, dev, R64, E):
    r_max, r_rms = R.ratios(dev, R64, E)
    print(f"[f64] transformer {what}: {dev.numel()} outputs of scale {float(R64.abs().max()):.3g}; max|dev - R64| / max(E) = {r_max:.2f}, "
          f"rms(dev - R64) / rms(E) = {r_rms:.2f} (the margin allows {R.FACTOR:g}); max(E) {float(E.max()):.3e}, rms(E) {R.rms(E):.3e}")


def _held(what, dev, R64, E):
    """check_outputs with the tolerance of exactly these elements; the figures are printed first"""
    assert dev.shape == R64.shape, (what, dev.shape, R64.shape)
    _record(what, dev, R64, E)
    tol_max, tol_rms = R.tolerance(E)
    R.check_outputs(dev, R64, tol_max, tol_rms, what)
    return tol_max


@pytest.mark.parametrize("tag", TAGS)
def test_transformer_steps_within_the_float64_envelope(device, tag):
    case = R.BY_TAG[tag]
    net = R.build_case(case, device)
    B, P, n, rf = case.clips, case.prompt, case.n, case.rf
    data = _blank(case, case.inputs(), n, device)
    net.before_generate((data[:, :P],), None)
    ends, t = [], P
    for nb in case.parts:
        assert net.generate_block((data,), t, nb) is True
        t += nb
        if case.classes:
            ends.append(net._plan.last_logits(B).cpu())
    hist = data.cpu()
    env = R.envelope(hist, case)
    if case.classes:
        rows = case.ends()
        failed = []
        try:
            _held(f"{tag} last_logits after the blocks", torch.stack(ends, 1), env.R64[:, rows], env.E[:, rows])
        except AssertionError as err:      # (the figures of every step are printed before the first failure is raised)
            failed.append(err)
        # the same windows teacher-forced, step by step (no graph): the plan's raw head outputs of EVERY step
        steps = []
        for t in range(P, P + n):
            net.generate_step((data[:, t - rf:t],), t=t)
            steps.append(net._plan.last_logits(B).cpu())
        tol_max = _held(f"{tag} every step", torch.stack(steps, 1), env.R64, env.E)
        if failed:
            raise failed[0]
        R.check_picks(hist[:, P:], env.R64, tol_max, f"{tag} picks")
    else:
        tol_max = _held(f"{tag} every frame", hist[:, P:], env.R64, env.E)
    letters = ""
    for name, out in R.defects(case, hist, env.R64):
        R.check_near_miss(out, env.R64, tol_max, f"{tag} {name}")
        letters += name[1]
    assert letters == R.applicable(case)


@pytest.mark.parametrize("tag", R.CACHE_HIT_CASES)
def test_a_cached_graph_replays_on_a_changed_history(device, tag):
    """run_steps keys the stored graph by the call's pointers and strides: the second call below has the first one's key and replays its graph;
    the window is read through the device's step counter, so the new prompt must decide the new picks"""
    case = R.BY_TAG[tag]
    net = R.build_case(case, device)
    P, n = case.prompt, case.parts[0]
    assert n >= 16                                 # (a graph: at least two replays of 8 steps)
    data = _blank(case, case.inputs(), n, device)
    net.before_generate((data[:, :P],), None)
    assert net.generate_block((data,), P, n) is True
    first = data[:, P:].cpu()
    data[:, :P] = case.inputs(seed=1000 + case.seed).to(device)
    data[:, P:] = 0
    assert net.generate_block((data,), P, n) is True
    hist = data.cpu()
    env = R.envelope(hist, case)
    tol_max, _ = R.tolerance(env.E)
    R.check_picks(hist[:, P:], env.R64, tol_max, f"{tag} picks of the replayed graph")
    tol_last = _held(f"{tag} last_logits of the replayed graph", net._plan.last_logits(case.clips).cpu(), env.R64[:, -1], env.E[:, -1])
    assert tol_last > 0
    assert not torch.equal(first, hist[:, P:]), f"{tag}: the second call produced the first history's picks"


def test_sampled_block_on_the_tiled_head(device):
    case = R.BY_TAG[R.SAMPLED_CASE]
    net = R.build_case(case, device)
    B, P, n = case.clips, case.prompt, case.parts[0]
    data = _blank(case, case.inputs(), n, device)
    temps = torch.linspace(0.5, 1.5, B)
    net.before_generate((data[:, :P],), None)
    torch.manual_seed(1234)
    net.generate_block((data,), P, n, temperature=temps)
    torch.manual_seed(1234)
    u = torch.rand((B, n), device=device)
    hist = data.cpu()
    ok, exact = H.sampled_picks_ok(R.reference32(case, hist), temps, u.cpu(), hist[:, P:])
    print(f"[f64] transformer {case.tag} sampled: {float(exact.float().mean()) * 100:.2f} % of {exact.numel()} picks inside their interval")
    assert bool(ok.all()) and float(exact.float().mean()) >= 0.98
    assert len(torch.unique(hist[:, P:])) > 8          # (a sampled stream, not one class)
