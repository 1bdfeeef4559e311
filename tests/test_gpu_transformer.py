"""SimpleTransformer on the HIP generate path (csrc/transformer_plan.hip): golden parity with the reference's GenerateLoopV2,
the default-sized network against torch running the network's own modules on the device, sampled decode, geometry edges."""
import json

import numpy as np
import pytest
import torch

import mimikit_amd as mmk
from tests import helpers as H
from tests.f64_bounds import check_bound, check_near_miss
from tests.transformer_refs import build, f64_walk, torch_outputs, torch_outputs_f64, windows_of

pytestmark = pytest.mark.gpu

G = H.golden("transformer.npz")
CASES = json.loads(str(G["cases"]))
LOGIT_TOL = dict(rtol=1e-4, atol=2e-4)


def loop_run(net, prompt, n_steps):
    loop = mmk.GenerateLoopV2(mmk.GenerateLoopV2.Config(display_waveform=False, yield_inversed_outputs=False), net, n_steps,
                              [[np.arange(prompt.size(0)), prompt]], logger=None)
    out = list(loop.run())[0][0]
    torch.set_grad_enabled(False)
    return out


def device_logits(net, hist, t0, n):
    """teacher-forced generate_step over the windows of `hist`, the plan's raw head outputs after each: (B, n, q + 1)"""
    rows = []
    for t in range(t0, t0 + n):
        net.generate_step((hist[:, t - net.rf:t],), t=t)
        rows.append(net._plan.last_logits(hist.size(0)))
    return torch.stack(rows, 1)


def check_greedy_block(net, batch, prompt_len, n_steps, seed=0, logits_every=1):
    """free-running generate_block, then torch over the device's own history: logits within 1e-3 of the largest, argmax equal where
    the top-2 gap is clear (at most 2 % of the steps excluded)"""
    gen = torch.Generator().manual_seed(seed)
    rf = net.rf
    hist = torch.cat([torch.randint(0, 256, (batch, prompt_len), generator=gen), torch.zeros(batch, n_steps, dtype=torch.long)], 1).cuda()
    net.before_generate((hist[:, :prompt_len],), None)
    assert net.generate_block((hist,), prompt_len, n_steps) is True
    want = torch_outputs(net, windows_of(hist, prompt_len, n_steps, rf)).reshape(batch, n_steps, -1)
    scale = float(want[..., :-1].abs().max())
    ok = H.margin_ok(want.cpu(), min_gap=2e-4 * scale)
    H.excluded_fraction(ok, f"rf {rf}, {batch} clips")
    picks = hist[:, prompt_len:]
    assert bool(((want[..., :-1].argmax(-1) == picks).cpu() | ~ok).all())
    steps = list(range(0, n_steps, logits_every))
    got = torch.stack([device_logits(net, hist, prompt_len + s, 1)[:, 0] for s in steps], 1)
    err = float((got - want[:, steps]).abs().max())
    assert err <= 1e-3 * scale, f"logits off by {err:.3e} (largest logit {scale:.3e})"
    return hist


@pytest.mark.parametrize("tag", sorted(CASES))
def test_golden_parity_through_the_loop(tag):
    net_kw, io_kw, clips, prompt_len, n_steps, seed = CASES[tag]
    net = build(net_kw, io_kw, seed, float(G["gain"]))
    prompt = H.T(G[f"{tag}_prompt"]).cuda()
    out = loop_run(net, prompt, n_steps).cpu()
    want = H.T(G[f"{tag}_out"])
    if io_kw["kind"] == "mulaw":
        assert torch.equal(out, want), f"{tag}: classes differ from the reference's"
        raw = device_logits(net, want.cuda(), prompt_len, n_steps).cpu()
        torch.testing.assert_close(raw, H.T(G[f"{tag}_raw"]), **LOGIT_TOL)
    else:
        torch.testing.assert_close(out, want, **LOGIT_TOL)


def test_default_size_teacher_forced_32_and_37_clips():
    net = build({}, dict(kind="mulaw", n_mlp_layers=1, mlp_dim=128), seed=71)
    assert (net.config.model_dim, net.config.n_heads, net.config.num_layers, net.rf) == (256, 8, 8, 64)
    check_greedy_block(net, 32, 64, 128, seed=1, logits_every=4)
    check_greedy_block(net, 37, 70, 128, seed=2, logits_every=4)


def test_sampled_decode_picks_lie_in_their_cdf_interval():
    net = build(dict(model_dim=128, n_heads=4, feedforward_dim=256, num_layers=3, rf=32), dict(kind="mulaw", n_mlp_layers=1), seed=72)
    batch, p, n = 8, 40, 64
    gen = torch.Generator().manual_seed(3)
    hist = torch.cat([torch.randint(0, 256, (batch, p), generator=gen), torch.zeros(batch, n, dtype=torch.long)], 1).cuda()
    temps = torch.linspace(0.5, 1.5, batch)
    net.before_generate((hist[:, :p],), None)
    torch.manual_seed(1234)
    net.generate_block((hist,), p, n, temperature=temps)
    torch.manual_seed(1234)
    u = torch.rand((batch, n), device="cuda")
    raw = torch_outputs(net, windows_of(hist, p, n, net.rf)).reshape(batch, n, -1).cpu()
    ok, exact = H.sampled_picks_ok(raw, temps, u.cpu(), hist[:, p:].cpu())
    assert bool(ok.all()) and float(exact.float().mean()) >= 0.98
    assert len(torch.unique(hist[:, p:])) > 8          # (a sampled stream, not one class)


@pytest.mark.parametrize("tag,net_kw,batch,prompt_len,n_steps", [
    ("head_dim128", dict(model_dim=512, n_heads=4, feedforward_dim=512, num_layers=2, rf=32), 4, 40, 24),
    ("rf300", dict(model_dim=64, n_heads=4, feedforward_dim=128, num_layers=2, rf=300), 3, 310, 24),
    ("rf1", dict(model_dim=32, n_heads=4, feedforward_dim=64, num_layers=1, rf=1), 5, 3, 24),
])
def test_geometry_edges(tag, net_kw, batch, prompt_len, n_steps):
    net = build(net_kw, dict(kind="mulaw", n_mlp_layers=1), seed=73)
    check_greedy_block(net, batch, prompt_len, n_steps, seed=4)


def test_a_larger_batch_re_plans():
    net = build(dict(model_dim=64, n_heads=4, feedforward_dim=128, num_layers=2, rf=16), dict(kind="mulaw", n_mlp_layers=0), seed=74)
    check_greedy_block(net, 3, 20, 16, seed=5)
    first = net._plan
    assert net._plan_batch == 3
    check_greedy_block(net, 9, 20, 16, seed=6)
    assert net._plan is not first and net._plan_batch == 9


def test_generate_step_equals_generate_block():
    net = build(dict(model_dim=64, n_heads=8, feedforward_dim=128, num_layers=2, rf=16, with_layer_norm=True), dict(kind="mulaw", n_mlp_layers=2),
                seed=75)
    gen = torch.Generator().manual_seed(7)
    p, n = 20, 40
    a = torch.cat([torch.randint(0, 256, (4, p), generator=gen), torch.zeros(4, n, dtype=torch.long)], 1).cuda()
    b = a.clone()
    net.before_generate((a[:, :p],), None)
    net.generate_block((a,), p, n)                      # (a hipGraph of 8 steps, replayed 5 times)
    for t in range(p, p + n):
        b[:, t:t + 1] = net.generate_step((b[:, t - net.rf:t],), t=t)[0]
    assert torch.equal(a, b)
    # frames: the same for the magspec IO
    mag = build(dict(model_dim=64, n_heads=4, feedforward_dim=128, num_layers=2, rf=8), dict(kind="magspec", n_fft=64), seed=76)
    fa = torch.cat([torch.rand(2, 10, 33, generator=gen), torch.zeros(2, 20, 33)], 1).cuda()
    fb = fa.clone()
    mag.generate_block((fa,), 10, 20)
    for t in range(10, 30):
        fb[:, t:t + 1] = mag.generate_step((fb[:, t - 8:t],), t=t)[0]
    assert torch.equal(fa, fb)
    want = torch_outputs(mag, windows_of(fa, 10, 20, 8)).reshape(2, 20, 33)
    torch.testing.assert_close(fa[:, 10:], want, **LOGIT_TOL)


def test_load_state_dict_between_generations_rebinds():
    kw = dict(model_dim=64, n_heads=4, feedforward_dim=128, num_layers=2, rf=16)
    net = build(kw, dict(kind="mulaw", n_mlp_layers=1), seed=77)
    other = build(kw, dict(kind="mulaw", n_mlp_layers=1), seed=78)
    gen = torch.Generator().manual_seed(8)
    prompt = torch.randint(0, 256, (3, 20), generator=gen).cuda()
    first = loop_run(net, prompt, 16)
    net.load_state_dict(other.state_dict())
    second = loop_run(net, prompt, 16)
    assert not torch.equal(first, second)
    assert torch.equal(second, loop_run(other, prompt, 16))


def test_loop_from_config_runs_end_to_end():
    net = build(dict(model_dim=64, n_heads=4, feedforward_dim=128, num_layers=2, rf=16), dict(kind="mulaw", n_mlp_layers=1), seed=79)
    gen = torch.Generator().manual_seed(9)
    signal = (torch.rand(16000, generator=gen) * 2 - 1).numpy().astype(np.float32)
    cfg = mmk.GenerateLoopV2.Config(output_duration_sec=0.002, prompts_length_sec=0.002, prompts_position_sec=(0.25, 0.5),
                                    batch_size=2, display_waveform=False, yield_inversed_outputs=False)
    loop = mmk.GenerateLoopV2.from_config(cfg, {"signal": signal}, net, logger=None)
    outs = list(loop.run())
    torch.set_grad_enabled(False)
    assert len(outs) == 1 and outs[0][0].shape == (2, 64)
    out = outs[0][0]
    # the same prompts through generate_block directly
    prompt = mmk.MuLawCompress()(torch.from_numpy(np.stack([signal[4000:4032], signal[8000:8032]])).cuda())
    assert torch.equal(out[:, :32], prompt)
    hist = torch.cat([prompt, torch.zeros(2, 32, dtype=torch.long, device="cuda")], 1)
    net.generate_block((hist,), 32, 32)
    assert torch.equal(out, hist)


# ---------------------------------------------------------------------------------------------------------------- float64 step check
# The plan's raw head outputs against the network's own modules run in float64 on the CPU, within a bound derived from the kernels'
# bounds (tests/f64_bounds.py, the bounds tests/test_gpu_kernels_f64.py holds every kernel to): tests/transformer_refs.py has the walk that
# carries the bound (f64_walk) and says how.  The walk's values must be the network's own float64 outputs (checked first), so the bound is
# about the network that ran.  (The bound is 18 to 100 times four times the reference's own fp32 error: test_gpu_transformer_f64.py holds the same steps,
# and the graph path, to that envelope.)
@pytest.mark.parametrize("tag,net_kw,io_kw,batch", [
    ("head_dim12", dict(model_dim=48, n_heads=4, feedforward_dim=96, num_layers=3, rf=16), dict(kind="mulaw", n_mlp_layers=2), 3),
    # rf 65: the window crosses the 64-row workgroup and the 64-key tile; B rf = 130 >= 128 rows: the plan's GEMMs run on the tiled
    # kernel, split along K where the grid is small (the plan hands it its partial buffer)
    ("layer_norm_rf65", dict(model_dim=48, n_heads=4, feedforward_dim=96, num_layers=2, rf=65, with_layer_norm=True),
     dict(kind="mulaw", n_mlp_layers=1), 2),
    ("magspec_rf65", dict(model_dim=64, n_heads=4, feedforward_dim=128, num_layers=2, rf=65), dict(kind="magspec", n_fft=64), 2),
])
def test_teacher_forced_steps_within_a_float64_bound(tag, net_kw, io_kw, batch):
    """the plan's raw head outputs (magspec: its frames) after teacher-forced generate_steps, element by element against the network's
    own modules in float64 on the CPU, within the bound f64_walk derives; that bound must sit well below the 1e-3 x max|output| of the
    tests above (a tenth of it), and a causal mask that leaks one key must break it"""
    net = build(net_kw, io_kw, seed=90)
    net64 = build(net_kw, io_kw, seed=90, device="cpu").double()
    net64.load_state_dict(net.state_dict())
    rf, n = net.rf, 4
    t0 = rf + 3
    gen = torch.Generator().manual_seed(12)
    if io_kw["kind"] == "mulaw":
        hist = torch.randint(0, 256, (batch, t0 + n), generator=gen).cuda()
        net.before_generate((hist[:, :t0],), None)
        got = device_logits(net, hist, t0, n).cpu()
        windows = windows_of(hist.cpu(), t0, n, rf)
    else:
        hist = torch.rand(batch, t0 + n, io_kw["n_fft"] // 2 + 1, generator=gen).cuda()
        got = torch.stack([net.generate_step((hist[:, t - rf:t],), t=t)[0].reshape(batch, -1) for t in range(t0, t0 + n)], 1).cpu()
        windows = windows_of(hist.cpu(), t0, n, rf).double()
    want = torch_outputs_f64(net64, windows)
    walk, bound = f64_walk(net64, windows)
    assert float((walk - want).abs().max()) <= 1e-12 * float(want.abs().max()), f"{tag}: the walk is not the network"
    want, bound = want.reshape(batch, n, -1), bound.reshape(batch, n, -1)
    scale = float(want.abs().max())
    assert float(bound.max()) <= 1e-4 * scale, f"{tag}: derived bound {float(bound.max()):.3e} is not well below 1e-3 x {scale:.3e}"
    check_bound(got, want, bound, f"{tag}: plan outputs")
    leak, _ = f64_walk(net64, windows, shift=1)
    check_near_miss(leak.reshape(batch, n, -1), want, bound, f"{tag}: a causal mask leaking one key")
