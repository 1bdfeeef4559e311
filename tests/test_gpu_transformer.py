"""SimpleTransformer on the HIP generate path (csrc/transformer_plan.hip): golden parity with the reference's GenerateLoopV2,
the default-sized network against torch running the network's own modules on the device, sampled decode, geometry edges."""
import json

import numpy as np
import pytest
import torch

import mimikit_amd as mmk
from oracle.weights import recipe_state_dict
from tests import helpers as H

pytestmark = pytest.mark.gpu

G = H.golden("transformer.npz")
CASES = json.loads(str(G["cases"]))
LOGIT_TOL = dict(rtol=1e-4, atol=2e-4)


def build(net_kw, io_kw, seed, gain=1.5, device="cuda"):
    if io_kw["kind"] == "mulaw":
        io = mmk.IOSpec.mulaw_io(mmk.IOSpec.MuLawIOConfig(input_module_type="embedding", mlp_dim=io_kw.get("mlp_dim", 32),
                                                          n_mlp_layers=io_kw["n_mlp_layers"]))
    else:
        io = mmk.IOSpec.magspec_io(mmk.IOSpec.MagSpecIOConfig(n_fft=io_kw["n_fft"], hop_length=io_kw["n_fft"] // 4))
    net = mmk.SimpleTransformer.from_config(mmk.SimpleTransformer.Config(io_spec=io, **net_kw)).eval()
    fill(net, seed, gain)
    return net.to(device)


def fill(net, seed, gain=1.5):
    """tests/golden/make_golden_transformer.py: the recipe for every parameter, the positional-encoding table as the network made it"""
    sd = net.state_dict()
    shapes = {k: tuple(v.shape) for k, v in sd.items() if torch.is_floating_point(v) and v.dim() > 0 and k != "pe.pe"}
    with torch.no_grad():
        for k, v in recipe_state_dict(shapes, seed, gain).items():
            sd[k].copy_(v.to(sd[k].device))


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


def windows_of(hist, t0, n, rf):
    """(B, T[, bins]) -> the (B n, rf[, bins]) windows ending before t0 .. t0 + n - 1"""
    w = hist.unfold(1, rf, 1)[:, t0 - rf:t0 - rf + n]          # (B, n, [bins,] rf)
    w = w.movedim(-1, 2) if hist.dim() == 3 else w
    return w.reshape(-1, rf, *hist.shape[2:]).contiguous()


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
