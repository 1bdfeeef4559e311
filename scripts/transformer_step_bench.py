"""SimpleTransformer generate-step benchmark on one MI355X.

    python scripts/transformer_step_bench.py [--clips 8,32,128] [--steps 2048] [--warmup 64] [--eager-steps 32]

The default network (D 256, 8 heads, FF 1024, 8 layers, rf 64, mu-law embedding in, MLP head out) with the deterministic recipe
weights.  One JSON line per clip count:
  us_per_step      device time of one step of a `steps`-long generate_block (HIP events), after a `warmup`-step block
  samples_per_s    clips x steps per second
  tflops           FLOPs of the reference's arithmetic per step (flops_per_clip_step below) / step time; peak_fraction of 157.3 TFLOP/s
  eager_us_per_step  the same network stepped by torch eager on the same device: the reference's own forward over the rf window
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import mimikit_amd as mmk  # noqa: E402
from oracle.weights import recipe_state_dict  # noqa: E402

FP32_MATRIX_PEAK = 157.3e12


def flops_per_clip_step(D, FF, L, rf, mlp_hidden, mlp_n_hidden, n_out):
    """(L - 1) full layers + the last layer's keys / values for all rows and the rest for one query + the MLP head"""
    full = 2 * rf * (8 * D * D + 2 * D * FF) + 4 * rf * (rf + 1) * D
    last = 2 * rf * 4 * D * D + 2 * (4 * D * D + 2 * D * FF) + 8 * rf * D
    head = 2 * (D * mlp_hidden + mlp_n_hidden * mlp_hidden * mlp_hidden + mlp_hidden * n_out)
    return (L - 1) * full + last + head


def make_net(device):
    io = mmk.IOSpec.mulaw_io(mmk.IOSpec.MuLawIOConfig(input_module_type="embedding"))
    net = mmk.SimpleTransformer.from_config(mmk.SimpleTransformer.Config(io_spec=io)).eval()
    sd = net.state_dict()
    shapes = {k: tuple(v.shape) for k, v in sd.items() if torch.is_floating_point(v) and v.dim() > 0 and k != "pe.pe"}
    with torch.no_grad():
        for k, v in recipe_state_dict(shapes, 71, 1.5).items():
            sd[k].copy_(v)
    return net.to(device)


def timed(fn, device):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize(device)
    start.record()
    fn()
    stop.record()
    torch.cuda.synchronize(device)
    return start.elapsed_time(stop) * 1e-3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clips", default="8,32,128")
    ap.add_argument("--steps", type=int, default=2048)
    ap.add_argument("--warmup", type=int, default=64)
    ap.add_argument("--eager-steps", type=int, default=32)
    args = ap.parse_args()
    device = torch.device("cuda", 0)
    torch.set_grad_enabled(False)
    net = make_net(device)
    cfg = net.config
    mlp = net.output_modules[0].estimator[0]
    flops = flops_per_clip_step(cfg.model_dim, cfg.feedforward_dim, cfg.num_layers, cfg.rf, mlp.hidden_dim, mlp.n_hidden_layers, mlp.out_dim)
    rf = net.rf
    for clips in [int(c) for c in args.clips.split(",")]:
        gen = torch.Generator().manual_seed(clips)
        total = rf + args.warmup + args.steps
        hist = torch.zeros(clips, total, dtype=torch.long)
        hist[:, :rf] = torch.randint(0, 256, (clips, rf), generator=gen)
        hist = hist.to(device)
        net.before_generate((hist[:, :rf],), None)
        net.generate_block((hist,), rf, args.warmup)
        sec = timed(lambda: net.generate_block((hist,), rf + args.warmup, args.steps), device)
        step = sec / args.steps
        # torch eager: the reference's forward (transformers.py:159-178) over the window, one step at a time
        eh = hist[:, :rf + args.eager_steps + 4].clone()

        def eager(t_from, n):
            for t in range(t_from, t_from + n):
                eh[:, t:t + 1] = net._forward_autograd((eh[:, t - rf:t],))[0]

        eager(rf, 4)
        esec = timed(lambda: eager(rf + 4, args.eager_steps), device)
        estep = esec / args.eager_steps
        tflops = flops * clips / step / 1e12
        print(json.dumps({"metric": "simple_transformer_step", "clips": clips, "steps": args.steps, "us_per_step": round(step * 1e6, 2),
                          "samples_per_s": round(clips / step, 1), "gflop_per_clip_step": round(flops / 1e9, 4),
                          "tflops": round(tflops, 2), "peak_fraction": round(tflops * 1e12 / FP32_MATRIX_PEAK, 4),
                          "eager_us_per_step": round(estep * 1e6, 1), "speedup_vs_eager": round(estep / step, 2),
                          "device": torch.cuda.get_device_name(0)}), flush=True)


if __name__ == "__main__":
    main()
