"""Envelop benchmark on one MI355X: 64 clips x 10 s at 22 050 Hz, n_fft 2048, hop 512.

    python scripts/envelope_bench.py [--iters 20] [--rounds 7] [--warmup 3]

One JSON line.  Every figure is the median over `rounds` of the device time of `iters` back-to-back calls (HIP events), with the spread
(max - min over the rounds, as a share of the median) beside it:
  energy_us        native.stft_energy alone (the fused epilogue: reads the samples, writes one float per frame)
  composed_us      what the library could do before it: native.stft(x, ..., "reflect", "pol")[..., 0].sum(-1) - the measure, not the code under
                   test (writes 2 floats per bin, reads half of them back)
  envelop_us       Envelop(2048, 512) end to end (length fix, energy, interpolation to the time domain, division by the maximum)
  energy_bytes / composed_bytes: the bytes each must move (samples in; frames or spectrogram out and back in), and energy_tbps
  fused_no_slower  energy_us <= composed_us beyond the two spreads
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from mimikit_amd import native  # noqa: E402
from mimikit_amd.features.functionals import Envelop  # noqa: E402


def timed(fn, iters, device):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize(device)
    start.record()
    for _ in range(iters):
        fn()
    stop.record()
    torch.cuda.synchronize(device)
    return start.elapsed_time(stop) * 1e-3 / iters


def rounds_of(fn, args, device):
    for _ in range(args.warmup):
        fn()
    t = [timed(fn, args.iters, device) for _ in range(args.rounds)]
    med = statistics.median(t)
    return med, (max(t) - min(t)) / med


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--clips", type=int, default=64)
    ap.add_argument("--seconds", type=float, default=10.0)
    args = ap.parse_args()
    device = torch.device("cuda", 0)
    torch.set_grad_enabled(False)
    n_fft, hop, sr = 2048, 512, 22050
    n = int(args.seconds * sr)
    x = (torch.rand(args.clips, n, generator=torch.Generator().manual_seed(1)) * 2 - 1).to(device)
    env = Envelop(n_fft, hop)
    xf = env.fft.stft._fix_length(x)
    frames = native.lib().mmk_stft_n_frames(xf.shape[-1], n_fft, hop, 1)
    bins = n_fft // 2 + 1
    t_energy, s_energy = rounds_of(lambda: native.stft_energy(xf, n_fft, hop, True, "reflect"), args, device)
    t_comp, s_comp = rounds_of(lambda: native.stft(xf, n_fft, hop, True, "reflect", "pol")[..., 0].sum(-1), args, device)
    t_env, s_env = rounds_of(lambda: env(x), args, device)
    a, b = native.stft_energy(xf, n_fft, hop, True, "reflect"), native.stft(xf, n_fft, hop, True, "reflect", "pol")[..., 0].sum(-1)
    energy_bytes = 4 * args.clips * (xf.shape[-1] + frames)
    composed_bytes = 4 * args.clips * (xf.shape[-1] + 2 * frames * bins + frames * bins + frames)
    print(json.dumps({
        "metric": "envelop", "clips": args.clips, "samples": n, "n_fft": n_fft, "hop": hop, "frames": int(frames), "iters": args.iters,
        "rounds": args.rounds,
        "energy_us": round(t_energy * 1e6, 1), "energy_spread": round(s_energy, 3),
        "composed_us": round(t_comp * 1e6, 1), "composed_spread": round(s_comp, 3),
        "envelop_us": round(t_env * 1e6, 1), "envelop_spread": round(s_env, 3),
        "energy_bytes": energy_bytes, "composed_bytes": composed_bytes, "energy_tbps": round(energy_bytes / t_energy / 1e12, 3),
        "max_rel_diff": float(((a - b).abs() / b).max()),
        "fused_no_slower": bool(t_energy * (1 - s_energy) <= t_comp * (1 + s_comp)),
        "device": torch.cuda.get_device_name(0)}), flush=True)


if __name__ == "__main__":
    main()
