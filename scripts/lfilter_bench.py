"""Signal-conditioning benchmark on one MI355X: the first-order filter section and the row normalisation
(csrc/filters.hip) next to MuLawExpand, the streaming kernel they sit beside at the loop's tail.

    python scripts/lfilter_bench.py [--clips 64] [--seconds 10] [--sr 22050] [--iters 200] [--warmup 20] [--only NAME]

One JSON line per pass over (clips, seconds * sr) fp32 rows:
  us               device time of one call (HIP events around `iters` calls on one stream, after `warmup` calls)
  tbps_algorithmic bytes the algorithm needs (read the input once, write the output once) / time
  tbps_moved       bytes the launches move (the two-pass forms read the input twice) / time
--only runs one pass (deemphasis, emphasis, normalize, mulaw_expand) - for a counter collection that wants one kernel family per run.
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import mimikit_amd as mmk  # noqa: E402


def timed(fn, iters, device):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize(device)
    start.record()
    for _ in range(iters):
        fn()
    stop.record()
    torch.cuda.synchronize(device)
    return start.elapsed_time(stop) * 1e-3 / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clips", type=int, default=64)
    ap.add_argument("--seconds", type=float, default=10.0)
    ap.add_argument("--sr", type=int, default=22050)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--only", default=None)
    args = ap.parse_args()
    device = torch.device("cuda", 0)
    torch.set_grad_enabled(False)
    n = int(args.seconds * args.sr)
    gen = torch.Generator().manual_seed(n)
    x = (torch.rand(args.clips, n, generator=gen) * 2 - 1).to(device)
    codes = torch.randint(0, 256, (args.clips, n), generator=gen).to(device)
    samples = args.clips * n
    # name -> (call, algorithmic bytes per sample, bytes moved per sample)
    passes = {
        "deemphasis": (lambda: mmk.Deemphasis(0.97)(x), 8, 12),
        "emphasis": (lambda: mmk.Emphasis(0.97)(x), 8, 8),
        "normalize": (lambda: mmk.Normalize()(x), 8, 12),
        "mulaw_expand": (lambda: mmk.MuLawExpand(256)(codes), 12, 12),
    }
    for name, (fn, algo, moved) in passes.items():
        if args.only not in (None, name):
            continue
        for _ in range(args.warmup):
            fn()
        sec = timed(fn, args.iters, device)
        print(json.dumps({"metric": "signal_conditioning", "pass": name, "clips": args.clips, "samples_per_clip": n, "iters": args.iters,
                          "us": round(sec * 1e6, 2), "tbps_algorithmic": round(samples * algo / sec / 1e12, 3),
                          "tbps_moved": round(samples * moved / sec / 1e12, 3), "device": torch.cuda.get_device_name(0)}), flush=True)


if __name__ == "__main__":
    main()
