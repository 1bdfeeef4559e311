"""discontinuity_scores on one MI355X against a plain torch evaluation on the same device.

    python scripts/novelty_bench.py [--frames 131072] [--bins 1025,16] [--repeats 50] [--warmup 3] [--block 1024] [--out FILE]

One JSON line per (bins, half-widths): [median, min, max] ms between HIP events of `repeats` calls after `warmup` calls of
  hip          mmk.discontinuity_scores: inv_row_norm, mmk_novelty_f32, mmk_novelty_finish_f32
  hip_kernel   native.novelty alone, the norms given
  torch        normalised frames, torch.matmul block by block over the band (`block` output frames and the 2 h_max + 1 frames around
               them), a float64 summed-area table of each block's distances and four rectangle sums per quadrant of the board
and `x_read_share`: the bytes of x (frames x bins x 4) over the hip_kernel time, as a share of the 8 TB/s HBM peak - what reading x ONCE
would represent; the kernel reads it 1 + (2 h_max + 1) / 64 times, mostly from cache.  `max_diff` is the largest difference between the two
results (the torch one carries fp32 matmul and summed-area roundings of its own).
"""
import argparse
import json
import os
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import mimikit_amd as mmk  # noqa: E402
from mimikit_amd import native  # noqa: E402

HBM_PEAK = 8.0e12
HALVES = ([6], [6, 12, 24])


def torch_scores(x, halves, block):
    T = x.shape[0]
    hm = max(halves)
    n = x.norm(dim=1)
    xn = x * torch.where(n > 0, 1.0 / n, torch.zeros_like(n))[:, None]
    raw = torch.empty((len(halves), T), dtype=torch.float32, device=x.device)
    for s in range(0, T, block):
        e = min(s + block, T)
        lo, hi = s - 1 - hm, e + hm                      # the frames the boards of [s, e) touch
        clo, chi = max(lo, 0), min(hi, T)
        seg = xn[clo:chi]
        d = 1.0 - seg @ seg.T
        d.fill_diagonal_(0.0)
        d = F.pad(d, (clo - lo, hi - chi, clo - lo, hi - chi))
        S = F.pad(d.double().cumsum(0).cumsum(1), (1, 0, 1, 0))
        pr = torch.arange(s, e, device=x.device) - lo
        pc = pr - 1

        def rect(r0, r1, c0, c1):
            return S[r1, c1] - S[r0, c1] - S[r1, c0] + S[r0, c0]

        for q, h in enumerate(halves):
            up, down, left, right = (pr - h, pr), (pr + 1, pr + h + 1), (pc - h, pc), (pc + 1, pc + h + 1)
            v = rect(*up, *right) + rect(*down, *left) - rect(*up, *left) - rect(*down, *right)
            raw[q, s:e] = (v / (4.0 * h * h)).float()
    return raw - raw.min(-1, keepdim=True).values


def timed(fn, device, warmup, repeats):
    for _ in range(warmup):
        fn()
    times = []
    for _ in range(repeats):
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize(device)
        start.record()
        fn()
        stop.record()
        torch.cuda.synchronize(device)
        times.append(start.elapsed_time(stop))
    times.sort()
    return [round(times[len(times) // 2], 4), round(times[0], 4), round(times[-1], 4)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=131072)
    ap.add_argument("--bins", default="1025,16")
    ap.add_argument("--repeats", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--block", type=int, default=1024)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    device = torch.device("cuda", 0)
    torch.set_grad_enabled(False)
    lines = []
    for bins in [int(b) for b in args.bins.split(",")]:
        x = torch.rand((args.frames, bins), generator=torch.Generator().manual_seed(bins)).to(device) ** 3
        inv = native.inv_row_norm(x)
        for halves in HALVES:
            hip = timed(lambda: mmk.discontinuity_scores(x, halves), device, args.warmup, args.repeats)
            kern = timed(lambda: native.novelty(x, halves, inv), device, args.warmup, args.repeats)
            ref = timed(lambda: torch_scores(x, halves, args.block), device, args.warmup, args.repeats)
            diff = float((mmk.discontinuity_scores(x, halves) - torch_scores(x, halves, args.block)).abs().max())
            lines.append(json.dumps({"metric": "novelty", "frames": args.frames, "bins": bins, "halves": halves, "repeats": args.repeats,
                                     "unit": "ms [median, min, max]", "hip": hip, "hip_kernel": kern, "torch": ref, "torch_block": args.block,
                                     "speedup_vs_torch": round(ref[0] / hip[0], 2), "x_bytes": args.frames * bins * 4,
                                     "x_read_share": round(args.frames * bins * 4 / (kern[0] * 1e-3) / HBM_PEAK, 4), "max_diff": diff,
                                     "device": torch.cuda.get_device_name(0), "library_digest": native.lib().mmk_build_digest().decode()}))
            print(lines[-1], flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
