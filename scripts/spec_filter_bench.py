"""AutoConvolve and F0Filter on one MI355X: each launch beside a device copy of the same bytes and beside the
eager-torch composition of the same formula, which is what a user would otherwise run.

    python scripts/spec_filter_bench.py [--clips 64] [--seconds 10] [--n-fft 2048 1024] [--window 3] [--overtone 4] [--undertone 4]
                                        [--repeats 15] [--warmup 3]

Per n_fft: `clips` magnitude spectrograms of `seconds` s at 22050 Hz, hop n_fft / 4 (1 + samples // hop frames of n_fft / 2 + 1 bins),
|N(0, 1)| times a per-frame scale.  One JSON line per n_fft, appended to profiles/spec_filter_bench.jsonl and printed; every time is
[median, min, max] ms over `repeats` calls (HIP events around the call, after `warmup` untimed calls):
  auto_convolve / f0_filter   native.auto_convolve(s, window) / native.f0_filter(s, overtone, undertone): the launch (and the allocation
                              of its output); f0_filter_max is the same at 16 overtones and 16 undertones
  auto_convolve_torch / f0_filter_torch
                              the same formula in eager torch, float64 as the reference computes it: shifted slices, prod, log, sum,
                              divide (AutoConvolve); index_select gathers per harmonic, the lerp, clamp, sum, divide (F0Filter).  Its result
                              rounded to float32 must agree with the launch's (`*_max_ulp`)
  copy                        a torch copy of the spectrogram: one read plus one write, the floor of either filter
*_over_copy = the median over the copy's median; *_gbps = 8 bytes per element over the median.
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from mimikit_amd import native  # noqa: E402

SR = 22050


def timed_ms(fn, device):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize(device)
    start.record()
    fn()
    stop.record()
    torch.cuda.synchronize(device)
    return start.elapsed_time(stop)


def stats_ms(fn, device, warmup, repeats):
    for _ in range(warmup):
        fn()
    times = [timed_ms(fn, device) for _ in range(repeats)]
    return [round(statistics.median(times), 4), round(min(times), 4), round(max(times), 4)]


def torch_auto_convolve(s, k):
    """(B, T, F) float32 -> float64, the reference's formula on shifted slices of a padded copy"""
    z = s.double()
    frames = z.shape[1]
    padded = torch.cat([torch.ones_like(z[:, :k // 2]), z, torch.ones_like(z[:, :k - 1 - k // 2])], dim=1)
    p = padded[:, 0:frames]
    for i in range(1, k):
        p = p * padded[:, i:i + frames]
    w = torch.log(1 + p)
    w = w / (w.sum(dim=2, keepdim=True) + 1e-8)
    return w * z


def torch_f0_filter(s, n_overtone, n_undertone):
    """(B, T, F) float32 -> float64, soft and normalised: gathers per harmonic"""
    z = s.double()
    bins = z.shape[2]
    b = torch.arange(bins, device=s.device)
    y = torch.zeros_like(z)
    for h in range(1, n_overtone):
        p = h * b
        ok = p <= bins - 1
        y[..., ok] += z.index_select(2, p[ok])
    for x in range(2, n_undertone):
        lo = torch.div(b, x, rounding_mode="floor")
        up = (lo + 1).clamp(max=bins - 1)
        a = z.index_select(2, lo)
        y -= a + (z.index_select(2, up) - a) * ((b - lo * x).double() / x)
    y = y.clamp(min=0)
    y = y / (y.sum(dim=2, keepdim=True) + 1e-8)
    return z * y


def max_ulp(got, want64):
    want = want64.float()
    return int((got.view(torch.int32).long() - want.view(torch.int32).long()).abs().max())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clips", type=int, default=64)
    ap.add_argument("--seconds", type=float, default=10.0)
    ap.add_argument("--n-fft", type=int, nargs="+", default=[2048, 1024])
    ap.add_argument("--window", type=int, default=3)
    ap.add_argument("--overtone", type=int, default=4)
    ap.add_argument("--undertone", type=int, default=4)
    ap.add_argument("--repeats", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "spec_filter_bench.jsonl"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("spec_filter_bench needs the MI355X: there is no CPU path to time")
    device = torch.device("cuda", 0)
    torch.set_grad_enabled(False)
    for n_fft in args.n_fft:
        frames, bins = 1 + int(args.seconds * SR) // (n_fft // 4), n_fft // 2 + 1
        g = torch.Generator().manual_seed(n_fft)
        s = (torch.randn((args.clips, frames, bins), generator=g).abs() * (0.01 + 2.99 * torch.rand((args.clips, frames, 1), generator=g))).to(device)
        k, n_over, n_under = args.window, args.overtone, args.undertone
        line = {"metric": "spec_filter", "clips": args.clips, "frames": frames, "bins": bins, "n_fft": n_fft, "window": k, "n_overtone": n_over,
                "n_undertone": n_under, "repeats": args.repeats, "unit": "ms [median, min, max]"}
        line["auto_convolve_max_ulp"] = max_ulp(native.auto_convolve(s, k), torch_auto_convolve(s, k))
        line["f0_filter_max_ulp"] = max_ulp(native.f0_filter(s, n_over, n_under), torch_f0_filter(s, n_over, n_under))
        line["auto_convolve"] = stats_ms(lambda: native.auto_convolve(s, k), device, args.warmup, args.repeats)
        line["f0_filter"] = stats_ms(lambda: native.f0_filter(s, n_over, n_under), device, args.warmup, args.repeats)
        line["f0_filter_max"] = stats_ms(lambda: native.f0_filter(s, native.F0_FILTER_MAX_OVERTONE, native.F0_FILTER_MAX_UNDERTONE), device, args.warmup, args.repeats)
        line["auto_convolve_torch"] = stats_ms(lambda: torch_auto_convolve(s, k), device, args.warmup, args.repeats)
        line["f0_filter_torch"] = stats_ms(lambda: torch_f0_filter(s, n_over, n_under), device, args.warmup, args.repeats)
        dst = torch.empty_like(s)
        line["copy"] = stats_ms(lambda: dst.copy_(s), device, args.warmup, args.repeats)
        moved = 8.0 * s.numel()
        for name in ("auto_convolve", "f0_filter", "f0_filter_max"):
            line[f"{name}_over_copy"] = round(line[name][0] / line["copy"][0], 2)
            line[f"{name}_gbps"] = round(moved / (line[name][0] * 1e-3) / 1e9, 1)
        line.update({"copy_gbps": round(moved / (line["copy"][0] * 1e-3) / 1e9, 1),
                     "auto_convolve_torch_over_launch": round(line["auto_convolve_torch"][0] / line["auto_convolve"][0], 1),
                     "f0_filter_torch_over_launch": round(line["f0_filter_torch"][0] / line["f0_filter"][0], 1),
                     "device": torch.cuda.get_device_name(0), "library_digest": native.lib().mmk_build_digest().decode(), "date": time.strftime("%Y-%m-%d")})
        text = json.dumps(line)
        print(text, flush=True)
        with open(args.out, "a") as fh:
            fh.write(text + "\n")
        del s, dst


if __name__ == "__main__":
    main()
