"""HPSS times on one MI355X.

    python scripts/hpss_bench.py [--shapes 100000x1025,8x2586x513] [--windows 17,31,63] [--repeats 9] [--warmup 3] [--scipy]

Seeded uniform magnitudes, (frames, bins) or (batch, frames, bins).  One JSON line per shape; per window w in `windows` (both axes):
  hpss_ms["w"]["one"]      the median over `repeats` calls of native.hpss asking for the harmonic output alone (HIP events around the call,
                           after `warmup` untimed calls)
  hpss_ms["w"]["both"]     the same asking for harmonic and percussive
  bytes_one, bytes_both    what the call must move: the spectrogram read once and each requested output written once
  copy_gbps                the rate of a torch copy of a tensor of the spectrogram's size in the same run (bytes read + bytes written / time)
  copy_fraction["w"][...]  (bytes / hpss_ms) / copy_gbps: 1 would be a call that moves its bytes as fast as a copy does
  scipy_s (with --scipy)   the host's two scipy.ndimage.median_filter calls at window 31 on the same frames (the masks are not timed):
                           context, not a baseline
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

from mimikit_amd import build, native  # noqa: E402


def timed_ms(fn, device):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize(device)
    start.record()
    fn()
    stop.record()
    torch.cuda.synchronize(device)
    return start.elapsed_time(stop)


def median_ms(fn, device, warmup, repeats):
    for _ in range(warmup):
        fn()
    times = [timed_ms(fn, device) for _ in range(repeats)]
    return statistics.median(times), min(times), max(times)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="100000x1025,8x2586x513")
    ap.add_argument("--windows", default="17,31,63")
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--scipy", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("hpss_bench needs the MI355X: there is no CPU path to time")
    device = torch.device("cuda", 0)
    torch.set_grad_enabled(False)
    windows = [int(w) for w in args.windows.split(",")]
    for shape in args.shapes.split(","):
        dims = tuple(int(v) for v in shape.split("x"))
        g = torch.Generator(device="cpu").manual_seed(736 + dims[-1])
        s = torch.rand(dims, generator=g).to(device)
        n_bytes = 4 * s.numel()
        dst = torch.empty_like(s)
        copy_ms, _, _ = median_ms(lambda: dst.copy_(s), device, args.warmup, args.repeats)
        copy_gbps = 2 * n_bytes / (copy_ms * 1e-3) / 1e9
        del dst
        line = {"metric": "hpss", "shape": list(dims), "repeats": args.repeats, "bytes_one": 2 * n_bytes, "bytes_both": 3 * n_bytes,
                "copy_ms": round(copy_ms, 3), "copy_gbps": round(copy_gbps, 1), "hpss_ms": {}, "hpss_ms_min_max": {}, "copy_fraction": {}}
        for w in windows:
            one = median_ms(lambda: native.hpss(s, w, percussive=False), device, args.warmup, args.repeats)
            both = median_ms(lambda: native.hpss(s, w), device, args.warmup, args.repeats)
            line["hpss_ms"][str(w)] = {"one": round(one[0], 3), "both": round(both[0], 3)}
            line["hpss_ms_min_max"][str(w)] = {"one": [round(one[1], 3), round(one[2], 3)], "both": [round(both[1], 3), round(both[2], 3)]}
            line["copy_fraction"][str(w)] = {"one": round(2 * n_bytes / (one[0] * 1e-3) / 1e9 / copy_gbps, 4),
                                             "both": round(3 * n_bytes / (both[0] * 1e-3) / 1e9 / copy_gbps, 4)}
        line.update({"device": torch.cuda.get_device_name(0), "library_digest": build.library_digest()})
        if args.scipy:
            from scipy.ndimage import median_filter
            host = s.cpu().numpy().reshape(-1, dims[-2], dims[-1])
            t0 = time.perf_counter()
            for clip in host:
                median_filter(clip, size=(31, 1), mode="reflect")
                median_filter(clip, size=(1, 31), mode="reflect")
            line["scipy_s"] = round(time.perf_counter() - t0, 3)
        print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
