"""NMF stage times on one MI355X.

    python scripts/nmf_bench.py [--shapes 100000x1025,100000x128] [--components 16] [--repeats 7] [--warmup 2] [--max-iter 200] [--sklearn]

Seeded non-negative rank-40-plus-noise frames, made on the device.  One JSON line per shape:
  start_ms, w_half_ms, h_half_ms, iteration_ms   the median over `repeats` runs of each stage's device time (HIP events around the stage,
                                                 after `warmup` untimed runs); an iteration is a W half and an H half from the same state
  fit_ms, n_iter                                 whole NMF()(x) calls, timed the same way, and their iteration count
  two_reads_ms                                   two streaming reads of X (2 N D 4 bytes: torch's row sums of x, twice): an iteration must
                                                 read X twice, so this is its floor in this run
  iteration_over_floor                           iteration_ms / two_reads_ms
  dgemm_ms                                       torch's float64 x @ ht on the same shape (x converted beforehand, untimed)
  sklearn_s (with --sklearn)                     the host's NMF.fit_transform on the same frames: context, not a baseline
"""
import argparse
import json
import os
import statistics
import sys
import time
import warnings

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import mimikit_amd as mmk  # noqa: E402
from mimikit_amd import native  # noqa: E402


def frames(n, d, rank, device):
    g = torch.Generator(device="cpu").manual_seed(2000 + d)
    act = torch.rand(n, rank, generator=g) ** 2 * (1.15 ** -torch.arange(rank, dtype=torch.float32))
    temp = torch.rand(rank, d, generator=g) * (torch.rand(rank, d, generator=g) < 0.2)
    noise = 0.01 * torch.rand(n, d, generator=g)
    return (act @ temp + noise).to(device)


def timed_ms(fn, device):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize(device)
    start.record()
    out = fn()
    stop.record()
    torch.cuda.synchronize(device)
    return start.elapsed_time(stop), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="100000x1025,100000x128")
    ap.add_argument("--components", type=int, default=16)
    ap.add_argument("--rank", type=int, default=40)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--max-iter", type=int, default=200)
    ap.add_argument("--sklearn", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("nmf_bench needs the MI355X: there is no CPU path to time")
    device = torch.device("cuda", 0)
    torch.set_grad_enabled(False)
    warnings.simplefilter("ignore")                       # (a fit that reaches max_iter warns; its count is in the line)
    k = args.components
    for shape in args.shapes.split(","):
        n, d = (int(v) for v in shape.split("x"))
        x = frames(n, d, args.rank, device)
        w0, ht0, _, _, _ = native.nmf_start(x, k)
        for _ in range(args.warmup):
            w, ht = w0.clone(), ht0.clone()
            native.nmf_w_half(x, w, ht)
            native.nmf_h_half(x, w, ht)
            x.sum(1)
        stages = {"start": [], "w_half": [], "h_half": [], "iteration": [], "fit": [], "two_reads": [], "dgemm": []}
        n_iter = None
        x64 = x.double()
        for _ in range(args.repeats):
            stages["start"].append(timed_ms(lambda: native.nmf_start(x, k), device)[0])
            w, ht = w0.clone(), ht0.clone()
            stages["w_half"].append(timed_ms(lambda: native.nmf_w_half(x, w, ht), device)[0])
            stages["h_half"].append(timed_ms(lambda: native.nmf_h_half(x, w, ht), device)[0])
            stages["iteration"].append(timed_ms(lambda: (native.nmf_w_half(x, w, ht), native.nmf_h_half(x, w, ht)), device)[0])
            stages["two_reads"].append(timed_ms(lambda: (x.sum(1), x.sum(1)), device)[0])
            stages["dgemm"].append(timed_ms(lambda: x64 @ ht, device)[0])
            nmf = mmk.NMF(n_components=k, max_iter=args.max_iter)
            stages["fit"].append(timed_ms(lambda: nmf(x), device)[0])
            n_iter = nmf.n_iter_
        del x64
        med = {name: statistics.median(v) for name, v in stages.items()}
        line = {"metric": "nmf_stages", "frames": n, "bins": d, "n_components": k, "repeats": args.repeats, "max_iter": args.max_iter}
        line.update({f"{name}_ms": round(v, 3) for name, v in med.items()})
        line.update({f"{name}_ms_min_max": [round(min(v), 3), round(max(v), 3)] for name, v in stages.items()})
        line.update({"n_iter": n_iter, "iteration_over_floor": round(med["iteration"] / med["two_reads"], 2),
                     "two_reads_gbps": round(2.0 * n * d * 4 / (med["two_reads"] * 1e-3) / 1e9, 1), "device": torch.cuda.get_device_name(0)})
        if args.sklearn:
            from sklearn.decomposition import NMF as SkNMF
            host = x.cpu().numpy()
            t0 = time.perf_counter()
            sk = SkNMF(n_components=k, max_iter=args.max_iter, random_state=42)
            sk.fit_transform(host)
            line["sklearn_s"], line["sklearn_n_iter"] = round(time.perf_counter() - t0, 3), int(sk.n_iter_)
        print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
