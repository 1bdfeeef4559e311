"""HCluster benchmark on one MI355X: labelling N frames of D bins.

    timeout -k 10 300 python scripts/hcluster_bench.py --part fit   [--frames 65536] [--bins 513] [--rounds 5] [--warmup 1]
    timeout -k 10 300 python scripts/hcluster_bench.py --part level0
    timeout -k 900 900 python scripts/hcluster_bench.py --part reference --frames 8192        (host only: needs the reference tree, no GPU)

One process and one part per call, each call under its own time limit; at most 16 host threads.  One JSON line per part; every time is the
median over `rounds`, with the spread (max - min over the rounds, as a share of the median) beside it:
  fit        HCluster().fit(X): wall time including the one read-back per level; levels and clusters per level; the peak allocation above
             what X holds, beside the 4 N^2 bytes of the matrix the reference forms
  level0     device time (HIP events) of native.nn_cosine_self(X) - level 0's arg-max alone - and of native.nn_cosine(X, X, inv_norm) on the
             same shape, the kernel without the self-exclusion: self_over_plain is their ratio (each call computes the inverse norms of X
             once)
  reference  the reference's own HCluster.fit (numpy, sklearn, scipy) on the host, at the largest N whose float32 matrix is still
             reasonable to hold (8192: 268 MB per copy), on the same seeded input: wall time of ONE fit, and whether the device's labels,
             when --labels-from names an .npy written by `--part fit --save-labels`, are the same
"""
import argparse
import json
import os
import statistics
import sys
import time

os.environ.setdefault("OMP_NUM_THREADS", "16")

import numpy as np  # noqa: E402
import torch  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def frames(n, d):
    """seeded magnitude-like frames: a few strong bins each (cubed uniforms), float32"""
    return torch.rand(n, d, generator=torch.Generator().manual_seed(1)) ** 3


def spread(t):
    med = statistics.median(t)
    return med, (max(t) - min(t)) / med


def device_time(fn, device):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize(device)
    start.record()
    fn()
    stop.record()
    torch.cuda.synchronize(device)
    return start.elapsed_time(stop) * 1e-3


def wall_time(fn, device):
    torch.cuda.synchronize(device)
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize(device)
    return time.perf_counter() - t0


def part_fit(args):
    import mimikit_amd as mmk
    device = torch.device("cuda", 0)
    x = frames(args.frames, args.bins).to(device)
    for _ in range(args.warmup):
        mmk.HCluster().fit(x)
    torch.cuda.synchronize(device)
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats(device)
    before = torch.cuda.memory_allocated(device)
    h = mmk.HCluster().fit(x)
    torch.cuda.synchronize(device)
    peak = torch.cuda.max_memory_allocated(device) - before
    t, s = spread([wall_time(lambda: mmk.HCluster().fit(x), device) for _ in range(args.rounds)])
    if args.save_labels:
        np.save(args.save_labels, h.labels_.cpu().numpy())
    return {"fit_ms": round(t * 1e3, 2), "fit_spread": round(s, 3), "levels": h.labels_.shape[1], "K_": h.K_,
            "clusters_per_level": [int(h.labels_[:, i].max()) + 1 for i in range(h.labels_.shape[1])],
            "peak_bytes": int(peak), "input_bytes": 4 * args.frames * args.bins, "matrix_bytes": 4 * args.frames * args.frames,
            "device": torch.cuda.get_device_name(0)}


def part_level0(args):
    from mimikit_amd import native
    device = torch.device("cuda", 0)
    x = frames(args.frames, args.bins).to(device)
    inv = native.inv_row_norm(x)
    for _ in range(args.warmup):
        native.nn_cosine_self(x)
        native.nn_cosine(x, x, inv)
    t_self, s_self = spread([device_time(lambda: native.nn_cosine_self(x), device) for _ in range(args.rounds)])
    t_plain, s_plain = spread([device_time(lambda: native.nn_cosine(x, x, inv), device) for _ in range(args.rounds)])
    flop = 2.0 * args.frames * args.frames * args.bins
    own = native.nn_cosine(x, x, inv)[0]
    other = native.nn_cosine_self(x)[0]
    return {"self_ms": round(t_self * 1e3, 2), "self_spread": round(s_self, 3), "self_tflops": round(flop / t_self / 1e12, 1),
            "plain_ms": round(t_plain * 1e3, 2), "plain_spread": round(s_plain, 3), "plain_tflops": round(flop / t_plain / 1e12, 1),
            "self_over_plain": round(t_self / t_plain, 3),
            "plain_finds_itself": round(float((own == torch.arange(args.frames, device=device)).float().mean()), 5),
            "self_finds_itself": round(float((other == torch.arange(args.frames, device=device)).float().mean()), 5),
            "device": torch.cuda.get_device_name(0)}


def part_reference(args):
    import importlib
    import types
    from oracle.ref_shim import REFERENCE_ROOT, load_reference
    torch.set_num_threads(min(16, torch.get_num_threads()))
    load_reference()
    pkg = types.ModuleType("mimikit.extract")
    pkg.__path__ = [os.path.join(REFERENCE_ROOT, "mimikit", "extract")]
    sys.modules["mimikit.extract"] = pkg
    CL = importlib.import_module("mimikit.extract.clusters")
    x = frames(args.frames, args.bins).numpy()
    t0 = time.perf_counter()
    h = CL.HCluster().fit(x)
    t = time.perf_counter() - t0
    out = {"reference_fit_s": round(t, 2), "levels": int(h.labels_.shape[1]), "K_": h.K_,
           "clusters_per_level": [int(h.labels_[:, i].max()) + 1 for i in range(h.labels_.shape[1])],
           "host_threads": int(os.environ["OMP_NUM_THREADS"])}
    if args.labels_from:
        ours = np.load(args.labels_from)
        out["same_shape"] = ours.shape == h.labels_.shape
        out["same_labels_share"] = round(float((ours == h.labels_).mean()), 5) if out["same_shape"] else None
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", choices=("fit", "level0", "reference"), required=True)
    ap.add_argument("--frames", type=int, default=65536)
    ap.add_argument("--bins", type=int, default=513)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--save-labels", default=None)
    ap.add_argument("--labels-from", default=None)
    args = ap.parse_args()
    torch.set_grad_enabled(False)
    res = {"fit": part_fit, "level0": part_level0, "reference": part_reference}[args.part](args)
    print(json.dumps({"metric": f"hcluster_{args.part}", "frames": args.frames, "bins": args.bins, "rounds": args.rounds, **res}), flush=True)


if __name__ == "__main__":
    main()
