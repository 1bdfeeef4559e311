"""QCluster benchmark on one MI355X: labelling N clustered frames of D bins.

    timeout -k 10 300 python scripts/qcluster_bench.py --part fit    [--frames 65536] [--bins 513] [--rounds 5] [--warmup 1]
    timeout -k 10 300 python scripts/qcluster_bench.py --part topk
    timeout -k 900 900 python scripts/qcluster_bench.py --part reference --frames 8192       (host only: needs the reference tree, no GPU)

One process and one part per call, each call under its own time limit; at most 16 host threads.  One JSON line per part; every time is the
median over `rounds`, with the spread (max - min over the rounds, as a share of the median) beside it.  The frames are clustered (seeded
centres plus noise), not uniform noise, which collapses to one cluster:
  fit        QCluster().fit(X): wall time including its synchronisations; K_, the cores; the peak allocation above what X holds, beside
             the 4 N^2 bytes of a distance matrix
  topk       device time (HIP events) of native.nn_topk(X, X, T, "cosine", self_exclude=True) with T = 9 and T = 16, beside
             native.nn_cosine_self(X) on the same shape - the arg-max kernel the k-best kernel shares its tile walk with:
             topk_over_argmax is their ratio (each call computes the inverse norms of X once); T = 8, euclidean - the call of the default
             fit - as well
  reference  the reference's own QCluster.fit (sklearn, scipy) on the host at N = 8192 on the same seeded input: wall time of ONE fit, and
             the share of equal labels when --labels-from names an .npy written by `--part fit --save-labels`
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

CENTRES = 24


def frames(n, d):
    """seeded clustered frames: one of CENTRES centres (uniform in [-1, 1]) plus 0.3 x normal noise, float32"""
    g = torch.Generator().manual_seed(1)
    centres = torch.rand(CENTRES, d, generator=g) * 2 - 1
    return centres[torch.randint(0, CENTRES, (n,), generator=g)] + 0.3 * torch.randn(n, d, generator=g)


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
        mmk.QCluster().fit(x)
    torch.cuda.synchronize(device)
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats(device)
    before = torch.cuda.memory_allocated(device)
    q = mmk.QCluster().fit(x)
    torch.cuda.synchronize(device)
    peak = torch.cuda.max_memory_allocated(device) - before
    t, s = spread([wall_time(lambda: mmk.QCluster().fit(x), device) for _ in range(args.rounds)])
    if args.save_labels:
        np.save(args.save_labels, q.labels_.cpu().numpy())
    sizes = torch.bincount(q.labels_)
    return {"fit_ms": round(t * 1e3, 2), "fit_spread": round(s, 3), "K_": q.K_, "cores": int(q.is_core_.sum()),
            "largest_clusters": sorted(sizes.cpu().tolist(), reverse=True)[:8], "centres": CENTRES,
            "peak_bytes": int(peak), "input_bytes": 4 * args.frames * args.bins, "matrix_bytes": 4 * args.frames * args.frames,
            "device": torch.cuda.get_device_name(0)}


def part_topk(args):
    from mimikit_amd import native
    device = torch.device("cuda", 0)
    x = frames(args.frames, args.bins).to(device)
    calls = {"argmax": lambda: native.nn_cosine_self(x),
             "topk9": lambda: native.nn_topk(x, x, 9, "cosine", self_exclude=True),
             "topk16": lambda: native.nn_topk(x, x, 16, "cosine", self_exclude=True),
             "topk8_euclidean": lambda: native.nn_topk(x, x, 8, "euclidean", self_exclude=True)}
    out = {}
    flop = 2.0 * args.frames * args.frames * args.bins
    for name, fn in calls.items():
        for _ in range(args.warmup):
            fn()
        t, s = spread([device_time(fn, device) for _ in range(args.rounds)])
        out[f"{name}_ms"], out[f"{name}_spread"], out[f"{name}_tflops"] = round(t * 1e3, 2), round(s, 3), round(flop / t / 1e12, 1)
    for name in ("topk9", "topk16", "topk8_euclidean"):
        out[f"{name}_over_argmax"] = round(out[f"{name}_ms"] / out["argmax_ms"], 3)
    out["topk_over_argmax"] = out["topk16_over_argmax"]
    out["first_equals_argmax"] = round(float((calls["topk9"]()[0][:, 0] == calls["argmax"]()[0]).float().mean()), 5)
    out["device"] = torch.cuda.get_device_name(0)
    return out


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
    q = CL.QCluster().fit(x)
    t = time.perf_counter() - t0
    out = {"reference_fit_s": round(t, 2), "K_": int(q.K_), "cores": int(q.is_core_.sum()),
           "largest_clusters": sorted(np.bincount(q.labels_).tolist(), reverse=True)[:8], "host_threads": int(os.environ["OMP_NUM_THREADS"])}
    if args.labels_from:
        ours = np.load(args.labels_from)
        out["same_shape"] = ours.shape == q.labels_.shape
        out["same_labels_share"] = round(float((ours == q.labels_).mean()), 5) if out["same_shape"] else None
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", choices=("fit", "topk", "reference"), required=True)
    ap.add_argument("--frames", type=int, default=65536)
    ap.add_argument("--bins", type=int, default=513)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--save-labels", default=None)
    ap.add_argument("--labels-from", default=None)
    args = ap.parse_args()
    torch.set_grad_enabled(False)
    res = {"fit": part_fit, "topk": part_topk, "reference": part_reference}[args.part](args)
    print(json.dumps({"metric": f"qcluster_{args.part}", "frames": args.frames, "bins": args.bins, "rounds": args.rounds, **res}), flush=True)


if __name__ == "__main__":
    main()
