"""PCA stage times on one MI355X.

    python scripts/pca_bench.py [--shapes 100000x1025,100000x128] [--components 16] [--repeats 7] [--warmup 2] [--sklearn]

Seeded low-rank-plus-noise frames (the recipe of tests/pca_refs.py, on the device).  One JSON line per shape:
  colstats_ms, cov_ms, eig_ms, project_ms   the median over `repeats` runs of each stage's device time (HIP events around the stage,
                                            after `warmup` untimed runs of the whole fit + transform)
  fit_transform_ms                          the median of whole PCA()(x) calls, timed the same way
  n_iter                                    iterations of the subspace iteration
  cov_tflops                                N D^2 useful multiply-adds of the full matrix (2 N D^2 FLOP; the kernel computes one triangle,
                                            so this is the rate a caller sees, not the matrix unit's) / cov_ms
  dgemm_tflops                              torch's float64 z^T z on the same shape in the same run (the library's DGEMM, z formed and
                                            written beforehand, untimed): the float64 matrix rate this run establishes
  cov_fraction_of_dgemm                     cov_tflops / dgemm_tflops - the covariance stage also standardises on load and never writes z
  sklearn_s (with --sklearn)                the host's StandardScaler + PCA on the same frames: context, not a baseline
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

import mimikit_amd as mmk  # noqa: E402
from mimikit_amd import native  # noqa: E402


def frames(n, d, rank, device):
    g = torch.Generator(device="cpu").manual_seed(1000 + d)
    latent = torch.randn(n, rank, generator=g) * (1.3 ** -torch.arange(rank, dtype=torch.float32))
    mix = torch.randn(rank, d, generator=g) / rank ** 0.5
    gain, offset = torch.exp(torch.rand(d, generator=g) * 4 - 2), torch.rand(d, generator=g) * 6 - 3
    noise = 0.1 * torch.randn(n, d, generator=g)
    return ((latent @ mix + noise) * gain + offset).to(device)


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
    ap.add_argument("--sklearn", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("pca_bench needs the MI355X: there is no CPU path to time")
    device = torch.device("cuda", 0)
    torch.set_grad_enabled(False)
    k = args.components
    for shape in args.shapes.split(","):
        n, d = (int(v) for v in shape.split("x"))
        x = frames(n, d, args.rank, device)
        for _ in range(args.warmup):
            mmk.PCA(n_components=k)(x)
        stages = {"colstats": [], "cov": [], "eig": [], "project": [], "fit_transform": []}
        n_iter = None
        for _ in range(args.repeats):
            t, (mean, scale) = timed_ms(lambda: native.pca_colstats(x), device)
            stages["colstats"].append(t)
            t, c = timed_ms(lambda: native.pca_cov(x, mean, scale), device)
            stages["cov"].append(t)
            t, (comps, var, n_iter) = timed_ms(lambda: native.pca_eig(c, k), device)
            stages["eig"].append(t)
            t, _ = timed_ms(lambda: native.pca_project(x, mean, scale, comps), device)
            stages["project"].append(t)
            t, _ = timed_ms(lambda: mmk.PCA(n_components=k)(x), device)
            stages["fit_transform"].append(t)
        z = (x.double() - mean) / scale
        torch.matmul(z.t(), z)
        dgemm = statistics.median(timed_ms(lambda: torch.matmul(z.t(), z), device)[0] for _ in range(args.repeats))
        del z
        med = {name: statistics.median(v) for name, v in stages.items()}
        flop = 2.0 * n * d * d
        cov_tflops, dgemm_tflops = flop / (med["cov"] * 1e-3) / 1e12, flop / (dgemm * 1e-3) / 1e12
        line = {"metric": "pca_stages", "frames": n, "bins": d, "n_components": k, "repeats": args.repeats}
        line.update({f"{name}_ms": round(v, 3) for name, v in med.items()})
        line.update({f"{name}_ms_min_max": [round(min(v), 3), round(max(v), 3)] for name, v in stages.items()})
        line.update({"n_iter": n_iter, "cov_tflops": round(cov_tflops, 3), "dgemm_ms": round(dgemm, 3), "dgemm_tflops": round(dgemm_tflops, 3),
                     "cov_fraction_of_dgemm": round(cov_tflops / dgemm_tflops, 4), "device": torch.cuda.get_device_name(0)})
        if args.sklearn:
            from sklearn.decomposition import PCA as SkPCA
            from sklearn.preprocessing import StandardScaler
            host = x.cpu().numpy()
            t0 = time.perf_counter()
            SkPCA(n_components=k, random_state=42).fit_transform(StandardScaler().fit_transform(host))
            line["sklearn_s"] = round(time.perf_counter() - t0, 3)
        print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
