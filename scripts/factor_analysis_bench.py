"""FactorAnalysis on one MI355X: where the time of a fit goes, and what the warm start of the eigen step buys.

    python scripts/factor_analysis_bench.py [--frames 20000] [--bins 1025 129] [--components 16] [--repeats 7] [--warmup 2] [--sklearn]

Per bin count D: `frames` x D float32 frames with `components` factors, generated as tests/factor_analysis_refs.py generates its fixtures
(falling loadings at snr 2, a noise variance of its own per column, a column offset).  One JSON line per D, appended to
profiles/factor_analysis_bench.jsonl and printed; every time is [median, min, max] ms over `repeats` calls after `warmup` untimed ones,
host clock around the call and a device synchronisation (the EM entry waits for its stream anyway):
  colstats_cov     native.pca_colstats and native.pca_cov: the one pass over the frames
  em               native.fa_fit: the whole EM loop from the D x D covariance
  transform        native.fa_transform_matrix and native.pca_project of the frames
  em_steps, inner_total, inner_step0, inner_later_mean
                   EM steps, inner (subspace) iterations in all, those of EM step 0 (hash start) and the mean of the later steps (warm start)
  em_us_per_inner  the EM entry's median over inner_total: seven launches per inner iteration
  sklearn_ms       with --sklearn and sklearn importable: sklearn's FactorAnalysis.fit_transform on this machine's CPUs, once (information)
No threshold: nothing here passes or fails.
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from mimikit_amd import native  # noqa: E402


def frames(seed, n, d, kt, snr):
    rng = np.random.RandomState(seed)
    load = rng.randn(kt, d) * snr * (np.arange(kt, 0, -1)[:, None] / kt + .5)
    return (rng.randn(n, kt) @ load + rng.randn(n, d) * (.5 + rng.rand(d)) + 3 * rng.rand(d)).astype(np.float32)


def stats_ms(fn, device, warmup, repeats):
    times = []
    for i in range(warmup + repeats):
        torch.cuda.synchronize(device)
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize(device)
        if i >= warmup:
            times.append((time.perf_counter() - t0) * 1e3)
    return [round(statistics.median(times), 4), round(min(times), 4), round(max(times), 4)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=20000)
    ap.add_argument("--bins", type=int, nargs="+", default=[1025, 129])
    ap.add_argument("--components", type=int, default=16)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--sklearn", action="store_true")
    args = ap.parse_args()
    device = torch.device("cuda", 0)
    torch.set_grad_enabled(False)
    out_path = os.path.join(ROOT, "profiles", "factor_analysis_bench.jsonl")
    for d in args.bins:
        n, k = args.frames, args.components
        x_np = frames(4, n, d, k, 2.0)
        x = torch.from_numpy(x_np).to(device)
        ones = torch.ones((d,), dtype=torch.float64, device=device)
        state = {}

        def cov():
            mean, _ = native.pca_colstats(x)
            state["mean"], state["c"] = mean, native.pca_cov(x, mean, ones) * ((n - 1) / n)

        def em():
            state["fit"] = native.fa_fit(state["c"], n, k, 1e-2, 1000)

        def transform():
            comps, noise = state["fit"][:2]
            state["z"] = native.pca_project(x, state["mean"], ones, native.fa_transform_matrix(comps, noise))

        rec = dict(frames=n, bins=d, components=k, device=torch.cuda.get_device_name(device))
        rec["colstats_cov"] = stats_ms(cov, device, args.warmup, args.repeats)
        rec["em"] = stats_ms(em, device, args.warmup, args.repeats)
        rec["transform"] = stats_ms(transform, device, args.warmup, args.repeats)
        _, _, _, n_iter, converged, (total, step0) = state["fit"]
        rec.update(em_steps=n_iter, converged=converged, inner_total=total, inner_step0=step0,
                   inner_later_mean=round((total - step0) / max(n_iter - 1, 1), 3), em_us_per_inner=round(rec["em"][0] * 1e3 / total, 2))
        if args.sklearn:
            try:
                from sklearn.decomposition import FactorAnalysis as skFA
                t0 = time.perf_counter()
                sk = skFA(n_components=k, tol=1e-2, max_iter=1000, random_state=42)
                z = sk.fit_transform(x_np)
                rec["sklearn_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
                rec["sklearn_em_steps"] = int(sk.n_iter_)
                mine = state["z"].cpu().numpy().astype(np.float64)
                sign = np.sign((mine * z).sum(0))
                rec["sklearn_max_dev"] = float(np.abs(mine * sign - z).max() / np.abs(z).max())
            except ImportError:
                rec["sklearn_ms"] = None
        line = json.dumps(rec)
        print(line, flush=True)
        os.makedirs(os.path.dirname(out_path), exist_ok=True)
        with open(out_path, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
