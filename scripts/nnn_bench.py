"""NearestNextNeighbor alignment benchmark on one MI355X: the cosine-cost kernel and the subsequence-DTW kernel
(csrc/nnn.hip), and the float64 restatement of tests/nnn_refs.py on the host as the baseline - the reference's algorithm where the
reference runs it: on the host, clip by clip.

    python scripts/nnn_bench.py [--iters 20] [--warmup 3] [--no-baseline] [--only N,K,M,B]

One JSON line per shape (N prompt frames, K bins, M corpus frames, B clips):
  cost_us          device time of mmk_inv_row_norm_f32 (prompts) + mmk_cosine_cost_f32 (HIP events around `iters` calls, after `warmup`)
  corpus_tbps      corpus bytes (M K 4) / cost time, and `peak_share` of 8 TB/s: the corpus read is the floor of that kernel
  dtw_us           device time of mmk_dtw_subseq_f32;  dtw_ns_per_column = dtw time / (M + N - 1) anti-diagonals (one wave per clip)
  host_s_per_clip  the float64 restatement (distances + DTW last row + argmin) for ONE clip on one core; `host_s_batch` = that times
                   ceil(B / 16): B clips spread over 16 cores
"""
import argparse
import json
import math
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from mimikit_amd import native  # noqa: E402
from tests import nnn_refs as R  # noqa: E402


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
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--no-baseline", action="store_true")
    ap.add_argument("--only", default=None, help="N,K,M,B")
    args = ap.parse_args()
    device = torch.device("cuda", 0)
    torch.set_grad_enabled(False)
    only = None if args.only is None else tuple(int(v) for v in args.only.split(","))
    gen = torch.Generator().manual_seed(1)
    for k in (513, 1025):
        for m in (10 ** 4, 10 ** 5):
            y = torch.rand(m, k, generator=gen)
            yd = y.to(device)
            ry = native.inv_row_norm(yd)
            for n in (16, 64):
                host = None
                for batch in (1, 8, 32):
                    if only not in (None, (n, k, m, batch)):
                        continue
                    x = torch.rand(batch, n, k, generator=gen)
                    xd = x.to(device)
                    cost = native.cosine_cost(xd, yd, ry)
                    for _ in range(args.warmup):
                        native.cosine_cost(xd, yd, ry)
                        native.dtw_subseq(cost, n)
                    t_cost = timed(lambda: native.cosine_cost(xd, yd, ry), args.iters, device)
                    t_dtw = timed(lambda: native.dtw_subseq(cost, n), args.iters, device)
                    if host is None and not args.no_baseline:
                        t0 = time.perf_counter()
                        R.end_column(R.dtw_last_row(R.cosine_distances(x[0].numpy(), y.numpy())))
                        host = time.perf_counter() - t0
                    line = {"metric": "nnn_alignment", "N": n, "K": k, "M": m, "B": batch, "iters": args.iters,
                            "cost_us": round(t_cost * 1e6, 1), "corpus_tbps": round(m * k * 4 / t_cost / 1e12, 3),
                            "peak_share": round(m * k * 4 / t_cost / 8e12, 4), "cost_tflops": round(2.0 * batch * n * m * k / t_cost / 1e12, 2),
                            "dtw_us": round(t_dtw * 1e6, 1), "dtw_ns_per_column": round(t_dtw * 1e9 / (m + n - 1), 2),
                            "device": torch.cuda.get_device_name(0)}
                    if host is not None:
                        line.update(host_s_per_clip=round(host, 3), host_s_batch=round(host * math.ceil(batch / 16), 3),
                                    speedup_vs_host_batch=round(host * math.ceil(batch / 16) / (t_cost + t_dtw), 1))
                    print(json.dumps(line), flush=True)
                    del cost


if __name__ == "__main__":
    main()
