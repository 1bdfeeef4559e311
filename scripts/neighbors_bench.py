"""Clip-scoring benchmark on one MI355X: 32 clips x 2584 frames x 1025 bins against a corpus of M frames.

    python scripts/neighbors_bench.py [--iters 3] [--rounds 5] [--warmup 1] [--corpus 131072 16384]

One JSON line per corpus size.  Every time is the median over `rounds` of the device time of `iters` back-to-back calls (HIP events), with the
spread (max - min over the rounds, as a share of the median) beside it:
  fused_ms         NeighborScorer.neighbors: inverse norms of the queries and the fused cosine arg-max (mmk_nn_cosine_f32); the (rows, M) matrix
                   is never formed
  torch_ms         the only device route there was before it - the measure, not the code under test: torch.matmul of a chunk of normalised
                   query rows with the normalised corpus into one reused (chunk, M) buffer, clamp, max over the corpus, chunk by chunk, the
                   chunk sized so that the buffer fits in --chunk-bytes
  *_tflops         2 rows M bins floating-point operations over that time (the GEMM alone: what the algorithm needs, not what either
                   route executes besides)
  *_peak_bytes     torch.cuda.max_memory_allocated over one call, above what the inputs hold
  entropy_ms       cum_entropy of the 32 rows of neighbours (mmk_cum_entropy_i64)
  same_neighbours  the share of rows on which the two routes return the same index
"""
import argparse
import json
import os
import statistics
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


def rounds_of(fn, args, device):
    for _ in range(args.warmup):
        fn()
    t = [timed(fn, args.iters, device) for _ in range(args.rounds)]
    med = statistics.median(t)
    return med, (max(t) - min(t)) / med


def peak_of(fn, device):
    torch.cuda.synchronize(device)
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats(device)
    before = torch.cuda.memory_allocated(device)
    out = fn()
    torch.cuda.synchronize(device)
    peak = torch.cuda.max_memory_allocated(device) - before
    return out, int(peak)


def torch_route(x, y_unit_t, chunk):
    """x (rows, k) queries, y_unit_t (k, M) the normalised corpus, transposed once outside the timed region"""
    rows, m = x.shape[0], y_unit_t.shape[1]
    buf = torch.empty((chunk, m), dtype=torch.float32, device=x.device)
    index = torch.empty((rows,), dtype=torch.int64, device=x.device)
    best = torch.empty((rows,), dtype=torch.float32, device=x.device)
    for r0 in range(0, rows, chunk):
        xc = x[r0:r0 + chunk]
        xc = xc / xc.norm(dim=-1, keepdim=True).clamp_min(1e-30)
        out = buf[:xc.shape[0]]
        torch.matmul(xc, y_unit_t, out=out)
        v, j = out.clamp_(-1.0, 1.0).max(dim=-1)
        best[r0:r0 + chunk], index[r0:r0 + chunk] = v, j
    return index, best


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--clips", type=int, default=32)
    ap.add_argument("--frames", type=int, default=2584)
    ap.add_argument("--bins", type=int, default=1025)
    ap.add_argument("--corpus", type=int, nargs="+", default=[131072, 16384])
    ap.add_argument("--chunk-bytes", type=int, default=2 << 30)
    args = ap.parse_args()
    device = torch.device("cuda", 0)
    torch.set_grad_enabled(False)
    gen = torch.Generator().manual_seed(1)
    rows = args.clips * args.frames
    x = (torch.rand(args.clips, args.frames, args.bins, generator=gen) ** 3).to(device)
    for m in args.corpus:
        y = (torch.rand(m, args.bins, generator=gen) ** 3).to(device)
        scorer = mmk.NeighborScorer(y)
        y_unit_t = (y * scorer.inv_norm[:, None]).t().contiguous()
        chunk = max(128, min(rows, args.chunk_bytes // (4 * m)))
        x2 = x.reshape(rows, args.bins)
        flop = 2.0 * rows * m * args.bins
        (nn, _), fused_peak = peak_of(lambda: scorer.neighbors(x), device)
        (tj, _), torch_peak = peak_of(lambda: torch_route(x2, y_unit_t, chunk), device)
        t_fused, s_fused = rounds_of(lambda: scorer.neighbors(x), args, device)
        t_torch, s_torch = rounds_of(lambda: torch_route(x2, y_unit_t, chunk), args, device)
        t_ent, s_ent = rounds_of(lambda: mmk.cum_entropy(nn), args, device)
        print(json.dumps({
            "metric": "neighbors", "clips": args.clips, "frames": args.frames, "bins": args.bins, "corpus": m, "rows": rows, "iters": args.iters,
            "rounds": args.rounds, "chunk_rows": chunk,
            "fused_ms": round(t_fused * 1e3, 2), "fused_spread": round(s_fused, 3), "fused_tflops": round(flop / t_fused / 1e12, 1),
            "torch_ms": round(t_torch * 1e3, 2), "torch_spread": round(s_torch, 3), "torch_tflops": round(flop / t_torch / 1e12, 1),
            "fused_over_torch": round(t_fused / t_torch, 3),
            "fused_peak_bytes": fused_peak, "torch_peak_bytes": torch_peak, "matrix_bytes": 4 * rows * m,
            "entropy_ms": round(t_ent * 1e3, 3), "entropy_spread": round(s_ent, 3),
            "same_neighbours": round(float((nn.reshape(-1) == tj).float().mean()), 5),
            "device": torch.cuda.get_device_name(0)}), flush=True)
        del y, scorer, y_unit_t


if __name__ == "__main__":
    main()
