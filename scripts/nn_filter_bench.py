"""NearestNeighborFilter on one MI355X: the k-nearest search, the new gather-and-aggregate launch, and the
torch composition that launch replaces.

    python scripts/nn_filter_bench.py [--shape 16384x1025] [--k 16] [--metric cosine] [--clusters 256] [--repeats 15] [--warmup 3]

N frames of D bins around --clusters seeded centres (|centre + 0.25 noise|: frames have near neighbours, as a corpus has, and most links
are mutual within a cluster; on uniform noise few are and the launch has little to read).  One JSON line, appended to profiles/nn_filter_bench.jsonl and printed; every time is
[median, min, max] ms over `repeats` calls (HIP events around the call, after `warmup` untimed calls):
  search      native.nn_topk(x, x, k, metric, self_exclude=True): the norms or shifts and the two launches of the search
  aggregate   native.nn_aggregate(x, index, "median", mutual=True): the new launch (and the allocation of its output)
  torch       the composition it replaces, on the same index: the mutual mask by a comparison of (N, k, k) gathered slots, x[index] - the
              (N, k, D) block of neighbour rows, 4 N k D bytes - a sort along k with the slots that do not count at +inf, and the pick of the
              one or two middle values by the row's count.  Its result must equal the launch's, bit for bit.
  copy        a torch copy of the frames: the memory floor of one pass
aggregate_bytes = 4 N D (1 + mean count) read + 4 N D written - what the launch has to move if every neighbour row is read once per
output row; aggregate_gbps = that over the median; over 8000 GB/s, the HBM peak, as aggregate_share_of_peak.
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

PEAK_GBPS = 8000.0


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


def torch_median_filter(x, index):
    """the composition: (N, k) mutual mask, the (N, k, D) block, sort, pick"""
    n, k = index.shape
    rows = torch.arange(n, device=x.device)
    listed = (index >= 0) & (index < n) & (index != rows[:, None])
    safe = torch.where(listed, index, torch.zeros_like(index))
    mutual = listed & (index[safe] == rows[:, None, None]).any(-1)
    count = mutual.sum(-1)
    block = x[safe]                                                                   # (N, k, D)
    block = torch.where(mutual[:, :, None], block, torch.full((), float("inf"), device=x.device))
    block = torch.sort(block, dim=1)[0]
    lo = ((count - 1).clamp(min=0) // 2)[:, None, None].expand(n, 1, x.shape[1])
    hi = (count // 2).clamp(max=k - 1)[:, None, None].expand(n, 1, x.shape[1])
    med = (torch.gather(block, 1, lo)[:, 0] + torch.gather(block, 1, hi)[:, 0]) * 0.5
    med = torch.where((count % 2 == 1)[:, None], torch.gather(block, 1, lo)[:, 0], med)
    return torch.where((count == 0)[:, None], x, med)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="16384x1025")
    ap.add_argument("--k", type=int, default=16)
    ap.add_argument("--metric", default="cosine")
    ap.add_argument("--clusters", type=int, default=256)
    ap.add_argument("--repeats", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "nn_filter_bench.jsonl"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("nn_filter_bench needs the MI355X: there is no CPU path to time")
    device = torch.device("cuda", 0)
    torch.set_grad_enabled(False)
    n, d = (int(v) for v in args.shape.split("x"))
    g = torch.Generator().manual_seed(n + d)
    centres = torch.rand((args.clusters, d), generator=g)
    x = (centres[torch.randint(0, args.clusters, (n,), generator=g)] + 0.25 * torch.randn((n, d), generator=g)).abs().to(device)
    index, _ = native.nn_topk(x, x, args.k, args.metric, self_exclude=True)
    out, count = native.nn_aggregate(x, index, "median", mutual=True, return_count=True)
    want = torch_median_filter(x, index)
    same = torch.equal(out.view(torch.int32), want.view(torch.int32))
    del want
    mean_count = float(count.double().mean())
    line = {"metric": "nn_filter", "n": n, "d": d, "k": args.k, "distance": args.metric, "clusters": args.clusters, "op": "median", "repeats": args.repeats,
            "unit": "ms [median, min, max]", "mean_count": round(mean_count, 3), "rows_without_neighbour": int((count == 0).sum()),
            "torch_composition_equal_bits": same}
    line["search"] = stats_ms(lambda: native.nn_topk(x, x, args.k, args.metric, self_exclude=True), device, args.warmup, args.repeats)
    line["aggregate"] = stats_ms(lambda: native.nn_aggregate(x, index, "median", mutual=True), device, args.warmup, args.repeats)
    line["aggregate_mean"] = stats_ms(lambda: native.nn_aggregate(x, index, "mean", mutual=True), device, args.warmup, args.repeats)
    line["aggregate_max"] = stats_ms(lambda: native.nn_aggregate(x, index, "max", mutual=True), device, args.warmup, args.repeats)
    line["torch"] = stats_ms(lambda: torch_median_filter(x, index), device, args.warmup, args.repeats)
    dst = torch.empty_like(x)
    line["copy"] = stats_ms(lambda: dst.copy_(x), device, args.warmup, args.repeats)
    moved = 4.0 * n * d * (1 + mean_count) + 4.0 * n * d
    gbps = moved / (line["aggregate"][0] * 1e-3) / 1e9
    line.update({"aggregate_bytes": int(moved), "aggregate_gbps": round(gbps, 1), "aggregate_share_of_peak": round(gbps / PEAK_GBPS, 3),
                 "torch_block_bytes": 4 * n * args.k * d, "torch_over_aggregate": round(line["torch"][0] / line["aggregate"][0], 2),
                 "copy_gbps": round(2 * 4 * n * d / (line["copy"][0] * 1e-3) / 1e9, 1), "device": torch.cuda.get_device_name(0),
                 "library_digest": native.lib().mmk_build_digest().decode(), "date": time.strftime("%Y-%m-%d")})
    text = json.dumps(line)
    print(text, flush=True)
    with open(args.out, "a") as fh:
        fh.write(text + "\n")


if __name__ == "__main__":
    main()
