"""One Lloyd iteration of KMeans on one MI355X: assign every frame to its nearest centre, then sum every label's
frames.

    python scripts/kmeans_bench.py [--parent-lib PATH/libmmk_hip.so] [--shapes 1048576x16x16,262144x128x16,131072x1025x16,131072x1025x256]
                                   [--repeats 15] [--warmup 3] [--fit-shape 262144x128]

N frames of D bins around K seeded centres, centred by their float32 column mean as KMeans.fit does.  One JSON line per shape N x D x K,
appended to profiles/kmeans_bench.jsonl and printed; every entry is [median, min, max] ms over `repeats` calls (HIP events around the call,
after `warmup` untimed calls):
  assign          mmk_half_neg_sqnorm_f32 of the centres + mmk_kmeans_assign_f32 (labels and the changed count), this tree's library
  sums            mmk_kmeans_label_sums_f64 (sums and counts)
  step            the two, one after the other: one Lloyd iteration of this tree
  chain_assign, chain_sums, chain
                  (with --parent-lib only; without it the line holds this tree's times and the copy alone, which is what a comparison
                  of two builds of THIS kernel through MMK_DIAG_LIB needs) the same iteration chained from the entry points the library had before, through the library given by --parent-lib (the
                  PARENT commit's build, never this tree's): mmk_half_neg_sqnorm_f32 -> mmk_nn_topk_f32 (t = 1) for the labels, then a
                  stable torch.sort of the labels -> bincount / cumsum -> mmk_segment_mean_f32 (the means, fp32).  It works on a corpus
                  that was centred beforehand (the parent has no offset argument), which is not timed
  copy            a torch copy of the corpus: the memory floor of one pass; copy_gbps = bytes read + written / median
With --fit-shape N x D one more line: KMeans().fit at the reference's defaults (16 clusters, n_init 2, max_iter 100), wall time of the
whole call, its n_iter_ and inertia_.
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import mimikit_amd as mmk  # noqa: E402
from mimikit_amd import build, native  # noqa: E402

vp, i32, i64, f32 = C.c_void_p, C.c_int32, C.c_int64, C.c_float


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


def parent_library(path):
    """the entry points of the chain in another build of the library, typed by hand (its digest is not this tree's, so native.load_library
    refuses it)"""
    lib = C.CDLL(path)
    for name, res, args in (("mmk_half_neg_sqnorm_f32", i32, [vp, i64, i64, i32, vp, vp]),
                            ("mmk_nn_topk_workspace_bytes", C.c_size_t, [i64, i64, i32]),
                            ("mmk_nn_topk_f32", i32, [vp, i64, vp, i64, vp, i64, vp, vp, f32, f32, i64, i32, i32, i32, vp, vp, vp, C.c_size_t, vp]),
                            ("mmk_segment_mean_f32", i32, [vp, i64, i64, i32, vp, vp, i64, vp, i64, vp]),
                            ("mmk_build_digest", C.c_char_p, [])):
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = res, args
    assert not hasattr(lib, "mmk_kmeans_assign_f32"), "--parent-lib names a library that has the new kernels: the baseline is the parent commit's build"
    return lib


def corpus(n, d, k, device):
    g = torch.Generator(device="cpu").manual_seed(n + d + k)
    centres = torch.rand((k, d), generator=g) * 2 - 1
    x = torch.empty((n, d), dtype=torch.float32, device=device)
    step = max(1, (1 << 24) // d)
    for r0 in range(0, n, step):
        r1 = min(n, r0 + step)
        x[r0:r1] = (centres[torch.randint(0, k, (r1 - r0,), generator=g)] + 0.5 * torch.randn((r1 - r0, d), generator=g)).to(device)
    return x, centres.to(device)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="1048576x16x16,262144x128x16,131072x1025x16,131072x1025x256")
    ap.add_argument("--repeats", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--fit-shape", default="")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "kmeans_bench.jsonl"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("kmeans_bench needs the MI355X: there is no CPU path to time")
    device = torch.device("cuda", 0)
    torch.set_grad_enabled(False)
    parent = parent_library(args.parent_lib) if args.parent_lib else None
    lib, stream = native.lib(), native.stream_ptr(device)
    lines = []
    for shape in args.shapes.split(","):
        n, d, k = (int(v) for v in shape.split("x"))
        x, centres = corpus(n, d, k, device)
        mu = x.double().mean(0).float() if n * d <= 1 << 27 else native.pca_colstats(x)[0].float()
        centres = centres - mu
        labels = torch.full((n,), -1, dtype=torch.int32, device=device)
        changed = torch.zeros((), dtype=torch.int64, device=device)
        shift = torch.empty((k,), dtype=torch.float32, device=device)
        sums = torch.empty((k, d), dtype=torch.float64, device=device)
        counts = torch.empty((k,), dtype=torch.int64, device=device)
        n_work = lib.mmk_kmeans_label_sums_workspace_bytes(n, d, k)
        work = torch.empty((n_work // 8,), dtype=torch.float64, device=device)

        def assign():
            assert lib.mmk_half_neg_sqnorm_f32(centres.data_ptr(), d, k, d, shift.data_ptr(), stream) == 0
            assert lib.mmk_kmeans_assign_f32(x.data_ptr(), d, mu.data_ptr(), n, d, centres.data_ptr(), d, shift.data_ptr(), k, labels.data_ptr(), None,
                                             changed.data_ptr(), stream) == 0

        def label_sums():
            assert lib.mmk_kmeans_label_sums_f64(x.data_ptr(), d, mu.data_ptr(), n, d, labels.data_ptr(), k, sums.data_ptr(), counts.data_ptr(), None, 0,
                                                 None, None, work.data_ptr(), n_work, stream) == 0

        # the chain of the parent's entry points, on a corpus centred beforehand
        xc = x - mu
        ones = torch.ones((max(n, k),), dtype=torch.float32, device=device)
        index = torch.empty((n, 1), dtype=torch.int64, device=device)
        key = torch.empty((n, 1), dtype=torch.float32, device=device)
        n_topk = parent.mmk_nn_topk_workspace_bytes(n, k, 1) if parent else 0
        topk_work = torch.empty((n_topk // 4,), dtype=torch.float32, device=device)
        means = torch.empty((k, d), dtype=torch.float32, device=device)
        offsets = torch.zeros((k + 1,), dtype=torch.int64, device=device)

        def chain_assign():
            assert parent.mmk_half_neg_sqnorm_f32(centres.data_ptr(), d, k, d, shift.data_ptr(), stream) == 0
            assert parent.mmk_nn_topk_f32(xc.data_ptr(), d, ones.data_ptr(), n, centres.data_ptr(), d, ones.data_ptr(), shift.data_ptr(), float("-inf"),
                                          float("inf"), k, d, 1, 0, index.data_ptr(), key.data_ptr(), topk_work.data_ptr(), n_topk, stream) == 0

        def chain_sums():
            order = torch.sort(index[:, 0], stable=True)[1]
            torch.cumsum(torch.bincount(index[:, 0], minlength=k), 0, out=offsets[1:])
            assert parent.mmk_segment_mean_f32(xc.data_ptr(), d, n, d, order.data_ptr(), offsets.data_ptr(), k, means.data_ptr(), d, stream) == 0

        line = {"metric": "kmeans_step", "n": n, "d": d, "k": k, "repeats": args.repeats, "unit": "ms [median, min, max]"}
        line["assign"] = stats_ms(assign, device, args.warmup, args.repeats)
        line["sums"] = stats_ms(label_sums, device, args.warmup, args.repeats)
        line["step"] = stats_ms(lambda: (assign(), label_sums()), device, args.warmup, args.repeats)
        if parent:
            line["chain_assign"] = stats_ms(chain_assign, device, args.warmup, args.repeats)
            assert torch.equal(index[:, 0].int(), labels), "the chain's labels and the new kernel's differ"
            assert int(torch.bincount(index[:, 0], minlength=k).min()) > 0, "the chain's segment_mean takes no empty segment: pick other centres"
            line["chain_sums"] = stats_ms(chain_sums, device, args.warmup, args.repeats)
            line["chain"] = stats_ms(lambda: (chain_assign(), chain_sums()), device, args.warmup, args.repeats)
            line.update({"step_over_chain": round(line["step"][0] / line["chain"][0], 3), "parent_digest": parent.mmk_build_digest().decode(),
                         "means_max_abs_diff": float(((sums / counts[:, None]).float() - means).abs().max())})
        dst = torch.empty_like(x)
        line["copy"] = stats_ms(lambda: dst.copy_(x), device, args.warmup, args.repeats)
        line.update({"corpus_bytes": 4 * n * d, "copy_gbps": round(2 * 4 * n * d / (line["copy"][0] * 1e-3) / 1e9, 1),
                     "assign_over_half_copy": round(line["assign"][0] / (line["copy"][0] / 2), 2), "device": torch.cuda.get_device_name(0),
                     "library_digest": lib.mmk_build_digest().decode(), "date": time.strftime("%Y-%m-%d")})
        lines.append(line)
        del dst, xc, x, topk_work, work
    if args.fit_shape:
        n, d = (int(v) for v in args.fit_shape.split("x"))
        x, _ = corpus(n, d, 16, device)
        mmk.KMeans().fit(x[:4096])                       # (code loading, the allocator's first blocks)
        torch.cuda.synchronize(device)
        t0 = time.perf_counter()
        km = mmk.KMeans().fit(x)
        torch.cuda.synchronize(device)
        lines.append({"metric": "kmeans_fit", "n": n, "d": d, "k": km.n_clusters, "n_init": km.n_init, "max_iter": km.max_iter, "wall_ms": round((time.perf_counter() - t0) * 1e3, 2),
                      "n_iter": km.n_iter_, "inertia": km.inertia_, "device": torch.cuda.get_device_name(0), "library_digest": build.library_digest(),
                      "date": time.strftime("%Y-%m-%d")})
    with open(args.out, "a") as fh:
        for line in lines:
            text = json.dumps(line)
            print(text, flush=True)
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
