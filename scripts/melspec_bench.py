"""MelSpec / MFCC times on one MI355X.

    python scripts/melspec_bench.py [--configs 1024x256x0,2048x512x1] [--clips 64] [--seconds 10] [--repeats 15] [--warmup 3]
                                    [--parent-lib PATH/libmmk_hip.so]

bench.py's `stft` workload: `clips` clips of `seconds` s at 22050 Hz, seeded noise.  One JSON line per config n_fft x hop x center, appended
to profiles/melspec_bench.jsonl and printed; every entry is [median, min, max] ms over `repeats` calls (HIP events around the call, after
`warmup` untimed calls):
  magspec         (a) MagSpec alone, this tree's library
  magspec_abi, magspec_parent
                  (a) the same as a bare mmk_stft_mag_f32 call into one output buffer, through this tree's library and through the one
                  given by --parent-lib (the parent commit's build), timed turn by turn; the two must agree within their min-max ranges,
                  or the shared kernels were disturbed
  two_launches    (b) MelSpec()(MagSpec()(x))
  mel_fused       (c) MelSpec().from_signal(x, MagSpec(...))
  mfcc_fused      (d) MFCC().from_signal(x, MagSpec(...), MelSpec())
  copy            (e) a torch copy of a tensor of the spectrogram's size; copy_gbps = bytes read + written / median
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from mimikit_amd import build, native  # noqa: E402
from mimikit_amd.features.functionals import MFCC, MagSpec, MelSpec  # noqa: E402


def timed_ms(fn, device):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize(device)
    start.record()
    fn()
    stop.record()
    torch.cuda.synchronize(device)
    return start.elapsed_time(stop)


def summary(times):
    return [round(statistics.median(times), 4), round(min(times), 4), round(max(times), 4)]


def stats_ms(fn, device, warmup, repeats):
    for _ in range(warmup):
        fn()
    return summary([timed_ms(fn, device) for _ in range(repeats)])


def stats_ms_pair(fn_a, fn_b, device, warmup, repeats):
    """two callables timed turn by turn (a b b a a b ..), so that neither has the warmer clocks or caches of coming second"""
    for _ in range(warmup):
        fn_a(), fn_b()
    ta, tb = [], []
    for i in range(repeats):
        for which in ((0, 1) if i % 2 == 0 else (1, 0)):
            (ta if which == 0 else tb).append(timed_ms(fn_a if which == 0 else fn_b, device))
    return summary(ta), summary(tb)


def parent_magspec(path):
    """mmk_stft_mag_f32 of another build of the library, typed by hand (its digest is not this tree's, so native.load_library refuses it)"""
    lib = C.CDLL(path)
    lib.mmk_stft_n_frames.restype = C.c_int64
    lib.mmk_stft_n_frames.argtypes = [C.c_int64, C.c_int32, C.c_int32, C.c_int32]
    lib.mmk_stft_mag_f32.restype = C.c_int32
    lib.mmk_stft_mag_f32.argtypes = [C.c_void_p, C.c_int64, C.c_int32, C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p]
    lib.mmk_build_digest.restype = C.c_char_p
    return lib


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="1024x256x0,2048x512x1")
    ap.add_argument("--clips", type=int, default=64)
    ap.add_argument("--seconds", type=float, default=10.0)
    ap.add_argument("--repeats", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "melspec_bench.jsonl"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("melspec_bench needs the MI355X: there is no CPU path to time")
    device = torch.device("cuda", 0)
    torch.set_grad_enabled(False)
    parent = parent_magspec(args.parent_lib) if args.parent_lib else None
    n = int(args.seconds * 22050)
    x = torch.randn((args.clips, n), generator=torch.Generator(device="cpu").manual_seed(22050)).mul_(0.1).to(device)
    for config in args.configs.split(","):
        n_fft, hop, center = (int(v) for v in config.split("x"))
        magspec = MagSpec(n_fft, hop, center=bool(center), alignment=None)
        melspec, mfcc = MelSpec(), MFCC()
        spec = magspec(x)
        assert torch.equal(melspec.from_signal(x, magspec), melspec(spec))
        line = {"metric": "melspec", "n_fft": n_fft, "hop": hop, "center": bool(center), "clips": args.clips, "samples": n,
                "frames": spec.shape[1], "repeats": args.repeats, "unit": "ms [median, min, max]"}
        line["magspec"] = stats_ms(lambda: magspec(x), device, args.warmup, args.repeats)
        if parent is not None:
            out = torch.empty_like(spec)
            stream = native.stream_ptr(device)

            def call(lib):
                rc = lib.mmk_stft_mag_f32(x.data_ptr(), x.stride(0), x.shape[0], n, n_fft, hop, center, out.data_ptr(), stream)
                assert rc == 0, rc
            line["magspec_abi"], line["magspec_parent"] = stats_ms_pair(lambda: call(native.lib()), lambda: call(parent), device, args.warmup,
                                                                        args.repeats)
            assert torch.equal(out, spec), "the parent's MagSpec and this tree's differ"
            line["parent_digest"] = parent.mmk_build_digest().decode()
            del out
        line["two_launches"] = stats_ms(lambda: melspec(magspec(x)), device, args.warmup, args.repeats)
        line["mel_fused"] = stats_ms(lambda: melspec.from_signal(x, magspec), device, args.warmup, args.repeats)
        line["mfcc_fused"] = stats_ms(lambda: mfcc.from_signal(x, magspec, melspec), device, args.warmup, args.repeats)
        dst = torch.empty_like(spec)
        line["copy"] = stats_ms(lambda: dst.copy_(spec), device, args.warmup, args.repeats)
        line["spectrogram_bytes"] = 4 * spec.numel()
        line["copy_gbps"] = round(2 * 4 * spec.numel() / (line["copy"][0] * 1e-3) / 1e9, 1)
        line.update({"device": torch.cuda.get_device_name(0), "library_digest": build.library_digest()})
        text = json.dumps(line)
        print(text, flush=True)
        with open(args.out, "a") as fh:
            fh.write(text + "\n")
        del dst, spec


if __name__ == "__main__":
    main()
