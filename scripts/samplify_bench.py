"""Samplifyer stage times on one MI355X.

    python scripts/samplify_bench.py [--seconds 60] [--sr 44100] [--filter-level 1] [--sensitivity 0.05] [--repeats 7] [--warmup 2]

A seeded signal of decaying tone bursts over faint noise, made on the device.  One JSON line:
  transforms_ms     every level's Envelop(interp_to_time_domain=False) and Derivative(normalize=True): the median over `repeats` runs of the
                    stage's device time (HIP events around the stage, after `warmup` untimed runs).  This IS the sum of the existing Envelop and
                    Derivative calls, measured in the same run: the yardstick of everything after it
  coef_ms           the coefficient solves of every level (two rows each)
  periods_ms        the count and fill calls of the coarse gradient, with the host's wait for the two counts between them
  scores_ms         the score kernel and the torch.nonzero that reads the number kept
  cuts_ms           side, refine and snap of the kept cuts
  fit_ms            whole Samplifyer.fit calls, timed the same way; n_attacks, n_cuts
  eval_ms           ONE spline evaluation to T float32 (the coarse envelope), which a fit does not do; eval_gbps = T 4 bytes / eval_ms
  read_ms           one streaming read of the signal (torch's sum): a level's transform must read the samples once; transforms_floor_ms =
                    levels * read_ms, selection_bytes = the coefficients of every level plus 4 bytes per evaluated sample
"""
import argparse
import json
import math
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import mimikit_amd as mmk  # noqa: E402
from mimikit_amd import native  # noqa: E402


def signal(seconds, sr, device):
    g = torch.Generator(device="cpu").manual_seed(4410)
    T = int(seconds * sr)
    t = torch.arange(T, dtype=torch.float64, device=device) / sr
    y = (0.003 * torch.randn(T, generator=g, dtype=torch.float64)).to(device)
    for start in torch.sort(torch.rand(int(2 * seconds), generator=g) * (seconds - 0.5))[0].tolist():
        f, amp, tau = 150 + 750 * float(torch.rand(1, generator=g)), 0.4 + 0.6 * float(torch.rand(1, generator=g)), 0.04 + 0.1 * float(torch.rand(1, generator=g))
        on = t >= start
        dt = t[on] - start
        y[on] += amp * torch.sin(2 * math.pi * f * dt) * torch.exp(-dt / tau) * (1 - torch.exp(-dt / 0.004))
    return (y / y.abs().max()).float()


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
    ap.add_argument("--seconds", type=float, default=60.0)
    ap.add_argument("--sr", type=int, default=44100)
    ap.add_argument("--filter-level", type=int, default=1)
    ap.add_argument("--sensitivity", type=float, default=0.05)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("samplify_bench needs the MI355X: there is no CPU path to time")
    device = torch.device("cuda", 0)
    torch.set_grad_enabled(False)
    y = signal(args.seconds, args.sr, device)
    T = y.shape[0]
    s = mmk.Samplifyer(filter_level=args.filter_level, sensitivity=args.sensitivity)
    levels = s.levels

    def transforms():
        out = []
        for lv in levels:
            e = lv.env_ex(y)
            out.append(torch.stack((e, lv.dx(e[None, :])[0])))
        return out

    def coefs(frames):
        return [native.spline2_coef(f) for f in frames]

    def scores(c, att, dec):
        sc, ea, ed, keep = native.samplify_scores(c[0][0], T, att, dec, args.sensitivity)
        return torch.nonzero(keep).reshape(-1)

    for _ in range(args.warmup):
        s.fit(y)
        y.sum()
    stages = {k: [] for k in ("transforms", "coef", "periods", "scores", "cuts", "fit", "eval", "read")}
    for _ in range(args.repeats):
        ms, frames = timed_ms(transforms, device)
        stages["transforms"].append(ms)
        ms, c = timed_ms(lambda: coefs(frames), device)
        stages["coef"].append(ms)
        ms, (att, dec, _) = timed_ms(lambda: native.periods(c[0][1], T), device)
        stages["periods"].append(ms)
        ms, kept = timed_ms(lambda: scores(c, att, dec), device)
        stages["scores"].append(ms)
        ms, _ = timed_ms(lambda: native.samplify_cuts(y, [k[0] for k in c], [k[1] for k in c], att[kept], dec[kept]), device)
        stages["cuts"].append(ms)
        stages["fit"].append(timed_ms(lambda: s.fit(y), device)[0])
        stages["eval"].append(timed_ms(lambda: native.spline2_eval(c[0][0], T), device)[0])
        stages["read"].append(timed_ms(lambda: y.sum(), device)[0])
    med = {name: statistics.median(v) for name, v in stages.items()}
    coef_bytes = sum(2 * 8 * lv.n_frames(T) for lv in levels)
    line = {"metric": "samplify_stages", "samples": T, "sr": args.sr, "filter_level": args.filter_level, "levels": len(levels),
            "sensitivity": args.sensitivity, "repeats": args.repeats}
    line.update({f"{name}_ms": round(v, 3) for name, v in med.items()})
    line.update({f"{name}_ms_min_max": [round(min(v), 3), round(max(v), 3)] for name, v in stages.items()})
    line.update({"n_attacks": int(att.shape[0]), "n_cuts": int(s.cuts.shape[0]), "transforms_floor_ms": round(len(levels) * med["read"], 3),
                 "selection_over_transforms": round((med["coef"] + med["periods"] + med["scores"] + med["cuts"]) / med["transforms"], 3),
                 "coef_bytes": coef_bytes, "selection_bytes": coef_bytes + 4 * T,
                 "eval_gbps": round(4.0 * T / (med["eval"] * 1e-3) / 1e9, 1), "read_gbps": round(4.0 * T / (med["read"] * 1e-3) / 1e9, 1),
                 "device": torch.cuda.get_device_name(0)})
    print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
