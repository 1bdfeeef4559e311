"""CPU-only checks of tests/picker_refs.py: the two fp32 emulations of the documented picker arithmetic pass `check_picks` on every crafted
row and on random rows, the crafted rows are what they claim to be, and a picker with ONE defect is rejected (f64_bounds.check_near_miss's
idea: a checker that a near miss passes is too loose)."""
import math

import numpy as np
import pytest
import torch

from tests import picker_refs as P

CLASSES = [48, 200, 256, 321, 1000]
TEMPS = [0.25, 0.7, 1.0, 2.0]


def layouts(n):
    return ("general", "256") if n <= 256 else ("general",)


def draw_row(layout, row, n, temps=TEMPS, size=256, defect=None):
    """one crafted row drawn with its U_GRID at each temperature through an emulation -> the checker's verdicts, concatenated"""
    out = []
    for T in ([row["T"]] if row["T"] is not None else temps):
        u, on_step = P.U_GRID(row["logits"], n, row["temp_logit"], P.MIN_TEMP, T, size=size, extra=row["u_extra"])
        picks, fell = P.emulate_sampled(layout, row["logits"], n, row["temp_logit"], P.MIN_TEMP, T, u, defect=defect)
        r = P.check_picks_detail(row["logits"], n, row["temp_logit"], P.MIN_TEMP, torch.full((size,), T), u, picks)
        r.update(on_step=on_step, fell=fell, picks=picks, u=u)
        out.append(r)
    return {k: torch.cat([r[k] for r in out]) for k in out[0]}


@pytest.mark.parametrize("n", CLASSES)
def test_emulations_pass_the_checker_on_crafted_rows(n):
    for layout in layouts(n):
        for row in P.CRAFTED_ROWS(n):
            if row["kind"] != "sampled":
                want = P.picker_ref(row["logits"], n, row["temp_logit"], P.MIN_TEMP)
                if row["expect"] is not None:
                    assert want == row["expect"], (row["name"], want, row["expect"])
                assert P.emulate_greedy(layout if row["kind"] == "greedy" else "256", row["logits"], n, row["temp_logit"], P.MIN_TEMP) == want, \
                    (layout, row["name"])
                continue
            r = draw_row(layout, row, n)
            assert bool(r["hard"].all()), (layout, row["name"], "a class without mass was drawn")
            assert bool(r["ok"].all()), (layout, row["name"], float(r["miss"].max()), float(r["tol"].max()))
            assert float(r["tol"].max()) < 2e-5, (row["name"], float(r["tol"].max()))
            off = ~r["on_step"]
            print(f"[picker] {layout:7s} n={n:4d} {row['name']:18s} draws {r['ok'].numel():5d}  off-step inexact {float((~r['exact'][off]).float().mean()) * 100:6.3f} %"
                  f"  on-step inexact {float((~r['exact'][r['on_step']]).float().mean()) * 100:6.3f} %  largest miss {float(r['miss'].max()):.2e}"
                  f"  tol {float(r['tol'].max()):.2e}")
            if row["name"] == "fallback" and (layout == "256" or P.per_general(n) > 1):
                at_top = r["u"] == P.ONE_BELOW_1
                assert bool(r["fell"][at_top].all()), (layout, n, "the fallback row does not reach the fallback")


@pytest.mark.parametrize("n", CLASSES)
def test_emulations_pass_the_checker_on_random_rows(n):
    """logits randn * 2 and randn * 6 less their maximum (the classes that would fall into expf's denormal band moved down), T in [0.25, 1.75], with the sigmoid
    divisor, the min_temp divisor and none; random uniforms: the share of draws that need the tolerance is at most 1 %"""
    g = torch.Generator().manual_seed(n)
    inexact, count, worst, worst_tol = 0, 0, 0.0, 0.0
    for i in range(24):
        l = torch.randn(n, generator=g) * (2.0 if i % 2 else 6.0)
        l = P.clear_band(l - l.max())           # (the maximum at 0: the tolerance grows with |m|, two roundings of every quotient)
        tl = (P.TL_SIG, P.TL_MIN, None)[i % 3]
        T = float(0.25 + 1.5 * torch.rand(1, generator=g))
        u = torch.rand(400, generator=g).clamp(max=P.ONE_BELOW_1)
        for layout in layouts(n):
            picks, _ = P.emulate_sampled(layout, l, n, tl, P.MIN_TEMP, T, u)
            r = P.check_picks_detail(l, n, tl, P.MIN_TEMP, torch.full((400,), T), u, picks)
            assert bool(r["ok"].all()) and bool(r["hard"].all()), (layout, i, float(r["miss"].max()), float(r["tol"].max()))
            assert float(r["tol"].max()) < 2e-5
            inexact += int((~r["exact"]).sum())
            count += 400
            worst, worst_tol = max(worst, float(r["miss"].max())), max(worst_tol, float(r["tol"].max()))
    print(f"[picker] random rows n={n}: {inexact} of {count} draws need the tolerance ({inexact / count * 100:.4f} %; limit 1 %), largest miss {worst:.2e} "
          f"of the total, largest tolerance {worst_tol:.2e}")
    assert inexact <= 0.01 * count


def test_crafted_rows_are_what_they_claim():
    a, b, tl = P.find_near_tie()
    d0, dd = np.float32(P.MIN_TEMP), np.float32(P.denom32(tl, P.MIN_TEMP).item())
    assert np.float32(a) < np.float32(b) and np.nextafter(np.float32(a), np.float32(2)) == np.float32(b)
    assert np.float32(a) / d0 == np.float32(b) / d0 and np.float32(a) / dd < np.float32(b) / dd        # the collision, and its absence
    assert float(P.denom32(P.TL_MIN, P.MIN_TEMP)) == P.MIN_TEMP and float(P.denom32(P.TL_SIG, P.MIN_TEMP)) > P.MIN_TEMP
    nan_row = torch.tensor([0.0, math.nan, 5.0, math.nan])
    assert int(torch.argmax(nan_row)) == 1                      # torch.argmax: the first NaN
    for n in CLASSES + [64, 1024]:
        names = [r["name"] for r in P.CRAFTED_ROWS(n)]
        assert len(set(names)) == len(names)
        for want in ("flat", "one_hot_first", "one_hot_last", "straddle_lanes_0", "tail_masked", "head_masked", "underflow_tail", "random_wide",
                     "tie_first", "near_tie_collide", "near_tie_distinct", "nan_first_one", "nan_first_two"):
            assert want in names, (n, want)
        for row in P.CRAFTED_ROWS(n):
            assert row["logits"].shape == (n,)
            if row["kind"] == "sampled":                         # the precondition of check_picks at both ends of the temperatures
                for T in ([row["T"]] if row["T"] else [P.T_MIN, P.T_MAX]):
                    P.check_picks(row["logits"], n, row["temp_logit"], P.MIN_TEMP, torch.tensor([T]), torch.tensor([0.5]), torch.tensor([0]))
                    u, on = P.U_GRID(row["logits"], n, row["temp_logit"], P.MIN_TEMP, T, extra=row["u_extra"])
                    assert u.shape == (256,) and float(u[0]) == 0.0 and float(u[1]) == P.ONE_BELOW_1 and bool((~on).sum() >= 62)
                    assert bool(((u >= 0) & (u < 1)).all())


# ---- near misses: one defect each, rejected on the crafted rows ------------------------------------------------------------------------------
def rejected(layout, n, defect, names):
    bad = 0
    for row in P.CRAFTED_ROWS(n):
        if row["kind"] == "sampled" and row["name"] in names:
            r = draw_row(layout, row, n, defect=defect)
            bad += int((~r["ok"]).sum())
    return bad


def test_near_miss_no_guard():
    """(a) no `e > 0` guard: a class without mass is drawn where a lane starts above the lane before's last running sum"""
    for layout, n in (("general", 256), ("256", 256), ("256", 48), ("general", 321), ("general", 1000), ("general", 200)):
        names = [f"guard_{4 if layout == '256' else P.per_general(n)}"]
        assert rejected(layout, n, None, names) == 0
        assert rejected(layout, n, "no_guard", names) > 0, (layout, n)


def test_near_miss_dropped_row_carry():
    """(b) the carry of DPP row 2 dropped from the scan of the 256-class layout: row 2 (lanes 32 - 47) no longer receives the total of rows
    0 + 1 that the second row step hands it"""
    for n in (256, 200):
        for names in (["flat"], ["straddle_rows"], ["random_narrow"]):
            assert rejected("256", n, "drop_row2_carry", names) > 0, (n, names)


def test_near_miss_ge_instead_of_gt():
    """(c) `>=` instead of `>` against the target: only a row that rounds nothing (tolerance 0) can tell"""
    for layout in ("general", "256"):
        assert rejected(layout, 256, "ge", ["flat"]) > 0, layout
    assert rejected("general", 1000, "ge", ["straddle_rows", "straddle_lanes_0", "flat"]) > 0


def test_near_miss_greedy_rules():
    """(d) the last maximum instead of the first on ties; (e) argmax of the raw logits where the quotients collide"""
    for n in CLASSES:
        rows = {r["name"]: r for r in P.CRAFTED_ROWS(n)}
        for name, defect in (("tie_first", "last_max"), ("tie_first_ends", "last_max"), ("tie_random", "last_max"), ("near_tie_collide", "last_max"),
                             ("near_tie_collide", "raw_argmax")):
            row = rows[name]
            for layout in layouts(n):
                good = P.emulate_greedy(layout, row["logits"], n, row["temp_logit"], P.MIN_TEMP)
                pick = P.emulate_greedy(layout, row["logits"], n, row["temp_logit"], P.MIN_TEMP, defect=defect)
                ok, _ = P.check_picks(row["logits"], n, row["temp_logit"], P.MIN_TEMP, None, None, torch.tensor([good, pick]))
                assert bool(ok[0]) and not bool(ok[1]), (n, name, defect)
        # (and the raw argmax is RIGHT where the quotients stay distinct: the row pair tells the two rules apart)
        row = rows["near_tie_distinct"]
        assert P.emulate_greedy("general", row["logits"], n, row["temp_logit"], P.MIN_TEMP, defect="raw_argmax") == row["expect"]


def test_near_miss_fallback_takes_the_last_class():
    """(f) the fallback returning class n - 1 instead of the last class with mass"""
    for layout, n in (("general", 256), ("256", 256), ("256", 48), ("general", 321), ("general", 1000)):
        assert rejected(layout, n, "fallback_last_class", ["fallback"]) > 0, (layout, n)


def test_near_miss_per_off_by_one():
    """(g) an off-by-one in `per` at 321 classes (5 instead of 6 per lane: class 320 is never looked at, every lane boundary moves)"""
    for names in (["one_hot_last"], ["flat"], ["random_narrow"], ["straddle_lanes_0"]):
        assert rejected("general", 321, "per_off_by_one", names) > 0, names
