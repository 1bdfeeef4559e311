"""The class pickers against an exact reference: one row of head logits -> one class, greedy (torch.argmax's first-maximum rule on the fp32
quotients logits / denom) or by inverting the CDF of softmax(logits / denom / T) at a given uniform (modules/targets.py, DESIGN.md
"class pickers").  CPU only: the float64 reference, the crafted rows, the uniforms to draw with, the checker with its derived tolerance, and
two fp32 emulations of the documented arithmetic (a second reference, written from the comments of csrc/sampler256.h and csrc/kernels.hip -
never the thing under test).

Rows are built so that every logit is (as a quotient by denom * T, against the row's maximum) within 30 of the maximum, at least 200 below
it, or -inf: expf of the first is a normal number above 9e-14, of the other two exactly 0 - nothing lies in expf's denormal band
(-104 .. -87), where a kernel may or may not flush.  `check_picks` asserts that as a precondition.
"""
import math

import numpy as np
import torch

U = 2.0 ** -24            # fp32 unit roundoff (tests/f64_bounds.py)
C_PICK = 2.0              # the one constant of the tolerance below
MIN_TEMP = float(np.float32(0.9))     # the heads' min_temp in these tests: with a very negative temperature logit denom IS this fp32 number
TL_MIN = -30.0            # temperature logit whose sigmoid (1e-13) lies below min_temp whatever the sigmoid's last bit: denom = min_temp exactly
TL_SIG = 3.0              # temperature logit whose sigmoid (0.9526) decides: denom carries the kernel's fp32 sigmoid
T_MIN, T_MAX = 0.25, 2.0
LIVE_RAW = 6.0            # live classes lie within this of the row maximum: / (denom >= 0.9) / (T >= 0.25) <= 26.7 < 30
DEAD_RAW = -1000.0        # dead classes: / (denom < 1) / (T <= 2) <= -500 < -200
LIVE_D, DEAD_D = 30.0, 200.0
ONE_BELOW_1 = float(np.float32(1.0 - 2.0 ** -24))


def denom32(temp_logit, min_temp):
    """the divisor as torch forms it in fp32 (modules/mlp.py: maximum(sigmoid(t), min_temp)); 1 without a temperature column"""
    if temp_logit is None:
        return torch.tensor(1.0)
    return torch.maximum(torch.sigmoid(torch.tensor(temp_logit, dtype=torch.float32)), torch.tensor(min_temp, dtype=torch.float32))


def picker_ref(logits_f32, n_classes, temp_logit, min_temp, T=None, u=None):
    """Greedy (T None): argmax of the fp32 quotients l / denom, computed with torch on the CPU - what modules/targets.py and the oracle do; the
    first maximum wins (a NaN counts as the maximum).  Sampled: float64 on the fp32 inputs, denom = max(sigmoid(temp_logit), min_temp) or 1,
    v = (l / denom) / T, e = exp(v - max v) with the classes at least 200 below the maximum at exactly 0 (expf's result), the CDF and the
    total; returns a dict with the half-open interval [lo_k, hi_k) of every class (`lo`, `hi`), `e`, `v`, `d` = v - max v, `live`, `total`,
    and with `u` the `target` = u * total."""
    l32 = torch.as_tensor(logits_f32, dtype=torch.float32)[:n_classes]
    if T is None:
        q = l32 / denom32(temp_logit, min_temp) if temp_logit is not None else l32
        return int(torch.argmax(q))
    l = l32.double()
    den = 1.0
    if temp_logit is not None:
        tl = float(np.float32(temp_logit))
        den = max(1.0 / (1.0 + math.exp(-tl)), float(np.float32(min_temp)))
    v = (l / den) / float(T)
    d = v - v.max()
    live = d > -0.5 * (LIVE_D + DEAD_D)
    e = torch.where(live, torch.exp(d), torch.zeros_like(d))
    hi = torch.cumsum(e, 0)
    out = dict(lo=hi - e, hi=hi, e=e, v=v, d=d, live=live, total=hi[-1])
    if u is not None:
        out["target"] = torch.as_tensor(u, dtype=torch.float32).double() * hi[-1]
    return out


def per_general(n_classes):
    return (n_classes + 63) // 64


# ---- the tolerance -----------------------------------------------------------------------------------------------------------------------------
# A kernel forms, per class, v_c = fl(fl(l_c / denom) / T) (two roundings: |dv_c| <= 2 u |v_c|), the maximum m of those (|dm| <= 2 u |m|), the
# difference fl(v_c - m) (u |v_c - m|) and expf of it (within 2 ulp: 4 u, relative); where sigmoid(temp_logit) decides, denom itself is an fp32
# sigmoid, a few ulp off (6 u, which scales every v_c - m).  Term c is therefore off by the relative amount
#     eps_c = (2 |v_c| + 2 |m| + (1 + D) |v_c - m| + 4) u,     D = 6 with a temperature column, 0 without
# (for a row whose maximum is 0 this is the (3 |v_c - m| + 4) u of a plain reading), and a CDF step, as a fraction of the total, by at most the
# share-weighted sum of the eps_c.  The running sum a class is compared through is `per` sequential additions inside a lane on top of a scan
# of six additions (max(per, 4) + 6 in all: each u of the partial sum, at most the total), and the target u * total is rounded once more.
#     tol = C_PICK u (sum_c share_c (2 |v_c| + 2 |m| + (1 + D) |v_c - m| + 4) + max(per, 4) + 6 + 1)
# of the total; C_PICK = 2 covers the second-order terms and the total's own error entering both sides.  For the rows here (live classes within
# 30 of a maximum near 0) it is a few 1e-6: well below the 2e-5 that helpers.sampled_picks_ok needs against ORACLE logits.
#
# A row whose live classes all EQUAL the maximum leaves nothing to round: every exponent is exactly 0, every term exactly 1, every partial sum
# an integer below 2^24, the total the count of live classes.  The one fp32 operation left is the product u * total, which the reference then
# makes too: tolerance 0, half-open intervals - which is what tells `>` from `>=` against the target.
def check_picks_detail(logits_f32, n_classes, temp_logit, min_temp, T, u, picks):
    """One row of logits, R draws: T (R,) fp32 temperatures (None: greedy, then u is ignored), u (R,) fp32 uniforms, picks (R,).  Returns a
    dict: ok, exact, hard (bool (R,)), miss (distance of the target from the picked class's interval, as a fraction of the total), tol (R,)."""
    picks = torch.as_tensor(picks).long().reshape(-1)
    R = picks.numel()
    in_range = (picks >= 0) & (picks < n_classes)
    if T is None:
        want = picker_ref(logits_f32, n_classes, temp_logit, min_temp)
        same = picks == want
        return dict(ok=same, exact=same, hard=in_range, miss=(~same).double(), tol=torch.zeros(R, dtype=torch.float64))
    T = torch.as_tensor(T, dtype=torch.float32).reshape(-1).expand(R)
    u = torch.as_tensor(u, dtype=torch.float32).reshape(-1)
    assert u.numel() == R and bool(((u >= 0) & (u < 1)).all())
    l32 = torch.as_tensor(logits_f32, dtype=torch.float32)[:n_classes]
    assert not bool(torch.isnan(l32).any()), "NaN logits are defined on the greedy_256 path only"
    ok = torch.zeros(R, dtype=torch.bool)
    exact, hard = ok.clone(), ok.clone()
    miss, tol = torch.zeros(R, dtype=torch.float64), torch.zeros(R, dtype=torch.float64)
    k = picks.clamp(0, n_classes - 1)
    D = 6.0 if temp_logit is not None else 0.0
    depth = max(per_general(n_classes), 4) + 6
    for t in torch.unique(T):
        sel = T == t
        r = picker_ref(l32, n_classes, temp_logit, min_temp, float(t), u[sel])
        d, live = r["d"], r["live"]
        assert bool(((d >= -LIVE_D) | (d <= -DEAD_D)).all()), "a logit lies in the band between the live and the dead classes"
        total = r["total"]
        if bool((l32[live] == l32[live].max()).all()):      # nothing rounds but the product (above)
            target = (u[sel] * torch.tensor(float(total), dtype=torch.float32)).double()
            tol_t = 0.0
        else:
            target = r["target"]
            share = r["e"] / total
            vv = torch.where(live, r["v"].abs(), torch.zeros_like(d))
            dd = torch.where(live, d.abs(), torch.zeros_like(d))
            m = float(r["v"].max().abs())
            tol_t = C_PICK * U * (float((share * (2 * vv + 2 * m + (1 + D) * dd + 4)).sum()) + depth + 1)
        lo, hi = r["lo"][k[sel]], r["hi"][k[sel]]
        exact[sel] = (lo <= target) & (target < hi)
        ok[sel] = (lo - tol_t * total <= target) & (target < hi + tol_t * total)
        hard[sel] = in_range[sel] & live[k[sel]]
        miss[sel] = torch.maximum(torch.maximum(lo - target, target - hi), torch.zeros_like(lo)) / total
        tol[sel] = tol_t
    exact &= hard
    ok &= hard
    return dict(ok=ok, exact=exact, hard=hard, miss=miss, tol=tol)


def check_picks(logits_f32, n_classes, temp_logit, min_temp, T, u, picks):
    """(ok, exact) as helpers.sampled_picks_ok returns them, for exact logits: the tolerance is derived per row (above; 0 for a row that
    rounds nothing), the hard condition - a picked class exists and has mass - holds with no tolerance, greedy picks (T None) are compared
    exactly with `picker_ref`."""
    r = check_picks_detail(logits_f32, n_classes, temp_logit, min_temp, T, u, picks)
    return r["ok"], r["exact"]


# ---- crafted rows ---------------------------------------------------------------------------------------------------------------------------
def _f32(x):
    return float(np.float32(x))


def find_near_tie(min_temp=MIN_TEMP, start=0.95, tries=20000):
    """adjacent floats a < b above `start` whose fp32 quotients by min_temp COLLIDE, and a temperature logit whose sigmoid (> min_temp) keeps
    their quotients DISTINCT - for the divisor torch forms and for every fp32 number within 2 ulp of it (a kernel's sigmoid)"""
    d0 = np.float32(min_temp)
    tl = None
    for cand in (TL_SIG, 3.5, 4.0, 2.5):
        dd = np.float32(denom32(cand, min_temp).item())
        if dd > d0:
            tl = cand
            break
    assert tl is not None
    ds = [dd]
    for _ in range(2):
        ds = [np.nextafter(ds[0], np.float32(0))] + ds + [np.nextafter(ds[-1], np.float32(2))]
    a = np.float32(start)
    for _ in range(tries):
        b = np.nextafter(a, np.float32(2))
        if a / d0 == b / d0 and all(a / d < b / d for d in ds):
            return float(a), float(b), tl
        a = b
    raise AssertionError("no colliding pair found")


def _row(name, logits, temp_logit, kind="sampled", T=None, expect=None, u_extra=()):
    return dict(name=name, logits=torch.as_tensor(logits, dtype=torch.float32).clone(), temp_logit=temp_logit, kind=kind, T=T, expect=expect,
                u_extra=tuple(u_extra))


def clear_band(l, live_raw=LIVE_RAW):
    """logits further than `live_raw` below the row's maximum become dead classes (DEAD_RAW and below)"""
    l = torch.as_tensor(l, dtype=torch.float32).clone()
    m = l[torch.isfinite(l)].max()
    gone = torch.isfinite(l) & (l < m - live_raw)
    l[gone] = m + DEAD_RAW - (m - l[gone])
    return l


def boundaries(n):
    """(lane boundaries, DPP-row boundaries) of the two layouts: `per` classes per lane in the general loops, 4 in sample_256 (which pads a
    narrower head to 256 classes); rows of 16 lanes"""
    per = per_general(n)
    lanes = sorted({b for b in range(per, n, per)} | {b for b in range(4, n, 4)})
    rows = sorted({b for b in range(64, n, 64)} | {b for b in range(16 * per, n, 16 * per)})
    return lanes, rows


def _straddle(n, bs):
    l = torch.full((n,), DEAD_RAW)
    for b in bs:
        l[b - 1] = 0.0
        l[b] = 0.0
    return l


def CRAFTED_ROWS(n, seed=0):
    """named rows of `n` logits with a temperature-column value each (kind 'sampled', 'greedy' or 'greedy_nan'; T: the one temperature a row
    is built for, else any; expect: the greedy pick where the row is built around one)"""
    g = torch.Generator().manual_seed(1000 + n + seed)
    per = per_general(n)
    rows = [_row("flat", torch.zeros(n), TL_SIG)]
    last_lane = sorted({per * ((n - 1) // per), 4 * ((n - 1) // 4)})
    for tag, at in [("first", 0), ("last", n - 1)] + [(f"lastlane{c}", c) for c in last_lane]:
        l = torch.full((n,), -200.0 * T_MAX)
        l[at] = 0.0
        rows.append(_row(f"one_hot_{tag}", l, TL_MIN))
    lanes, drows = boundaries(n)
    if drows:
        rows.append(_row("straddle_rows", _straddle(n, drows), TL_SIG))
    rows.append(_row("straddle_lanes_0", _straddle(n, lanes[0::2]), TL_MIN))
    if len(lanes) > 1:
        rows.append(_row("straddle_lanes_1", _straddle(n, lanes[1::2]), TL_SIG))
    third = n // 3
    l = -(torch.randn(n, generator=g).abs() * 1.5).clamp(max=LIVE_RAW)
    l[int(torch.randint(0, n - third, (1,), generator=g))] = 0.0
    l[n - third:] = -math.inf
    rows.append(_row("tail_masked", l, TL_SIG))
    l = -(torch.randn(n, generator=g).abs() * 1.5).clamp(max=LIVE_RAW)
    l[third + int(torch.randint(0, n - third, (1,), generator=g))] = 0.0
    l[:third] = -math.inf
    rows.append(_row("head_masked", l, TL_MIN))
    l = torch.full((n,), DEAD_RAW)
    l[:5] = torch.tensor([0.0, -0.5, -1.0, -0.2, -2.0])
    rows.append(_row("underflow_tail", l, TL_SIG))
    l = torch.randn(n, generator=g) * 6
    rows.append(_row("random_wide", clear_band(l - l.max()), TL_SIG))
    l = torch.randn(n, generator=g)
    rows.append(_row("random_narrow", (l - l.max()).clamp(min=-LIVE_RAW), TL_MIN))
    # The `e > 0` guard of the pick.  `run` starts in every lane from incl - local, which need not be the lane before's last running sum: a
    # small class e_s in (2^-24, 2^-23) at the end of lane 0, then a dead class and the maximum (e = 1) in lane 1: incl_1 = fl(e_s + 1) =
    # 1 + 2^-23, so lane 1 starts from 2^-23 > e_s.  A target between the two (u = 0.9 * 2^-23) finds no class in lane 0, and in lane 1
    # first the dead class, whose running sum already exceeds it: only the guard keeps it from being drawn.  exp(-16.3) = 0.70 * 2^-23.
    # (T = 1 and denom = min_temp exactly; lanes of `p` classes.)
    for p in sorted({per, 4} - {1}):
        if p + 1 < n:
            l = torch.full((n,), DEAD_RAW)
            l[p - 1], l[p + 1] = -16.3 * MIN_TEMP, 0.0
            rows.append(_row(f"guard_{p}", l, TL_MIN, T=1.0, u_extra=(0.9 * 2.0 ** -23, 0.8 * 2.0 ** -23)))
    # The fallback (no running sum exceeds the target: the LAST class with mass).  The maximum in lane 0, two classes of e = 0.37 * 2^-23
    # (exp(-16.95)) side by side in a later lane: its incl = fl(1 + 0.73 * 2^-23) = 1 + 2^-23 is the total, but its lane starts from
    # fl(incl - local) = 1 and adds 0.37 * 2^-23 twice without ever leaving 1.  At u = 1 - 2^-24 the target rounds to 1: nothing exceeds it.
    s = 4 * per // math.gcd(4, per)
    if per > 1 or n <= 256:
        if s + 1 < n - 1:
            l = torch.full((n,), DEAD_RAW)
            l[0], l[s], l[s + 1] = 0.0, -16.95 * MIN_TEMP, -16.95 * MIN_TEMP
            rows.append(_row("fallback", l, TL_MIN, T=1.0))
    # ---- greedy
    l = torch.full((n,), -1.0)
    i1 = n // 3
    l[i1], l[i1 + 1], l[n - 1] = -0.0, 0.0, 0.0
    rows.append(_row("tie_first", l, TL_SIG, kind="greedy", expect=i1))
    l = torch.full((n,), -1.0)
    l[0], l[n - 1] = 2.5, 2.5
    rows.append(_row("tie_first_ends", l, TL_MIN, kind="greedy", expect=0))
    l = torch.randn(n, generator=g) * 2
    l[n // 2:] = l[:n - n // 2].clone()
    rows.append(_row("tie_random", l, TL_SIG, kind="greedy", expect=int(torch.argmax(l))))
    a, b, tl_distinct = find_near_tie()
    ia, ib = 5 % n, n - 2
    l = torch.full((n,), 0.5)
    l[ia], l[ib] = a, b
    rows.append(_row("near_tie_collide", l, TL_MIN, kind="greedy", expect=ia))
    rows.append(_row("near_tie_distinct", l, tl_distinct, kind="greedy", expect=ib))
    l = torch.full((n,), 0.5)
    l[ia], l[ib] = b, a
    rows.append(_row("near_tie_collide_rev", l, TL_MIN, kind="greedy", expect=ia))
    j = n // 2 + 1
    l = torch.randn(n, generator=g)
    l[j], l[3] = math.nan, 7.0
    rows.append(_row("nan_first_one", l, TL_SIG, kind="greedy_nan", expect=j))
    l = torch.randn(n, generator=g)
    l[6], l[j], l[(6 + j) // 2] = math.nan, math.nan, 9.0
    rows.append(_row("nan_first_two", l, TL_MIN, kind="greedy_nan", expect=6))
    return rows


def U_GRID(logits_f32, n_classes, temp_logit, min_temp, T, size=256, seed=0, extra=()):
    """the uniforms to draw one row with at temperature T: 0, 1 - 2^-24, for the CDF steps of the row the two fp32 numbers nearest to
    step / total from below and from above (after the row's own `extra` uniforms) (all of them while they fill at most 3/4 of `size`, else evenly spaced ones with the first and the
    last), random uniforms for the rest.  Returns (u (size,) fp32, on_step (size,) bool: the entries that sit on a step on purpose)."""
    r = picker_ref(logits_f32, n_classes, temp_logit, min_temp, T)
    steps = (r["hi"][r["live"]] / r["total"]).numpy()
    cap = max((size * 3 // 4 - 2) // 2, 1)
    if len(steps) > cap:
        steps = steps[np.unique(np.round(np.linspace(0, len(steps) - 1, cap)).astype(np.int64))]
    pts = [0.0, ONE_BELOW_1] + [float(x) for x in extra]
    for s in steps:
        f = np.float32(s)
        lo, hi = (f, np.nextafter(f, np.float32(2))) if float(f) <= s else (np.nextafter(f, np.float32(-1)), f)
        pts += [float(lo), float(hi)]
    pts = np.clip(np.asarray(pts, dtype=np.float32), 0.0, np.float32(ONE_BELOW_1))[:size]
    g = torch.Generator().manual_seed(7000 + seed)
    rnd = torch.rand(size - len(pts), generator=g)
    u = torch.cat([torch.from_numpy(pts), rnd]).float().clamp(max=ONE_BELOW_1)
    on_step = torch.zeros(size, dtype=torch.bool)
    on_step[:len(pts)] = True
    return u, on_step


# ---- fp32 emulations of the documented arithmetic -------------------------------------------------------------------------------------------
def _scan_hillis_steele(local):
    inc = local.clone()
    for o in (1, 2, 4, 8, 16, 32):
        nxt = inc.clone()
        nxt[o:] = inc[o:] + inc[:-o]
        inc = nxt
    return inc


def _scan_rows(local, defect=None):
    """Kogge-Stone inside the rows of 16 lanes, then the rows' totals: row 0's into row 1 and row 2's into row 3, then row 1's (now rows
    0 + 1) into rows 2 and 3"""
    x = local.clone().view(4, 16)
    for o in (1, 2, 4, 8):
        nxt = x.clone()
        nxt[:, o:] = x[:, o:] + x[:, :-o]
        x = nxt
    nxt = x.clone()
    nxt[1] = x[1] + x[0, 15]
    nxt[3] = x[3] + x[2, 15]
    x = nxt
    nxt = x.clone()
    if defect != "drop_row2_carry":
        nxt[2] = x[2] + x[1, 15]
    nxt[3] = x[3] + x[1, 15]
    return nxt.reshape(64)


def emulate_sampled(layout, logits_f32, n_classes, temp_logit, min_temp, T, u, defect=None):
    """layout 'general': lane i owns classes [i per, (i + 1) per), per = ceil(n / 64), Hillis-Steele scan (csrc/kernels.hip and the general
    loops of the step kernels); layout '256': the row padded to 256 classes with -inf, 4 classes per lane, the scan through the DPP rows
    (csrc/sampler256.h).  One row, one temperature, u (R,).  Returns (picks (R,), fell_back (R,)).  defect: None, 'no_guard', 'ge',
    'drop_row2_carry' (layout 256), 'fallback_last_class', 'per_off_by_one'."""
    n = n_classes
    l = torch.as_tensor(logits_f32, dtype=torch.float32)[:n]
    if layout == "256":
        assert n <= 256
        per = 4
    else:
        per = per_general(n) - (1 if defect == "per_off_by_one" else 0)
    slots = 64 * per
    v = l / denom32(temp_logit, min_temp) if temp_logit is not None else l.clone()
    v = v / torch.tensor(float(T), dtype=torch.float32)
    pad = torch.full((max(slots, n),), -math.inf)
    pad[:n] = v
    pad = pad[:slots]                              # (per_off_by_one: the classes past 64 per are never looked at)
    valid = torch.arange(slots) < n
    e = torch.exp(pad - pad.max())
    E = e.view(64, per)
    local = torch.zeros(64)
    for q in range(per):
        local = local + E[:, q]
    inc = _scan_rows(local, defect) if layout == "256" else _scan_hillis_steele(local)
    total = inc[63]
    run = inc - local
    runs = torch.empty(64, per)
    for q in range(per):
        run = run + E[:, q]
        runs[:, q] = run
    runs = runs.reshape(-1)
    target = torch.as_tensor(u, dtype=torch.float32).reshape(-1) * total
    mass = (e > 0) & valid
    over = (runs[None, :] >= target[:, None]) if defect == "ge" else (runs[None, :] > target[:, None])
    over = over & (valid if defect == "no_guard" else mass)[None, :]
    found = over.any(1)
    first = torch.argmax(over.int(), 1)
    if defect == "fallback_last_class":
        last = n - 1
    else:
        last = int(mass.nonzero().max()) if bool(mass.any()) else 0
    return torch.where(found, first, torch.full_like(first, last)), ~found


def emulate_greedy(layout, logits_f32, n_classes, temp_logit, min_temp, defect=None):
    """'general': the fp32 quotients, the first maximum.  '256': greedy_256 as csrc/sampler256.h documents it - the first maximum of the RAW
    logits, unless another logit lies within 4 ulp of it (then the quotients are formed and compared); a NaN logit: the first one.
    defect: None, 'last_max', 'raw_argmax'."""
    n = n_classes
    l = torch.as_tensor(logits_f32, dtype=torch.float32)[:n]
    den = denom32(temp_logit, min_temp)

    def arg(x):
        m = x.max()
        hit = (x == m).nonzero().reshape(-1)
        return int(hit[-1] if defect == "last_max" else hit[0])

    if defect == "raw_argmax":
        return arg(l)
    if layout == "general":
        return arg(l / den if temp_logit is not None else l)
    nan = torch.isnan(l)
    if bool(nan.any()):
        return int(nan.nonzero()[0])
    m = l.max()
    lim = m - torch.maximum(m.abs() * torch.tensor(4.8e-7), torch.tensor(1e-37))
    near = (l != m) & (l >= lim)
    if temp_logit is not None and bool(near.any()):
        return arg(l / den)
    return arg(l)
