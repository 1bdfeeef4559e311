"""The spline and onset-cut kernels on the MI355X (csrc/samplify.hip, include/mmk_samplify.h) against tests/samplify_refs.py: the spline
inside its derived bound of scipy's interp1d(kind="quadratic") at every size where the solve or the evaluation takes another path; the
period and cut kernels bit for bit against the numpy restatement fed the DEVICE's own materialised curves (every kernel evaluates a
sample through the same device function, so the comparison is exact); Samplifyer.fit against tests/golden/samplify.npz where the
recorded cuts are robust; Interpolate(mode="quadratic"); and the stream contract by the method of tests/stream_cases.py.  Each test
prints its worst error / bound."""
import numpy as np
import pytest
import torch

import mimikit_amd as mmk
from mimikit_amd import native
from tests import samplify_refs as R
from tests import stream_cases as S
from tests.f64_bounds import check_written
from tests.strided_inputs import FLOAT_SURROUNDS, Strided, surround_rule

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

G = R.golden()
TILE, HALO, ETILE, PTILE, GROUP = native.SPLINE2_TILE, native.SPLINE2_HALO, native.SPLINE2_EVAL_TILE, native.PERIODS_TILE, native.SAMPLIFY_GROUP


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def dev(a, device):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device)


def worst(got, want, bound):
    return float(np.max(np.abs(np.asarray(got, dtype=np.float64) - want) / bound))


# ------------------------------------------------------------------------------------------------------------------------ the spline
# the overlapping special rows, a knot tile and its halo +- 1, several tiles
SPLINE_N = (3, 4, 5, 6, 7, TILE - 1, TILE, TILE + 1, TILE + HALO - 1, TILE + HALO, TILE + HALO + 1, 2 * TILE + HALO + 3)


@pytest.mark.parametrize("n", SPLINE_N)
def test_spline_inside_the_bound_of_scipy(device, n):
    rng = np.random.default_rng(100 + n)
    wide = np.zeros((2, n + 7), dtype=np.float32)
    wide[0, :n] = rng.uniform(-1, 1, n)
    wide[1, :n] = np.cumsum(rng.uniform(-1, 1, n)) * 3.0                         # two rows of different content and size
    x = dev(wide, device)[:, :n]                                                # a strided view: rows n + 7 apart
    assert x.stride(0) == n + 7
    coef = native.spline2_coef(x)
    assert coef.dtype == torch.float64 and coef.shape == (2, n)
    ratio = 0.0
    for n_out in sorted({1, n - 1, n, ETILE - 1, ETILE, ETILE + 1, 3 * ETILE + 5}):
        got = native.spline2_eval(coef, n_out).cpu().numpy()
        want, bound = R.spline_ref(wide[:, :n], n_out)
        assert got.shape == (2, n_out) and got.dtype == np.float32
        bad = ~(np.abs(got.astype(np.float64) - want) <= bound)
        assert not bad.any(), (n, n_out, np.argwhere(bad)[:3].tolist())
        ratio = max(ratio, worst(got, want, bound))
        for r in range(2):                                                      # a single-row call gives the batched call's bits
            c1 = native.spline2_coef(dev(wide[r, :n].copy(), device))
            assert torch.equal(c1, coef[r]), (n, r)
            assert np.array_equal(bits(native.spline2_eval(c1, n_out).cpu().numpy()), bits(got[r])), (n, n_out, r)
    print(f"spline n={n}: worst error / bound {ratio:.3f}")


@surround_rule(*FLOAT_SURROUNDS)
def coef_call(x_np, device):
    """mmk_spline2_coef_f64 on strided, misaligned float32 rows into a NaN-surrounded float64 view (rows n + 5 apart, 16 bytes in)"""
    rows, n = x_np.shape
    x, coef = Strided.of(x_np, 1, device), Strided((rows, n), 2, device, float("nan"), torch.float64, row_stride=n + 5, tail=2)
    native.check(native.lib().mmk_spline2_coef_f64(x.ptr, x.stride, rows, n, coef.ptr, coef.stride, native.stream_ptr(device)), "mmk_spline2_coef_f64")
    check_written(coef.buf, coef.mask(), "spline2_coef")
    return coef.view.clone()


@surround_rule(*FLOAT_SURROUNDS)
def eval_call(coef_np, n_out, device):
    """mmk_spline2_eval_f32 on strided float64 coefficients into a NaN-surrounded view (rows n_out + 3 apart, 4 bytes in)"""
    rows, n = coef_np.shape
    coef = Strided.of(coef_np, 2, device, row_stride=n + 5, tail=2)
    out = Strided((rows, n_out), 1, device, float("nan"), row_stride=n_out + 3, tail=1)
    native.check(native.lib().mmk_spline2_eval_f32(coef.ptr, coef.stride, rows, n, out.ptr, out.stride, n_out, native.stream_ptr(device)), "mmk_spline2_eval_f32")
    check_written(out.buf, out.mask(), "spline2_eval")
    return out.view.clone()


def test_spline_entry_points_write_their_outputs_only(device):
    n, n_out = TILE + 3, ETILE + 9
    x = torch.rand(2, n) - 0.5
    coef = coef_call(x.numpy(), device)
    assert torch.equal(coef, native.spline2_coef(x.to(device)))
    assert torch.equal(eval_call(coef.cpu().numpy(), n_out, device), native.spline2_eval(coef.contiguous(), n_out))
    print("spline entry points: worst error / bound 0.000 (exact)")


def test_interpolate_quadratic_and_the_modes_that_still_raise(device):
    x = np.random.default_rng(3).uniform(-1, 1, (3, 37)).astype(np.float32)
    got = mmk.Interpolate(mode="quadratic", length=100)(dev(x, device)).cpu().numpy()
    want, bound = R.spline_ref(x, 100)
    assert got.shape == (3, 100) and not (~(np.abs(got.astype(np.float64) - want) <= bound)).any()
    got1 = mmk.Interpolate(mode="quadratic", factor=3)(dev(x[0].copy(), device)).cpu().numpy()
    want1, bound1 = R.spline_ref(x[0], 111)
    assert got1.shape == (111,) and not (~(np.abs(got1.astype(np.float64) - want1) <= bound1)).any()
    for miss in R.NEAR_MISSES:
        assert (~(np.abs(R.near_miss(x[0], 111, miss) - want1) <= bound1)).any(), miss
    with pytest.raises(NotImplementedError, match="cubic"):
        mmk.Interpolate(mode="cubic", length=4)(dev(x, device))
    with pytest.raises(NotImplementedError, match="axis=0"):
        mmk.Interpolate(mode="quadratic", axis=0, length=4)(dev(x, device))
    with pytest.raises(ValueError, match="n >= 3"):
        mmk.Interpolate(mode="quadratic", length=4)(dev(x[:, :2].copy(), device))
    print(f"Interpolate quadratic: worst error / bound {worst(got, want, bound):.3f}")


# ----------------------------------------------------------------------------------------------------------------------- the periods
T3 = 2 * PTILE + 300          # three tiles, the last one partial


def period_rows():
    """name -> (knots (n,), T): rows whose materialised gradient holds the listed feature"""
    rng = np.random.default_rng(17)
    rows = {}
    rows["no_attack"] = (np.linspace(0.1, 1.0, T3).astype(np.float32), T3)
    one = np.ones(T3, dtype=np.float32)
    one[:700] = -1.0
    rows["one_attack_no_peak"] = (one, T3)
    zero = np.ones(T3, dtype=np.float32)
    zero[:500], zero[500:600] = -1.0, 0.0                                       # 100 knots of exact 0: the coefficients in the middle are 0 too
    rows["exact_zero"] = (zero, T3)
    alt = np.where(np.arange(T3) % 2 == 0, -1.0, 1.0).astype(np.float32)        # an attack at every odd sample: on both sides of both tile boundaries
    rows["boundary"] = (alt, T3)
    late = np.ones(T3, dtype=np.float32)
    late[:100], late[PTILE + 500:] = -1.0, -1.0                                 # attack in tile 0, its peak in tile 1
    late[2 * PTILE + 50:2 * PTILE + 60] = 1.0
    rows["late_peak"] = (late, T3)
    rows["smooth"] = (np.cumsum(rng.uniform(-1, 1, 90)).astype(np.float32), 3 * PTILE + 17)        # 90 knots at 3089 positions
    return rows


PERIOD_ROWS = period_rows()


@pytest.mark.parametrize("name", tuple(PERIOD_ROWS))
def test_periods_equal_the_restatement_on_the_materialised_gradient(device, name):
    knots, T = PERIOD_ROWS[name]
    coef = native.spline2_coef(dev(knots, device))
    g = native.spline2_eval(coef, T).cpu().numpy()
    want_att, want_dec = R.attack_decay(g)
    att, dec, peaks = native.periods(coef, T)
    assert att.dtype == dec.dtype == torch.int64
    assert np.array_equal(att.cpu().numpy(), want_att) and np.array_equal(dec.cpu().numpy(), want_dec), name
    want_peaks = np.nonzero((g[:-1] > 0) & (g[1:] < 0))[0]
    assert np.array_equal(peaks.cpu().numpy(), want_peaks)
    # the same row taken as it is
    p = mmk.Periods().fit(dev(g, device))
    assert np.array_equal(p.att_i.cpu().numpy(), want_att) and np.array_equal(p.dec_i.cpu().numpy(), want_dec)
    a2, d2 = mmk.attack_decay(dev(g, device))
    assert torch.equal(a2, p.att_i) and torch.equal(d2, p.dec_i)
    if name == "no_attack":
        assert want_att.size == 0
    if name == "one_attack_no_peak":
        assert want_att.tolist() == [700] and want_dec.tolist() == [T - 1]
    if name == "exact_zero":               # (the coefficients, and with them the values, are exactly 0 a halo inside the run of zero knots)
        assert (g[540:560] == 0).all() and (g[:480] < 0).all() and (g[620:] > 0).all() and not ((want_att >= 540) & (want_att <= 620)).any()
        raw = np.array([-1, 0, 1, 1, -1, 1, -1, -0.0, 2, -3, 3], dtype=np.float32)          # an exact 0 between - and +: no attack at 2 or 8
        ra, rd = mmk.attack_decay(dev(raw, device))
        assert ra.tolist() == [5, 10] == R.attack_decay(raw)[0].tolist() and rd.tolist() == [5, 10] == R.attack_decay(raw)[1].tolist()
    if name == "boundary":
        for edge in (PTILE, 2 * PTILE):
            assert {edge - 1, edge + 1} <= set(want_att.tolist())
        assert want_att.size == T // 2 and (want_dec[:-1] == want_att[:-1]).all() and want_dec[-1] == T - 1      # (a peak at the attack itself)
    if name == "late_peak":
        assert want_att[0] == 100 and want_dec[0] == PTILE + 499 and want_dec[0] // PTILE > want_att[0] // PTILE
    print(f"periods {name}: {want_att.size} attacks, worst error / bound 0.000 (exact)")


# -------------------------------------------------------------------------------------------------------------------------- the cuts
def make_levels(device, frames):
    """frames: per level (env knots, grad knots) -> (env coefs, grad coefs) on the device"""
    coefs = [native.spline2_coef(dev(np.stack([e, g]).astype(np.float32), device)) for e, g in frames]
    return [c[0] for c in coefs], [c[1] for c in coefs]


def materialise(ec, gc, T):
    return [native.spline2_eval(c, T).cpu().numpy() for c in ec], [native.spline2_eval(c, T).cpu().numpy() for c in gc]


def check_cuts(device, y, frames, cc, cp, what):
    T = y.shape[0]
    ec, gc = make_levels(device, frames)
    envs, grads = materialise(ec, gc, T)
    want = R.cuts_ref(y, envs, grads, cc, cp)
    sides, lr, cuts = native.samplify_cuts(dev(y, device), ec, gc, dev(np.asarray(cc, dtype=np.int64), device), dev(np.asarray(cp, dtype=np.int64), device))
    assert np.array_equal(sides.cpu().numpy(), want["sides"]), (what, sides.tolist(), want["sides"].tolist())
    assert np.array_equal(bits(lr.cpu().numpy()), bits(want["lr"])), what
    assert np.array_equal(cuts.cpu().numpy(), want["cuts"]), (what, cuts.tolist(), want["cuts"].tolist())
    return want, envs, grads


CT = 6000


def hand_frames(rng, equal_ends=False, falling=False):
    e0 = np.abs(np.cumsum(rng.uniform(-1, 1, 40))) / 8 + 0.1
    e1 = np.linspace(2.0, 0.5, 80) if falling else np.abs(np.cumsum(rng.uniform(-1, 1, 80))) / 8 + 0.1
    e2 = np.abs(np.cumsum(rng.uniform(-1, 1, 160))) / 8 + 0.1
    g1 = np.zeros(80) if falling else rng.uniform(-1, 1, 80)
    frames = [(e0, rng.uniform(-1, 1, 40)), (e1, g1), (e2, rng.uniform(-1, 1, 160))]
    if equal_ends:
        frames[2] = (e0, rng.uniform(-1, 1, 40))
    return frames


def test_cuts_hand_built_cases_equal_the_restatement(device):
    rng = np.random.default_rng(23)
    y = rng.uniform(-1, 1, CT).astype(np.float32)
    y[5000:] = np.abs(y[5000:]) + 0.01                                          # no crossing to the right of the last cuts
    y[4999] = -0.5
    # a cut at sample 0; peak - cut of 1, 2000, 2001; ranges longer than GROUP; cuts whose walk to the right leaves the signal
    cc = [0, 100, 1000, 1000, 2500, 5600, 5990, 5998]
    cp = [50, 101, 3000, 3001, 2500 + GROUP + 1, 5999, 5999, 5999]
    want, _, _ = check_cuts(device, y, hand_frames(rng), cc, cp, "random levels")
    assert want["lr"][0, 0] == -np.inf and want["windows"].tolist()[1:4] == [1, 2000, 2000]
    assert (want["sides"] == 1).any() and set(want["cuts"][-3:].tolist()) <= set(range(0, 5001))
    # equal left and right scores: the finest level is the coarse one, every difference is 0
    want, _, _ = check_cuts(device, y, hand_frames(rng, equal_ends=True), cc, cp, "equal ends")
    assert (want["lr"][1:] == 0).all() and (want["sides"][1:] == 0).all() and want["sides"][0] == 1      # (-inf on the left of sample 0)
    z = R.zero_crossings(y)
    assert want["cuts"].tolist()[1:] == [R.snap(c, z) for c in cc[1:]]          # (left-side cuts are only snapped)
    # a range that collapses at the second level: a falling envelope with a flat gradient has its argmin last and its argmax first
    frames = hand_frames(rng, falling=True)
    frames[0] = (np.linspace(1.0, 3.0, 40), frames[0][1])                       # coarse above fine on the right: side 1
    frames[2] = (np.linspace(1.0, 0.1, 160), frames[2][1])
    want, envs, grads = check_cuts(device, y, frames, [1000, 2000], [1900, 2000 + 3 * GROUP], "collapse")
    assert (want["sides"] == 1).all()
    c, d, _ = R.refine_step(1000, 1900, envs[1], grads[1])
    assert c == d == 1899
    # y all positive: only z[0]
    ones = np.full(CT, 0.25, dtype=np.float32)
    want, _, _ = check_cuts(device, ones, hand_frames(rng), cc, cp, "all positive")
    assert (want["cuts"] == 0).all()
    # one level: nothing to refine, both scores 0 where the windows are not empty
    e0 = hand_frames(rng)[:1]
    want, _, _ = check_cuts(device, y, e0, cc, cp, "one level")
    assert (want["sides"][1:] == 0).all() and want["sides"][0] == 1
    # pairs outside 0 <= cut <= peak <= T - 1 are refused in the kernel
    ec, gc = make_levels(device, hand_frames(rng))
    sides, lr, cuts = native.samplify_cuts(dev(y, device), ec, gc, dev(np.array([5, -1, 10, 0]), device), dev(np.array([4, 3, CT, CT - 1]), device))
    assert sides.tolist()[:3] == [-1, -1, -1] and cuts.tolist()[:3] == [-1, -1, -1] and sides.tolist()[3] in (0, 1)
    assert torch.isnan(lr[:3]).all() and not torch.isnan(lr[3]).any()
    print("cuts hand-built: worst error / bound 0.000 (exact)")


def fitted(device, name):
    levels = [dict(n_fft=n, overlap=o, grad_max_lag=g) for n, o, g in R.LEVELS]
    s = mmk.Samplifyer(sensitivity=float(G[f"{name}_sensitivity"]), levels_def=levels)
    y = dev(G[f"{name}_y"], device)
    return s, y


@pytest.mark.parametrize("name", tuple(R.FIXTURES))
def test_fit_equals_the_restatement_on_its_own_curves(device, name):
    s, y = fitted(device, name)
    s.fit(y)
    envs = [s.coarse_env.cpu().numpy()] + [e.cpu().numpy() for e in s.fine_envs]
    grads = [lv.grad.cpu().numpy() for lv in s.levels]
    assert np.array_equal(bits(grads[0]), bits(s.coarse_grad.cpu().numpy())) and all(e.shape == (y.shape[0],) for e in envs + grads)
    want = R.fit_ref(G[f"{name}_y"], envs, grads, float(G[f"{name}_sensitivity"]))
    att, dec, _ = native.periods(s.levels[0].grad_coef, s.T)
    assert np.array_equal(att.cpu().numpy(), want["att"]) and np.array_equal(dec.cpu().numpy(), want["dec"])
    for key in ("coarse_cuts", "coarse_peaks", "sides", "cuts", "windows"):
        assert np.array_equal(getattr(s, key).cpu().numpy(), want[key]), key
        assert getattr(s, key).dtype == torch.int64
    assert np.array_equal(bits(s.scores.cpu().numpy()), bits(want["scores"])) and s.scores.dtype == torch.float32
    assert np.array_equal(bits(s.left_right_scores.cpu().numpy()), bits(want["lr"]))
    n = len(want["cuts"])
    ce = envs[0]
    assert sorted(s.mins_rank.tolist()) == sorted(s.maxs_rank.tolist()) == list(range(n))
    order = np.empty(n, dtype=np.int64)
    order[s.mins_rank.cpu().numpy()] = np.arange(n)
    assert (np.diff(ce[want["coarse_cuts"]][order]) >= 0).all()
    order[s.maxs_rank.cpu().numpy()] = np.arange(n)
    assert (np.diff(ce[want["coarse_peaks"]][order]) <= 0).all()
    print(f"fit {name}: {n} cuts of {len(want['att'])} attacks, worst error / bound 0.000 (exact)")


@pytest.mark.parametrize("name", tuple(R.FIXTURES))
def test_fit_against_the_golden_file(device, name):
    """the golden curves come from a float64 transform and scipy: the lists agree where the recorded decisions are robust (three quarters of
    the cuts at least), the scores inside the recorded bound"""
    s, y = fitted(device, name)
    labels = s(y)
    g = {k: G[f"{name}_{k}"] for k in R.GOLDEN_KEYS}
    cc = s.coarse_cuts.cpu().numpy()
    assert len(cc) == len(g["coarse_cuts"]), (len(cc), len(g["coarse_cuts"]))
    robust = g["robust"]
    assert 4 * int(robust.sum()) >= 3 * len(robust)
    for key in ("coarse_cuts", "coarse_peaks", "sides", "cuts", "windows"):
        got = getattr(s, key).cpu().numpy()
        assert np.array_equal(got[robust], g[key][robust]), (key, got.tolist(), g[key].tolist())
    scores = s.scores.cpu().numpy()
    same = (cc == g["coarse_cuts"]) & (s.coarse_peaks.cpu().numpy() == g["coarse_peaks"])
    err = np.abs(scores.astype(np.float64) - g["scores"])[same]
    bound = (g["score_bound"] + R.U * np.abs(g["scores"]))[same]
    assert err.size >= int(robust.sum()) and (err <= bound).all(), (err / bound).max()
    want_labels = torch.zeros(y.shape[0], dtype=torch.int64, device=y.device)
    want_labels[s.cuts] = 1
    assert labels.dtype == torch.int64 and torch.equal(labels, torch.cumsum(want_labels, 0)) and int(labels[-1]) == len(set(s.cuts.tolist()))
    for t in (s.scores, s.left_right_scores, s.coarse_env, s.coarse_grad, *s.fine_envs):
        assert not torch.isnan(t).any()
    pieces = s.export_as_list()
    assert len(pieces) == len(cc) + 1 and pieces[0].shape[0] == int(s.cuts[0])
    assert s.export_with_silence(0.01, 16000).shape[0] == sum(p.shape[0] for p in pieces) + 160 * len(pieces)
    n_same = int((s.cuts.cpu().numpy() == g["cuts"]).sum())
    print(f"golden {name}: {len(cc)} cuts, {int(robust.sum())} robust, {n_same} equal; scores worst error / bound {float((err / bound).max()):.3f}")


def test_fit_costs_two_host_synchronisations(device):
    import warnings
    s, y = fitted(device, "bursts")
    s.fit(y)                                                                    # (the tables of the first spectral call are built)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("warn")
    try:
        with warnings.catch_warnings(record=True) as caught:
            warnings.simplefilter("always")
            s.fit(y)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    waits = [str(w.message) for w in caught if "synchroniz" in str(w.message)]
    assert len(waits) == 2, waits
    print("fit: two waits (the counts, the kept), worst error / bound 0.000")


# ------------------------------------------------------------------------------------------------------------------ the stream contract
SN, ST = 300, 3 * PTILE + 100          # knots (two coefficient tiles), samples (four period tiles)
SK = 24                                # attacks / cuts of the score and cut cases


def _smooth(g, n, scale=1.0):
    return torch.cumsum(S.uni(g, n), 0).double() * scale


def _stream_coef():
    return S.Case("mmk_spline2_coef_f64", lambda seed: dict(x=S.uni(S.gen(seed), 2, SN)), lambda L, i: dict(coef=((2, SN), torch.float64)),
                  lambda L, a, s: L.mmk_spline2_coef_f64(S.P(a["x"]), SN, 2, SN, S.P(a["coef"]), SN, s))


def _stream_eval():
    return S.Case("mmk_spline2_eval_f32", lambda seed: dict(coef=S.uni(S.gen(seed), 2, SN).double()), lambda L, i: dict(out=((2, ST), torch.float32)),
                  lambda L, a, s: L.mmk_spline2_eval_f32(S.P(a["coef"]), SN, 2, SN, S.P(a["out"]), ST, ST, s))


def _periods_work(L, i):
    return dict(work=L.mmk_periods_workspace_bytes(ST))


def _stream_periods_count():
    def call(L, a, s):
        return L.mmk_periods_count_i64(S.P(a["coef"]), SN, None, ST, S.P(a["counts"]), S.P(a["work"]), a["work"].numel(), s)
    return S.Case("mmk_periods_count_i64", lambda seed: dict(coef=S.uni(S.gen(seed), SN).double()), lambda L, i: dict(counts=((2,), torch.int64)), call,
                  work=_periods_work)


def _stream_periods_fill():
    cap = ST // 2                      # room for any count: an index past the stated counts is not written, and the sentinels stay

    def call(L, a, s):
        rc = L.mmk_periods_count_i64(S.P(a["coef"]), SN, None, ST, S.P(a["counts"]), S.P(a["work"]), a["work"].numel(), s)
        return rc or L.mmk_periods_fill_i64(S.P(a["coef"]), SN, None, ST, S.P(a["work"]), a["work"].numel(), cap, cap, S.P(a["att"]), S.P(a["dec"]),
                                            S.P(a["peaks"]), s)
    outs = lambda L, i: dict(counts=((2,), torch.int64), att=((cap,), torch.int64), dec=((cap,), torch.int64), peaks=((cap,), torch.int64))      # noqa: E731
    return S.Case("mmk_periods_fill_i64", lambda seed: dict(coef=S.uni(S.gen(seed), SN).double()), outs, call, work=_periods_work)


def _stream_scores():
    def build(seed):
        g = S.gen(seed)
        att = torch.sort(torch.randperm(ST - 1, generator=S.gen(5))[:SK])[0]      # (the lists stay, the curve is late)
        return dict(coef=S.uni(g, SN).double(), att=att, dec=torch.clamp(att + 37, max=ST - 1))

    def call(L, a, s):
        return L.mmk_samplify_scores_f32(S.P(a["coef"]), SN, ST, S.P(a["att"]), S.P(a["dec"]), SK, 0.0, S.P(a["scores"]), S.P(a["ea"]), S.P(a["ed"]),
                                         S.P(a["keep"]), s)
    outs = lambda L, i: dict(scores=((SK,), torch.float32), ea=((SK,), torch.float32), ed=((SK,), torch.float32), keep=((SK,), torch.uint8))      # noqa: E731
    return S.Case("mmk_samplify_scores_f32", build, outs, call)


def _stream_cuts():
    def build(seed):
        g = S.gen(seed)
        cc = torch.sort(torch.randperm(ST - 700, generator=S.gen(9))[:SK])[0]
        return dict(y=S.uni(g, ST), e0=S.uni(g, 60).double(), g0=S.uni(g, 60).double(), e1=S.uni(g, SN).double(), g1=S.uni(g, SN).double(),
                    cc=cc, cp=cc + torch.randint(1, 600, (SK,), generator=S.gen(10)))

    def call(L, a, s):
        e = (native.vp * 2)(a["e0"].data_ptr(), a["e1"].data_ptr())
        gr = (native.vp * 2)(a["g0"].data_ptr(), a["g1"].data_ptr())
        knots = (native.i64 * 2)(60, SN)
        return L.mmk_samplify_cuts_i64(S.P(a["y"]), ST, e, gr, knots, 2, S.P(a["cc"]), S.P(a["cp"]), SK, S.P(a["sides"]), S.P(a["lr"]), S.P(a["cuts"]), s)
    outs = lambda L, i: dict(sides=((SK,), torch.int64), lr=((SK, 2), torch.float32), cuts=((SK,), torch.int64))      # noqa: E731
    return S.Case("mmk_samplify_cuts_i64", build, outs, call)


STREAM_CASES = [_stream_coef(), _stream_eval(), _stream_periods_count(), _stream_periods_fill(), _stream_scores(), _stream_cuts()]


def test_every_entry_point_with_a_stream_has_a_case():
    with_stream = [name for name, (_, args) in native._SAMPLIFY_SIGNATURES.items() if name != "mmk_periods_workspace_bytes"]
    assert sorted(c.entry for c in STREAM_CASES) == sorted(with_stream)


@pytest.mark.parametrize("case", STREAM_CASES, ids=[c.id for c in STREAM_CASES])
def test_entry_point_behind_a_busy_side_stream(device, case):
    """tests/test_gpu_streams.py's method: the real input twice on the default stream (the same bits), the stale input once (other bits),
    then behind a delay and a late write of the input on a side stream: the default-stream bits, and the call came back while the stream
    was still busy"""
    bound = S.Bound(case, device)
    want = bound.run_default("real")
    again = bound.run_default("real")
    assert not S.differs(want, again), (case.id, "two default-stream calls disagree")
    bound.check_surround(case.id + " on the default stream")
    stale = bound.run_default("stale")
    assert S.differs(want, stale), (case.id, "the stale input gives the real input's bits: the case proves nothing")
    got, busy, host = S.late_input(bound, S.side_stream(device))
    print(f"[streams] {case.id}: host time of the call {host * 1e3:.3f} ms, busy on return: {busy}")
    assert not S.differs(want, got), (case.id, "behind a late input on a side stream the outputs differ from the default-stream run")
    bound.check_surround(case.id + " on the side stream")
    assert busy, (case.id, f"the call waited for its stream (or took {host * 1e3:.1f} ms on the host)")
