"""The references of tests/net_refs.py against each other, on the host: for every case of test_gpu_networks_f64.py, on the fp32 oracle's own
free-running history, the float64 run is the same function as the fp32 one, both fp32 runs lie inside the envelope, the oracle's own picks
pass check_picks on every step, and each of the four defects - and every option defect of an option case - leaves the envelope (a network
of several targets: per target, each with its own envelope).  And the kernels' activation formulas (csrc/mmk_common.h) against float64.
The 55 option cases add about 30 s to this module on the host, at most 1 s each for either test.
The same for lives 2 and 3 of every case (net_refs.lives: the later generations of test_gpu_plan_lives.py): the fp32 oracle inside the
life's own envelope, the life defects (e), (f) and (g) outside it, and the arithmetic of the lives.  The SampleRNN oracle can be started from
the tier states a generation left (defect (g)): its reset_hidden is stubbed on the one instance, nothing of it is rewritten."""
import functools

import pytest
import torch
import torch.nn.functional as F

from tests import net_refs as R

torch.set_grad_enabled(False)
IDS = [f"{net}-{case.id}" for net, case in R.ALL_CASES]


@functools.lru_cache(maxsize=None)
def _run(index):
    case = R.ALL_CASES[index][1]
    prompt, conds = case.inputs()
    hist = R.free_run(case, prompt, conds)
    return case, hist, conds, R.envelope(hist, case, conds)


@functools.lru_cache(maxsize=None)
def _life(index, which):
    """life `which` (1 .. 3) of the case on the fp32 oracle's own free-running history of that life; life 1 is the case itself"""
    if which == 1:
        return _run(index)
    life = R.lives(R.ALL_CASES[index][1])[which - 1]
    prompt, conds = life.inputs()
    hist = R.free_run(life, prompt, conds)
    return life, hist, conds, R.envelope(hist, life, conds)


@pytest.mark.parametrize("index", range(len(R.ALL_CASES)), ids=IDS)
def test_fp32_oracle_lies_inside_its_own_envelope(index):
    """the case, and lives 2 and 3 of it (net_refs.lives: the generations test_gpu_plan_lives.py runs on a plan that has generated before)"""
    for which in (1, 2, 3):
        _inside_its_own_envelope(IDS[index] + ("" if which == 1 else f" life {which}"), *_life(index, which))


def _inside_its_own_envelope(tag, case, hist, conds, envs):
    rows = case.rows()
    for k, env in enumerate(R.per_target(envs)):
        what = f"{tag} target {k}" if case.multi else tag
        R64, E = env.R64[:, rows], env.E[:, rows]
        assert env.R64.dtype == torch.float64 and env.R64.shape[:2] == (case.clips, case.n)
        scale = float(env.R64.abs().max())
        worst = float((env.R32.double() - env.R64).abs().max())
        # (affine residuals: a layer's output is x_hat(h) a(h) + b(h), a product of two functions of the same input, so a relative error of h
        #  leaves the layer doubled - the fp32 run of L such layers may lie 2^L times farther from the float64 one and is still the same function)
        grows = 2.0 ** len(case.arch["kernels"]) if case.arch.get("affine") else 1.0
        assert worst <= 1e-5 * scale * grows, f"the float64 run is another function: |R32 - R64| up to {worst:.3e} at an output scale of {scale:.3e}"
        tol_max, tol_rms = R.tolerance(E)
        assert tol_max > 0
        print(f"[net_refs] {what}: max(E) {float(E.max()):.3e}, rms(E) {R.rms(E):.3e}")
        for name, run in (("R32", env.R32), ("R32k", env.R32k)):
            got = run[:, rows]
            print(f"[net_refs] {what} {name}: max / rms error {float((got.double() - R64).abs().max()):.3e} / {R.rms(got.double() - R64):.3e}, "
                  f"ratios {R.ratios(got, R64, E)}, output scale {scale:.3g}")
            R.check_outputs(got, R64, tol_max, tol_rms, f"{what} {name}")
        if case.classes:
            picks = R.streams(hist)[k][:, case.P:].long()
            R.check_picks(picks, env.R64, tol_max, f"{what} the fp32 oracle's own picks")


@pytest.mark.parametrize("index", range(len(R.ALL_CASES)), ids=IDS)
def test_every_defect_leaves_the_envelope(index):
    """the four standing defects and the case's option defects; a network of several targets: each target has its own tol_max"""
    case, hist, conds, envs = _run(index)
    rows = case.rows()
    envs = R.per_target(envs)
    R64 = [env.R64[:, rows] for env in envs]
    tol_max = [R.tolerance(env.E[:, rows])[0] for env in envs]
    full = [env.R64 for env in envs]
    names = []
    for name, out in R.defects(case, hist, conds, full if case.multi else full[0]):
        out = [o[:, rows] for o in R.per_target(out)]
        print(f"[net_refs] {IDS[index]} {name}: moves the compared outputs by up to {[f'{float((o - r).abs().max()):.3e}' for o, r in zip(out, R64)]}, "
              f"tol_max {[f'{t:.3e}' for t in tol_max]}")
        R.check_near_miss(out, R64, tol_max, f"{IDS[index]} {name}")
        names.append(name)
    assert len(names) >= 4 + len(case.options)


@pytest.mark.parametrize("index", range(len(R.ALL_CASES)), ids=IDS)
def test_every_life_defect_leaves_the_envelope(index):
    """lives 2 and 3: (e) a prompt of the life before, (f) a ragged group's rows of the life before and, for SampleRNN's life 2, (g) tier
    states carried over - each against the tol_max of the life's compared rows, the tolerance the device is held to"""
    for which in (2, 3):
        life, hist, conds, envs = _life(index, which)
        prev, prev_hist, _, prev_envs = _life(index, which - 1)
        rows = life.rows()
        envs = R.per_target(envs)
        tol_max = [R.tolerance(env.E[:, rows])[0] for env in envs]
        full, prev_full = [env.R64 for env in envs], [env.R64 for env in R.per_target(prev_envs)]
        names = ""
        for name, out, where in R.life_defects(life, hist, conds, full if life.multi else full[0], prev_hist, prev_full if life.multi else prev_full[0], prev):
            assert where, (IDS[index], which, name, "no compared row is reached by the prompt")
            at = [rows[i] for i in where]
            out, R64 = [o[:, at] for o in R.per_target(out)], [r[:, at] for r in full]
            print(f"[net_refs] {IDS[index]} life {which} {name}: moves {len(at)} of {len(rows)} compared rows by up to "
                  f"{[f'{float((o - r).abs().max()):.3e}' for o, r in zip(out, R64)]}, tol_max {[f'{t:.3e}' for t in tol_max]}")
            R.check_near_miss(out, R64, tol_max, f"{IDS[index]} life {which} {name}")
            names += name[1]
        assert names == ("efg" if life.kind == "srnn" and which == 2 else "ef")


# the clips of life 3, B -> max(1, B // 2 - 1): ragged against the groups of 2, 4 and 16 the kernels work in, or a single clip
LIFE_3_CLIPS = {5: 1, 8: 3, 13: 5, 20: 9, 24: 11, 21: 9, 33: 15, 40: 19, 17: 7, 128: 63, 16: 7, 3: 1, 9: 3, 11: 4}


def test_life_arithmetic():
    """what net_refs.lives promises test_gpu_plan_lives.py: lives 1 and 4 are the case bit for bit, life 3's clips, life 2 starts below
    life 1's end on another ring phase, the warm-up starts, and the resident blocks of the later lives"""
    seen = set()
    for _, case in R.ALL_CASES:
        one, two, three, four = R.lives(case)
        for life in (one, four):
            assert (life.clips, life.P, life.parts, life.n, life.rows()) == (case.clips, case.P, case.parts, case.n, case.rows())
        if case.id in ("chain-cond", "multi-srnn_mean_3x3", "two_inputs", "frames-g4"):
            for a, b in zip((*R.streams(case.inputs()[0]), *case.inputs()[1]), (*R.streams(four.inputs()[0]), *four.inputs()[1])):
                assert torch.equal(a, b)
            assert not torch.equal(R.streams(case.inputs()[0])[0], R.streams(two.inputs()[0])[0][:, :case.P])
            assert all(torch.equal(a, b) for a, b in zip(R.streams(case.inputs(two)[0]), R.streams(two.inputs()[0])))
        assert three.clips == LIFE_3_CLIPS[case.clips] and two.clips == case.clips
        seen.add(case.clips)
        assert two.parts == three.parts == case.parts[:len(two.parts)] and two.sd is case.sd and three.arch is case.arch
        if case.kind in ("s2s", "s2s_classes"):
            assert two.P == three.P == case.hop and two.parts == (1, 1)
            continue
        assert two.P == case.P + 5 and two.P + two.n < case.P + case.n          # (life 1's last tags and slots lie ahead of all of life 2)
        assert three.P == case.shortest_prompt == case.P - 3 - (case.arch["frame_sizes"][0] if case.kind == "srnn" else 0)
        if case.kind != "srnn":
            assert two.P - case.shortest_prompt == 8 and sum(two.parts) == 15      # (the warm-up starts at position 8, life 3's at 0)
            continue
        fs0 = case.arch["frame_sizes"][0]
        assert (one.P % fs0, two.P % fs0, three.P % fs0) == (3 % fs0, 8 % fs0, 0)          # (the warm-up's offset: 3, 8 and 0 at frame sizes 16 and 32)
        assert one.whole_period_warmup and two.whole_period_warmup and not three.whole_period_warmup
        if case.parts not in (R.RES_PARTS_16, R.RES_PARTS_32):
            assert sum(two.parts) == 15
            continue
        # resident mode (csrc/srnn_plan.hip, run_steps): a head of (fs0 - t % fs0) % fs0 steps with the kernels in turns, then ONE resident launch
        # if at least a period is left.  Every block of lives 2 and 3 is at least two periods long and leaves the launch more than a period; behind
        # life 2's head of 8 (24) steps the first block holds two WHOLE periods and more (life 1's, behind a head of 13 (29), holds less than two)
        assert len(two.parts) == 2
        for life in (two, three):
            t = life.P
            for k, nb in enumerate(life.parts):
                head = (fs0 - t % fs0) % fs0
                assert nb >= 2 * fs0 and nb - head > fs0, (case.id, life.index, k, nb, head)
                if k == 0:
                    assert head == {2: fs0 - 8, 3: 0}[life.index] and nb - head >= 2 * fs0
                t += nb
    assert seen == set(LIFE_3_CLIPS)
    assert R.spipe_pair_form(24) and not R.spipe_pair_form(11) and not R.spipe_pair_form(22) and not R.spipe_pair_form(130)


def test_seq2seq_dropped_reverse_bias_is_seen_now():
    """entries of dec.lstm.0.bias_hh_l0_reverse zeroed one at a time, resident bi-LSTM geometry (128, 8, 16, 2 layers): some move the frames by
    less than the 2e-4 max|want| the older test allows, and every one of them leaves the envelope"""
    index = next(i for i, (_, c) in enumerate(R.ALL_CASES) if c.id == "resident-128-8-16-2layers")
    case, hist, conds, env = _run(index)
    tol_max, _ = R.tolerance(env.E)
    old = 2e-4 * float(env.R64.abs().max())
    unseen = 0
    for entry in range(0, 512, 37):
        name, out = R.bias_dropped(case, hist, conds, entry)
        assert "dec.lstm.0.bias_hh_l0_reverse" in name
        moved = float((out - env.R64).abs().max())
        print(f"[net_refs] {name}: moves the frames by {moved:.3e}; older tolerance {old:.3e}, tol_max {tol_max:.3e}")
        unseen += moved <= old
        with pytest.raises(AssertionError):
            R.check_outputs(out, env.R64, tol_max, float("inf"), "the defect as a device output")
        R.check_near_miss(out, env.R64, tol_max, name)
    assert unseen > 0, "the older tolerance would have seen every one of these"


def test_split_k_cases_force_a_split_the_default_does_not_take():
    """the arithmetic of csrc/gemm.hip for the split-K cases: the GEMM has at least three stages, the forced split is honoured as it stands (no
    clamp) and is not what the launch would choose by itself; and why model_dim 128 would not do"""
    cases = [c for _, c in R.ALL_CASES if c.forced_split]
    assert sorted(c.forced_split[3] for c in cases) == [2, 3]
    for c in cases:
        M, N, K, forced = c.forced_split
        assert M == c.clips * c.hop >= 128 and K == c.sd["enc.fc_out.weight"].shape[0] and N == c.sd["output_module.heads.0.0.weight"].shape[0]
        assert c.env["MMK_GEMM_KSPLIT"] == str(forced)
        ks, stages = R.gemm_k_split(M, N, K, forced)
        default, _ = R.gemm_k_split(M, N, K)
        assert stages >= 3 and ks == forced and ks != default, (c.id, ks, stages, default)
    assert R.gemm_k_split(128, 65, 128, 3) == (2, 2) and R.gemm_k_split(128, 65, 128) == (2, 2)


def test_check_picks_refuses_a_clear_second_best():
    R64 = torch.tensor([[[0.0, 1.0, 0.5, 9.0]]], dtype=torch.float64)      # (the last column is the temperature's)
    R.check_picks(torch.tensor([[1]]), R64, 1e-6)
    with pytest.raises(AssertionError):
        R.check_picks(torch.tensor([[2]]), R64, 1e-6)
    with pytest.raises(AssertionError):
        R.check_picks(torch.tensor([[3]]), R64, 1e-6)
    R.check_picks(torch.tensor([[2]]), R64, 0.25)


# ---- the formulas themselves ---------------------------------------------------------------------------------------------------------------------------
def _grid():
    """[-30, 30] in steps of 1 / 2048 and, around 0, +- 2^-k / 2^-k (1 + 2^-3 j): every binade down to 2^-40"""
    small = torch.cat([2.0 ** -k * (1 + torch.arange(8) / 8.0) for k in range(0, 41)])
    return torch.cat([torch.linspace(-30, 30, 60 * 2048 + 1), small, -small, torch.zeros(1)]).float()


U = 2.0 ** -24
# sigmoid_fast: t = fl(x c), c = fl(-log2 e): |dt| <= 2 u |t|, which 2^t turns into a relative 2 u |x| of e = exp(-x); exp2, the sum and the
# quotient add 3 u (relative, the CPU's are correctly rounded to ~1 ulp): |ds| <= s (1 - s) 2 u |x| + 3 u s <= (2 * 0.2239 + 3) u -> 4 u
SIGMOID_ABS = 4 * U
# tanh_fast = 2 s(2 x) - 1: twice that at 2 x, and the last sum: 9 u absolute.  RELATIVE to tanh(x) ~ x the formula has no bound near 0 (the
# 1 is subtracted from a rounded 2 s): below |x| = u it returns 0 or 2 u
TANH_ABS = 9 * U
# mish_fast = x n / (n + 2): e = exp(min(x, 20)) (~1 ulp), n = e (e + 2), the quotient and the product: every step a relative rounding, no
# cancellation (all terms positive): <= 8 u relative over the whole range
MISH_REL = 8 * U


def test_kernel_formulas_against_float64():
    """the figures recorded beside sigmoid_fast / tanh_fast / mish_fast in csrc/mmk_common.h (torch's exp2 / exp and an exact division stand for
    v_exp_f32 / v_rcp_f32 here)"""
    x = _grid()
    x64 = x.double()
    worst = {}
    for name, f, ref in (("sigmoid", R.k_sigmoid, torch.sigmoid), ("tanh", R.k_tanh, torch.tanh), ("mish", R.k_mish, F.mish)):
        got, want = f(x).double(), ref(x64)
        assert got.dtype == torch.float64 and f(x).dtype == torch.float32
        err = (got - want).abs()
        rel = torch.where(want != 0, err / want.abs(), torch.zeros_like(err))
        worst[name] = (float(err.max()), float(rel.max()), float(rel[x.abs() >= 2.0 ** -6].max()))
        print(f"[formulas] {name}_fast vs float64 over [-30, 30]: worst absolute {worst[name][0]:.3e} ({worst[name][0] / U:.2f} u), worst relative "
              f"{worst[name][1]:.3e}, worst relative for |x| >= 2^-6 {worst[name][2]:.3e}")
    assert worst["sigmoid"][0] <= SIGMOID_ABS and worst["tanh"][0] <= TANH_ABS and worst["mish"][1] <= MISH_REL
    assert worst["tanh"][1] >= 0.5          # (the comment says so: no relative bound near 0)
