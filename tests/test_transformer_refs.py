"""The references of tests/transformer_refs.py against each other, on the host: for every case of test_gpu_transformer_f64.py, on the fp32
modules' own free-running history (argmax of R32 fed back; frames fed back), the float64 walk is the network's own modules, both fp32 runs lie
inside the envelope, the fp32 picks pass check_picks on every step with no excused pick, and every defect that applies to the case leaves
tol_max.  Then what the cases claim about themselves: the plan branches their geometry reaches (the arithmetic of csrc/gemm.hip), that the
outputs depend on every layer and the picks on the prompt (why the cases' weights are what they are: transformer_refs.CASE_LN_OFFSET), and
that the conditions of the sampled-decode test hold for the references alone.

Records of the first run (tolerances are recomputed from the reference on every run).  derived / tol: the largest element of the bound
test_gpu_transformer.py derives from the kernels' bounds (first two steps) over tol_max = 4 max(E); the defects: max|defect - R64| / tol_max:

  case              outputs  scale     max(E)     rms(E) derived / tol   defects
  one_layer_rf9       30840  5.89   2.756e-06  6.871e-07           161   (a) 1.5e+03  (b) 45  (c) 1.98e+05  (d) 1.2e+05  (f) 1.89e+05  (g) 1.52e+05
  clips130_rf2      1336400  5.17   2.802e-06  5.819e-07      1.22e+05   (a) 390  (b) 19.3  (c) 5.74e+04  (d) 8.46e+04  (e) 3.39e+04  (f) 3.6e+04  (g) 1.56e+05  (h) 3.95e+05  (i) 1.03e+05
  ff24_rf33           41120  5.19   2.580e-06  5.554e-07      2.36e+03   (a) 774  (b) 30  (c) 1.03e+05  (d) 4.4e+04  (e) 1.42e+04  (f) 5.33e+04  (g) 5.92e+04  (h) 5.3e+05
  ff8_rf33            41120  4.87   3.831e-06  7.651e-07      1.17e+03   (a) 701  (b) 33.5  (c) 9.09e+04  (d) 3.34e+04  (e) 2.27e+04  (f) 2.94e+04  (g) 4.59e+04  (h) 2.92e+05
  frames130_rf2       41990  3.64   1.662e-06  3.952e-07       4.9e+03   (a) 1.37e+03  (b) 67.1  (c) 1.5e+05  (d) 3.55e+05  (f) 1.35e+05  (g) 1.25e+05
  layer_norm_rf65     20560  5.28   3.575e-06  7.547e-07      4.63e+03   (a) 717  (b) 42.6  (c) 9.09e+04  (d) 3.99e+04  (e) 2.73e+04  (f) 3.43e+04  (g) 3.47e+04  (h) 2.83e+05  (i) 1.06e+05
  head_dim128          9766  4.96   6.082e-06  1.447e-06      3.08e+03   (a) 87.4  (b) 11.5  (c) 1.48e+04  (d) 9.68e+03  (e) 3.39e+03  (f) 8.31e+03  (g) 1.42e+04  (h) 1.75e+05
  default              9766  4.29   4.118e-06  1.302e-06      3.43e+15   (a) 298  (b) 3.69  (c) 2.02e+04  (d) 1.13e+04  (e) 8.45e+03  (f) 1.27e+03  (g) 1.75e+04  (h) 2.95e+05

The derived bound carries every error through every later layer's first-order sensitivity, summed over the rows: on weights whose layers
pass what reaches them (these cases) it grows by two orders per layer and says nothing at eight layers.  With the recipe's own weights
(gain 1.5, LayerNorm weights around zero: each layer passes a twentieth) the same columns read, for the same geometries and seeds: derived / tol
39, 100, 20, 18, 23, 45, 52, 22; defect (b) 24, 4.3, 9.4, 7.9, 23, 14, 1.0 and 6e-5 tol_max - inside the envelope at the default size, at it
with head_dim 128 - and the greedy picks of every case are one class from the first step on.  Hence the cases' weights (transformer_refs.py).
The fp32 modules' own picks pass check_picks in every case with the seeds as first chosen; R32 / R32k: max ratios 0.79 .. 1.00, rms 0.76 .. 0.84.
"""
import functools

import pytest
import torch

from tests import helpers as H
from tests import net_refs as N
from tests import transformer_refs as R

torch.set_grad_enabled(False)
TAGS = [c.tag for c in R.CASES]


@functools.lru_cache(maxsize=None)
def _run(tag):
    case = R.BY_TAG[tag]
    hist = R.free_run(case)
    return case, hist, R.envelope(hist, case)


@pytest.mark.parametrize("tag", TAGS)
def test_walk_is_the_network_and_the_fp32_runs_lie_inside_the_envelope(tag):
    case, hist, env = _run(tag)
    assert env.R64.shape[:2] == (case.clips, case.n) and env.R64.shape == env.R32.shape == env.R32k.shape
    diff, scale = R.walk_is_the_network(case, hist)
    assert diff <= 1e-12 * scale, f"{tag}: the walk is not the network (off by {diff:.3e} at scale {scale:.3e})"
    tol_max, tol_rms = R.tolerance(env.E)
    assert tol_max > 0
    worst = float((env.R32.double() - env.R64).abs().max())
    assert worst <= 1e-5 * scale, f"{tag}: the float64 run is another function: |R32 - R64| up to {worst:.3e} at an output scale of {scale:.3e}"
    for name, run in (("R32", env.R32), ("R32k", env.R32k)):
        print(f"[transformer_refs] {tag} {name}: ratios {R.ratios(run, env.R64, env.E)}")
        R.check_outputs(run, env.R64, tol_max, tol_rms, f"{tag} {name}")
    if case.classes:
        picks = hist[:, case.prompt:]
        assert torch.equal(picks, env.R32[..., :-1].argmax(-1))
        R.check_picks(picks, env.R64, tol_max, f"{tag} the fp32 modules' own picks")
    derived = R.derived_bound(case, hist)
    print(f"[transformer_refs] {tag}: {env.R64.numel()} outputs of scale {scale:.3g}, max(E) {float(env.E.max()):.3e}, rms(E) {R.rms(env.E):.3e}, "
          f"derived bound / tol_max = {derived / tol_max:.3g}")


@pytest.mark.parametrize("tag", TAGS)
def test_every_applicable_defect_leaves_the_envelope(tag):
    case, hist, env = _run(tag)
    tol_max, _ = R.tolerance(env.E)
    letters = ""
    for name, out in R.defects(case, hist, env.R64):
        print(f"[transformer_refs] {tag} {name}: moves the outputs by {float((out - env.R64).abs().max()) / tol_max:.3g} tol_max")
        R.check_near_miss(out, env.R64, tol_max, f"{tag} {name}")
        letters += name[1]
    assert letters == R.applicable(case)
    # the rules of the defects that do not apply, as the module states them
    assert ("e" in letters) == ("h" in letters) == (case.layers >= 2) and ("f" in letters) == (case.rf >= 2)
    assert ("i" in letters) == bool(case.net_kw.get("with_layer_norm"))


@functools.lru_cache(maxsize=None)
def _life(tag, which):
    """life `which` (1 .. 3) of the case (transformer_refs.lives) on the fp32 modules' own free-running history of that life"""
    if which == 1:
        return _run(tag)
    life = R.lives(R.BY_TAG[tag])[which - 1]
    hist = R.free_run(life)
    return life, hist, R.envelope(hist, life)


@pytest.mark.parametrize("tag", TAGS)
def test_later_lives_lie_inside_the_envelope_and_their_defects_leave_it(tag):
    """lives 2 and 3 of test_gpu_plan_lives.py, for the references alone: both fp32 runs inside the life's envelope, the fp32 picks pass, and
    a prompt or a ragged group's rows of the life before leave tol_max"""
    for which in (2, 3):
        life, hist, env = _life(tag, which)
        _, prev_hist, prev_env = _life(tag, which - 1)
        assert env.R64.shape[:2] == (life.clips, life.n) and hist.shape[1] == life.prompt + life.n
        tol_max, tol_rms = R.tolerance(env.E)
        for name, run in (("R32", env.R32), ("R32k", env.R32k)):
            print(f"[transformer_refs] {tag} life {which} {name}: ratios {R.ratios(run, env.R64, env.E)}")
            R.check_outputs(run, env.R64, tol_max, tol_rms, f"{tag} life {which} {name}")
        if life.classes:
            R.check_picks(hist[:, life.prompt:], env.R64, tol_max, f"{tag} life {which} the fp32 modules' own picks")
        letters = ""
        for name, out, steps in R.life_defects(life, hist, env.R64, prev_hist, prev_env.R64):
            assert steps
            print(f"[transformer_refs] {tag} life {which} {name}: moves {len(steps)} of {life.n} steps by "
                  f"{float((out[:, steps] - env.R64[:, steps]).abs().max()) / tol_max:.3g} tol_max")
            R.check_near_miss(out[:, steps], env.R64[:, steps], tol_max, f"{tag} life {which} {name}")
            letters += name[1]
        assert letters == "ef"


def test_life_arithmetic():
    for case in R.CASES:
        one, two, three, four = R.lives(case)
        for life in (one, four):
            assert (life.clips, life.prompt, life.parts, life.tag) == (case.clips, case.prompt, case.parts, case.tag)
            assert torch.equal(life.inputs(), case.inputs())
        assert (two.clips, two.prompt, two.parts) == (case.clips, case.rf + 8, case.parts)
        assert (three.clips, three.prompt, three.parts) == ({130: 64, 4: 1, 3: 1, 2: 1}[case.clips], case.rf, case.parts)
        assert two.inputs().shape[1] == two.prompt and not torch.equal(two.inputs()[:, :case.prompt], case.inputs())
        assert two.ends() == case.ends() and R.nets(two.tag) is R.nets(case.tag)


def test_a_leaking_mask_moves_nothing_in_a_one_layer_network():
    """the rule of defect (e): the outputs depend on the last row's query only, which sees every key"""
    case, hist, env = _run("one_layer_rf9")
    assert torch.equal(R.reference64(case, hist, defect="leak"), env.R64)


def test_the_cases_reach_the_branches_they_name():
    """csrc/transformer_plan.hip, tr_linear: the tiled GEMM from 128 rows and K >= 16 on (gemm_bias_act_supported); emit_step: the last layer
    and the head run on M = clips rows, the other layers on clips x rf"""
    c = R.BY_TAG
    for tag, rows_all, rows_last in (("one_layer_rf9", False, False), ("clips130_rf2", True, True), ("ff24_rf33", True, False), ("ff8_rf33", True, False),
                                     ("frames130_rf2", True, True), ("layer_norm_rf65", True, False)):
        assert (c[tag].clips * c[tag].rf >= 128, c[tag].clips >= 128) == (rows_all, rows_last), tag
    assert c["one_layer_rf9"].layers == 1 and c["one_layer_rf9"].rf > 1 and c["frames130_rf2"].layers == 1
    ff = c["ff24_rf33"].net_kw["feedforward_dim"]
    assert ff >= 16 and ff % 16 != 0 and ff % 4 == 0                      # (ff2 tiled: K >= 16 and lda % 4 == 0, a ragged last chunk)
    assert c["ff8_rf33"].net_kw["feedforward_dim"] < 16                   # (ff2 on the row-tile kernel, ff1 tiled with N = 8)
    assert c["clips130_rf2"].io_kw["n_mlp_layers"] == 2                   # (a hidden block: three tiled Linears in the head, the last N = 257)
    kw = c["layer_norm_rf65"].net_kw
    # split K: ff2 of the rf-65 case has K = 96 = two stages and few tiles
    assert N.gemm_k_split(2 * 65, kw["model_dim"], kw["feedforward_dim"])[0] == 2
    hd = c["head_dim128"].net_kw
    assert hd["model_dim"] // hd["n_heads"] == 128
    assert R.nets("default")[0].config.rf == 64 and R.nets("default")[0].config.num_layers == 8
    # blocks: 19 = two replays of the 8-step graph + 3 plain steps, 16 = two replays at another t0, 5 < 2 x 8: no graph
    assert R.PARTS == (19, 16, 5) and all(case.parts[0] >= 16 for case in R.CASES)


def test_the_outputs_depend_on_every_layer_of_the_default_network():
    """why the cases' LayerNorm weights lie around one (transformer_refs.CASE_LN_OFFSET): the cross-attention in_proj_weight of layer l scaled by
    1 + 1e-4 moves the outputs by the same order for every l - the first layer's by no less than a hundredth of the last layer's.  With the
    recipe's own LayerNorm weights (around zero) every layer passes about a twentieth, and the first layer's share is 3e-10 of the last's:
    the two regimes lie eight orders apart, the threshold between them is not delicate"""
    case, hist, env = _run("default")
    tol_max, _ = R.tolerance(env.E)
    sd = R.nets("default")[1].state_dict()
    moved = []
    for l in range(case.layers):
        key = f"model.layers.{l}.multihead_attn.in_proj_weight"
        out = R.reference64(case, hist, weights={key: sd[key] * (1 + 1e-4)})
        moved.append(float((out - env.R64).abs().max()))
        print(f"[transformer_refs] default {key} scaled: moves the outputs by {moved[-1] / tol_max:.3g} tol_max")
    assert min(moved) >= 1e-2 * moved[-1], moved


@pytest.mark.parametrize("tag", R.CACHE_HIT_CASES)
def test_the_picks_depend_on_the_prompt(tag):
    """the graph cache-hit test writes another prompt and requires other picks: the fp32 modules give other picks for it"""
    case, hist, _ = _run(tag)
    other = R.free_run(case, case.inputs(seed=1000 + case.seed))
    a, b = hist[:, case.prompt:case.prompt + case.parts[0]], other[:, case.prompt:case.prompt + case.parts[0]]
    differ = float((a != b).float().mean())
    print(f"[transformer_refs] {tag}: {differ * 100:.1f} % of the picks differ under another prompt; {len(torch.unique(a))} classes picked")
    assert differ > 0 and len(torch.unique(a)) > 1


def sampled_inputs(case, n):
    g = torch.Generator().manual_seed(3)
    return torch.linspace(0.5, 1.5, case.clips), torch.rand(case.clips, n, generator=g)


def test_sampled_picks_of_the_float64_walk_pass_against_the_fp32_modules():
    """the conditions of the device's sampled-decode test (every pick within 2e-5 of its CDF interval, at least 98 % inside it), for the
    references alone: classes drawn from the float64 walk's logits, held against R32 of that history"""
    case = R.BY_TAG[R.SAMPLED_CASE]
    n = case.parts[0]
    temps, u = sampled_inputs(case, n)
    hist = R.sampled_run(case, temps, u)
    ok, exact = H.sampled_picks_ok(R.reference32(case, hist), temps, u, hist[:, case.prompt:])
    print(f"[transformer_refs] {case.tag} sampled: {float(exact.float().mean()) * 100:.2f} % of {exact.numel()} picks inside their interval, "
          f"{len(torch.unique(hist[:, case.prompt:]))} classes")
    assert bool(ok.all()) and float(exact.float().mean()) >= 0.98
    assert len(torch.unique(hist[:, case.prompt:])) > 8          # (a sampled stream, not one class)
