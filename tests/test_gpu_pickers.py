"""Every class picker on the device against tests/picker_refs.py (float64 inverse-CDF intervals, the fp32 argmax of the quotients), on
crafted rows of EXACT logits: `sample_kernel` directly, and each in-kernel site through a network whose head's last layer has zero weights
and a crafted bias - its output is 0 * h + bias, the bias row itself, for every clip and step (checked through last_logits; only a bias of
-0.0 comes out as +0.0, which equals it).  DESIGN.md, "class pickers", lists the sites."""
import pytest
import torch

import mimikit_amd as mmk
from mimikit_amd import native
from oracle.weights import load_recipe
from tests import helpers as H
from tests import picker_refs as P
from tests.strided_inputs import FLOAT_SURROUNDS, Strided, surround_rule

pytestmark = pytest.mark.gpu

B, N = 8, 32                                             # clips x steps per row: 256 draws, entry b * N + s of the row's U_GRID
CLIP_TEMPS = [0.25, 0.5, 0.7, 0.9, 1.0, 1.3, 1.7, 2.0]   # each clip its own T
DIRECT_TEMPS = [0.25, 0.9, 2.0]
WN_KEYS = ("MMK_WN_XCD_LOCAL", "MMK_WN_PERSISTENT", "MMK_WN_GROUPS", "MMK_WN_SMALL", "MMK_WN_PREFILL", "MMK_WN_CHAIN", "MMK_WN_LPIPE", "MMK_WN_SPIPE",
           "MMK_WN_BPIPE", "MMK_WN_PIPE", "MMK_WN_SPIPE_PAIR")
SRNN_KEYS = ("MMK_SRNN_FUSED", "MMK_SRNN_FUSED_UP", "MMK_SRNN_RESIDENT", "MMK_SRNN_RESIDENT_WARMUP", "MMK_SRNN_COMPOSED")


class Tally:
    """draws, the share that needs the tolerance (random uniforms only; the ones put on CDF steps are counted apart), the largest miss"""

    def __init__(self):
        self.draws = self.off = self.off_inexact = self.on = self.on_inexact = self.greedy = 0
        self.miss = self.tol = 0.0

    def add(self, r, on_step):
        self.draws += r["ok"].numel()
        self.off += int((~on_step).sum())
        self.off_inexact += int((~r["exact"][~on_step]).sum())
        self.on += int(on_step.sum())
        self.on_inexact += int((~r["exact"][on_step]).sum())
        self.miss, self.tol = max(self.miss, float(r["miss"].max())), max(self.tol, float(r["tol"].max()))

    def report(self, what):
        share = self.off_inexact / max(self.off, 1)
        print(f"[pickers] {what}: {self.draws} sampled draws, {self.greedy} greedy picks; random uniforms that need the tolerance {self.off_inexact} of "
              f"{self.off} ({share * 100:.3f} %, limit 1 %); on CDF steps {self.on_inexact} of {self.on}; largest miss {self.miss:.2e} of the total, "
              f"largest derived tolerance {self.tol:.2e} (C_PICK = {P.C_PICK})")
        assert share <= 0.01, what
        assert self.tol < 2e-5


def check_sampled(row, n, tl, T, u, on_step, picks, tally, what):
    r = P.check_picks_detail(row["logits"], n, tl, P.MIN_TEMP, T, u, picks)
    bad = (~r["ok"]).nonzero().reshape(-1)
    assert bool(r["hard"].all()), (what, row["name"], "a class that does not exist or has no mass was drawn", picks[~r["hard"]][:8].tolist())
    assert bad.numel() == 0, (what, row["name"], [(float(T.reshape(-1).expand(u.numel())[i]), float(u[i]), int(picks[i]), float(r["miss"][i])) for i in bad[:6]],
                              float(r["tol"].max()))
    tally.add(r, on_step)


# ---- sample_kernel directly ------------------------------------------------------------------------------------------------------------------------
@surround_rule(*FLOAT_SURROUNDS)
def sample_rows(logits, n, col, temp, uni, device):
    """native.categorical_sample on logits rows that are a strided, misaligned view (ld = width + PAD, 4 bytes in); the picks are those of
    the contiguous rows"""
    min_temp = P.MIN_TEMP if col else 0.
    temp, uni = (None if t is None else t.to(device) for t in (temp, uni))
    rows = Strided.of(logits.numpy(), 1, device)
    got = native.categorical_sample(rows.view, n, col, min_temp, temp, uni).cpu()
    assert torch.equal(got, native.categorical_sample(logits.to(device), n, col, min_temp, temp, uni).cpu()), "strided and contiguous rows give other picks"
    return got


@pytest.mark.parametrize("col", [True, False])
@pytest.mark.parametrize("n", [48, 64, 200, 256, 321, 1000, 1024])
def test_sample_kernel_on_crafted_rows(device, n, col):
    """csrc/kernels.hip: every crafted row x its U_GRID at three temperatures in one launch, the greedy rows in another; with the
    temperature column (denom = max(sigmoid, min_temp)) and without"""
    rows = P.CRAFTED_ROWS(n)
    width = n + int(col)
    what = f"sample_kernel n={n} {'with' if col else 'without'} the temperature column"

    def full(row):
        return torch.cat([row["logits"], torch.tensor([row["temp_logit"]])]) if col else row["logits"]

    tally = Tally()
    sampled = [r for r in rows if r["kind"] == "sampled"]
    blocks = []
    for row in sampled:
        tl = row["temp_logit"] if col else None
        for T in ([row["T"]] if row["T"] is not None else DIRECT_TEMPS):
            u, on = P.U_GRID(row["logits"], n, tl, P.MIN_TEMP, T, size=256, extra=row["u_extra"])
            blocks.append((row, tl, T, u, on))
    logits = torch.cat([full(row).expand(256, width) for row, *_ in blocks]).contiguous()
    temp = torch.cat([torch.full((256,), T) for _, _, T, _, _ in blocks])
    uni = torch.cat([u for *_, u, _ in blocks])
    got = sample_rows(logits, n, col, temp, uni, device)
    for i, (row, tl, T, u, on) in enumerate(blocks):
        check_sampled(row, n, tl, torch.tensor([T]), u, on, got[256 * i:256 * (i + 1)], tally, what)
    greedy = [r for r in rows if r["kind"] == "greedy"]
    logits = torch.stack([full(row) for row in greedy])
    got = sample_rows(logits, n, col, None, None, device)
    for row, pick in zip(greedy, got.tolist()):
        want = P.picker_ref(row["logits"], n, row["temp_logit"] if col else None, P.MIN_TEMP)
        assert pick == want, (what, row["name"], pick, want)
        if col and row["expect"] is not None:
            assert want == row["expect"]
        tally.greedy += 1
    tally.report(what)


# ---- the in-kernel sites -----------------------------------------------------------------------------------------------------------------------------
def _wavenet(q, C, blocks, mlp_dim, seed):
    net = mmk.WaveNet.from_config(mmk.WaveNet.Config(io_spec=H.mu_emb(mlp_dim=mlp_dim, q_levels=q, min_temperature=P.MIN_TEMP), blocks=blocks,
                                                     dims_dilated=(C,), residuals_dim=C, skips_dim=C)).eval()
    load_recipe(net, seed=seed, gain=2.0)
    return net


def _srnn(q, frame_sizes, seed, mlp_dim=128):
    net = mmk.SampleRNN.from_config(mmk.SampleRNN.Config(io_spec=H.mu_lin(mlp_dim=mlp_dim, q_levels=q, min_temperature=P.MIN_TEMP), frame_sizes=frame_sizes,
                                                         hidden_dim=128, rnn_class="gru")).eval()
    load_recipe(net, seed=seed, gain=2.0)
    return net


def _persist_loop(p, n):
    return p.persistent and not p.chain and not p.layer_pipelined and not p.stage_pipelined


# SampleRNN outside resident mode: the plan says what it emitted the bottom tier and the head as (include/mmk.h, mmk_srnn_bottom_kernel)
ONE_CLIP, FOUR_CLIPS, LAUNCHES = 1, 2, 3


def _bottom(kernel):
    return lambda p, n: p.resident_blocks() == 0 and p.bottom_kernel() == kernel


# site -> (network, plan switches, class counts, the path a count must take: (description, predicate on the plan), greedy of <= 256 classes
# goes through greedy_256: 'padded' - every head of <= 256 classes, padded to 256 -, 'at256' - at 256 classes -, or False)
SITES = {
    # wavenet_persist.hip's general loop: the two-hand-off kernel by name
    "wn_persist": dict(make=lambda q: _wavenet(q, 32, (3, 2), 32, 21), env={"MMK_WN_CHAIN": "0"}, counts=(48, 200, 256, 321),
                       path=lambda n: ("wavenet_persist general loop", _persist_loop), greedy256=False),
    # wavenet_chain.hip: sample_256 at 256 classes, its general loop otherwise (greedy: always its own loop)
    "wn_chain": dict(make=lambda q: _wavenet(q, 32, (3, 2), 32, 21), env={}, counts=(48, 200, 256, 321),
                     path=lambda n: ("wavenet_chain sample_256" if n == 256 else "wavenet_chain general loop", lambda p, n: p.chain), greedy256=False),
    # wavenet_lpipe.hip (heads of <= 256 classes, padded to 256 with -inf); beyond, the plan takes the one-hand-off kernel
    "wn_lpipe": dict(make=lambda q: _wavenet(q, 64, (4,), 128, 61), env={}, counts=(48, 200, 256, 321),
                     path=lambda n: ("wavenet_lpipe sample_256 / greedy_256", lambda p, n: p.layer_pipelined) if n <= 256 else
                     ("wavenet_chain general loop (the layer pipeline refuses > 256 classes)", lambda p, n: p.chain and not p.layer_pipelined),
                     greedy256="padded"),
    # wavenet_spipe.hip, one clip per visit; beyond 256 classes the two-hand-off kernel (256 channels: no chain by default)
    "wn_spipe": dict(make=lambda q: _wavenet(q, 256, (3,), 128, 62), env={"MMK_WN_SPIPE": "1", "MMK_WN_BPIPE": "0"}, counts=(48, 200, 256, 321),
                     path=lambda n: ("wavenet_spipe sample_256 / its greedy", lambda p, n: p.stage_pipelined and not p.batch_pipelined) if n <= 256 else
                     ("wavenet_persist general loop (the stage pipeline refuses > 256 classes)", _persist_loop), greedy256="padded"),
    # wavenet_bpipe.hip, 16 clips per visit; beyond 256 classes the plan refuses both stage pipelines: the two-hand-off kernel again
    "wn_bpipe": dict(make=lambda q: _wavenet(q, 256, (3,), 128, 62), env={"MMK_WN_SPIPE": "1", "MMK_WN_BPIPE": "1"}, counts=(48, 200, 256, 321),
                     path=lambda n: ("wavenet_bpipe sample_256 / greedy_256", lambda p, n: p.stage_pipelined and p.batch_pipelined) if n <= 256 else
                     ("wavenet_persist general loop (the batch pipeline refuses > 256 classes)", _persist_loop), greedy256="padded"),
    # srnn_bottom.hip, the one-clip-per-workgroup kernel (<= 256 classes): frame of one sample - greedy_256 in every wave at 256 classes
    "srnn_fused": dict(make=lambda q: _srnn(q, (16, 4, 1), 78), env={"MMK_SRNN_FUSED": "1", "MMK_SRNN_RESIDENT": "0"}, counts=(48, 200, 256),
                       path=lambda n: ("srnn_bottom one-clip kernel, " + ("sample_256 / greedy_256 in every wave" if n == 256 else "general loop"),
                                       _bottom(ONE_CLIP)), greedy256="at256", srnn=True),
    # ... a frame of two samples: wave 0 alone picks
    "srnn_fused_fs2": dict(make=lambda q: _srnn(q, (32, 8, 2), 79), env={"MMK_SRNN_FUSED": "1", "MMK_SRNN_RESIDENT": "0"}, counts=(256,),
                           path=lambda n: ("srnn_bottom one-clip kernel, sample_256 / greedy_256 in wave 0", _bottom(ONE_CLIP)),
                           greedy256="at256", srnn=True),
    # srnn_bottom.hip's first kernel (4 clips per workgroup, MFMA) takes the heads the one-clip kernel refuses: more than 256 classes.  Its fc2 image
    # in LDS is ceil((n + 1) / 16) * (mlp_dim / 16) KiB, held to 160 KiB with the rest: 322 outputs fit at mlp_dim 64 (84 KiB), not at 128 (168 KiB,
    # where the plan falls back to one launch per op)
    "srnn_bottom_tiles": dict(make=lambda q: _srnn(q, (16, 4, 1), 78, mlp_dim=64), env={"MMK_SRNN_FUSED": "1", "MMK_SRNN_RESIDENT": "0"}, counts=(321,),
                              path=lambda n: ("srnn_bottom four-clip kernel general loop (the one-clip kernel refuses > 256 classes)", _bottom(FOUR_CLIPS)),
                              greedy256=False, srnn=True),
    # MMK_SRNN_FUSED=0: one launch per op, the head's draw is sample_kernel
    "srnn_launches": dict(make=lambda q: _srnn(q, (16, 4, 1), 78), env={"MMK_SRNN_FUSED": "0"}, counts=(256, 321),
                          path=lambda n: ("sample_kernel behind the SampleRNN launch path", _bottom(LAUNCHES)), greedy256=False, srnn=True),
    # srnn_resident.hip
    "srnn_resident": dict(make=lambda q: _srnn(q, (16, 4, 1), 78), env={"MMK_SRNN_FUSED": "1"}, counts=(48, 200, 256),
                          path=lambda n: ("srnn_resident, " + ("sample_256 / greedy_256 in every wave" if n == 256 else "general loop"), None),
                          greedy256="at256", srnn=True, resident=True),
    "srnn_resident_fs2": dict(make=lambda q: _srnn(q, (32, 8, 2), 79), env={"MMK_SRNN_FUSED": "1"}, counts=(256,),
                              path=lambda n: ("srnn_resident, sample_256 / greedy_256 in wave 0", None), greedy256="at256", srnn=True, resident=True),
}
CASES = [(site, n) for site, s in SITES.items() for n in s["counts"]]


@pytest.mark.parametrize("site,n", CASES, ids=[f"{s}-{n}" for s, n in CASES])
def test_site_picks_on_crafted_rows(device, monkeypatch, site, n):
    """one small network per site, its head's last layer 0 * h + a crafted bias: every crafted row, 8 clips (each its own T) x 32 steps fed
    the row's U_GRID, then the greedy rows (the NaN rows where the greedy pick goes through greedy_256).  The plan's own flags say which kernel
    ran; last_logits must be the bias row."""
    spec = SITES[site]
    is_srnn = spec.get("srnn", False)
    for k in WN_KEYS + SRNN_KEYS:
        monkeypatch.delitem(native.PLAN_TUNING, k, raising=False)
    for k, v in spec["env"].items():
        monkeypatch.setitem(native.PLAN_TUNING, k, v)
    path, on_path = spec["path"](n)
    what = f"{site} n={n} [{path}]"
    net = spec["make"](n).to(device)
    last = net.output_modules[0].estimator[0].fc[-1]
    assert last.weight.shape[0] == n + 1
    Pn = 32 if is_srnn else net.rf + 3
    prompt = torch.randint(0, n, (B, Pn), generator=torch.Generator().manual_seed(n))
    residents = [0]

    def run(row, temp, uni):
        bias = torch.cat([row["logits"], torch.tensor([row["temp_logit"]])])
        with torch.no_grad():
            last.weight.zero_()
            last.bias.copy_(bias.to(device))
        idx = torch.cat([prompt, torch.zeros(B, N, dtype=torch.int64)], 1).to(device)
        packs = native.pack_launch_count()
        net.before_generate((idx[:, :Pn],), None)
        assert native.pack_launch_count() > packs, "the new bias was not packed"
        t_dev = None if temp is None else temp.to(device)
        u_dev = None if uni is None else uni.to(device).contiguous()
        if is_srnn:
            net._plan.generate(idx, Pn, N, t_dev, u_dev)
        else:
            net._plan.generate(idx, (), Pn, N, t_dev, u_dev)
        torch.cuda.synchronize()
        plan = net._plan
        if spec.get("resident"):
            residents[0] += 1
            assert plan.resident_blocks() == residents[0], (what, "the block did not run in resident mode", plan.resident_blocks())
            plan.sync_status()
        else:
            assert on_path(plan, n), (what, "the plan took another kernel")
            if not is_srnn and plan.persistent:
                plan.sync_status()
        got = plan.last_logits(B).cpu()
        assert got.shape == (B, n + 1)
        # (== takes -0.0 for +0.0, and has to: 0 * h + (-0.0) is +0.0.  So the three tied zeros of `tie_first` are all +0.0 at these sites; its
        # +0.0 / -0.0 tie reaches a picker only in test_sample_kernel_on_crafted_rows, which hands the row to sample_kernel itself)
        same = (got == bias) | (torch.isnan(got) & torch.isnan(bias))
        assert bool(same.all()), (what, row["name"], "the head's output is not the bias row", got[~same][:8].tolist(), bias.expand(B, -1)[~same][:8].tolist())
        return idx.cpu()[:, Pn:]

    tally = Tally()
    for row in P.CRAFTED_ROWS(n):
        if row["kind"] == "sampled":
            temps = [row["T"]] * B if row["T"] is not None else CLIP_TEMPS
            grids = [P.U_GRID(row["logits"], n, row["temp_logit"], P.MIN_TEMP, T, size=B * N, seed=b, extra=row["u_extra"]) for b, T in enumerate(temps)]
            uni = torch.stack([g[0][b * N:(b + 1) * N] for b, g in enumerate(grids)])
            on = torch.stack([g[1][b * N:(b + 1) * N] for b, g in enumerate(grids)])
            temp = torch.tensor(temps, dtype=torch.float32)
            picks = run(row, temp, uni)
            check_sampled(row, n, row["temp_logit"], temp[:, None].expand(B, N).reshape(-1), uni.reshape(-1), on.reshape(-1), picks.reshape(-1), tally, what)
        elif row["kind"] == "greedy" or (spec["greedy256"] == "padded" and n <= 256) or (spec["greedy256"] == "at256" and n == 256):
            picks = run(row, None, None)
            want = P.picker_ref(row["logits"], n, row["temp_logit"], P.MIN_TEMP)
            if row["expect"] is not None:
                assert want == row["expect"]
            assert bool((picks == want).all()), (what, row["name"], "greedy", sorted(set(picks.reshape(-1).tolist())), want)
            tally.greedy += picks.numel()
    tally.report(what)
