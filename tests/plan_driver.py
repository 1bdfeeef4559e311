"""How test_gpu_networks_f64.py and test_gpu_plan_lives.py drive a case of tests/net_refs.py on the device: the plan switches of the case, then
one generation through the network's own lifecycle (before_generate, generate_block in consecutive calls, after_generate), with the plan's
report of the kernel it took asserted after every block."""
import torch

import mimikit_amd as mmk
from mimikit_amd import native
from tests import net_refs as R

SWITCHES = ("MMK_WN_XCD_LOCAL", "MMK_WN_PERSISTENT", "MMK_WN_GROUPS", "MMK_WN_SMALL", "MMK_WN_PREFILL", "MMK_WN_CHAIN", "MMK_WN_LPIPE", "MMK_WN_SPIPE",
            "MMK_WN_BPIPE", "MMK_WN_PIPE", "MMK_WN_SPIPE_PAIR", "MMK_SRNN_FUSED", "MMK_SRNN_FUSED_UP", "MMK_SRNN_RESIDENT", "MMK_SRNN_RESIDENT_WARMUP",
            "MMK_SRNN_COMPOSED", "MMK_S2S_FUSED", "MMK_S2S_SEQ", "MMK_S2S_COMPOSED", "MMK_GEMM_KSPLIT")


def switch(monkeypatch, case):
    for k in SWITCHES:
        monkeypatch.delitem(mmk.native.PLAN_TUNING, k, raising=False)
    for k, v in case.env.items():
        monkeypatch.setitem(mmk.native.PLAN_TUNING, k, v)


def waits(case, plan):
    """whether the plan's kernels wait for each other (a timed-out wait is then an error sync_status reports)"""
    return plan.persistent if case.kind in ("wavenet", "wavenet_frames") else plan.resident_blocks() if case.kind == "srnn" else plan.resident_launches()


def logits_into(case, plan, clips, out, target=0):
    """last_logits of `clips` clips written into the caller's buffer `out`, which may hold more rows than that"""
    s = native.stream_ptr(plan.device)
    if case.kind == "s2s_classes":
        assert out.is_contiguous()
        native.check(plan._lib.mmk_s2s_last_logits(plan.handle, clips, native.ptr(out), out.shape[-1], s), "mmk_s2s_last_logits")
    else:
        entry = "mmk_wavenet_last_logits_of" if case.kind == "wavenet" else "mmk_srnn_last_logits_of"
        native.check(getattr(plan._lib, entry)(plan.handle, target, clips, native.ptr(out), out.stride(0), s), entry)
    return out


def generate(case, device, what, net=None, blocks_before=0, warmups=1, after_block=None, place=None):
    """the blocks of the case - or of a net_refs.Life of it - on the device -> (history on the host, the outputs the device hands back: (clips,
    compared steps, columns)).  net: the network to run it on (its plan may have generated before: `blocks_before` generate blocks, and
    `warmups` generations with a warm-up of whole periods, this one included - what case.ran counts); None: a fresh one.
    after_block(plan): called after every block, behind its checks.  place(host tensor, 'data' | 'cond') -> the device tensor the plan is
    given for it, a view of a wider buffer for one (tests/test_gpu_strided_inputs.py); None: a contiguous copy"""
    place = place or (lambda x, role: x.to(device))
    net = case.make()[0].to(device) if net is None else net
    prompt, conds = case.inputs()
    B, P, n, hop = case.clips, case.P, case.n, case.hop or 1
    conds_d = tuple(place(c, "cond") for c in conds)
    # one tensor per class stream (or the one of frames): the prompt and blanks - a stream no target feeds is given for the whole length
    data = tuple(place(torch.cat([p, torch.zeros(B, P + n - p.size(1), *p.shape[2:], dtype=p.dtype)], 1), "data") for p in R.streams(prompt))
    if case.kind in ("srnn", "s2s", "s2s_classes"):
        net.before_generate(tuple(x[:, :P] for x in data), None)
        if case.kind == "srnn" and "MMK_SRNN_RESIDENT_WARMUP" in case.env:
            assert case.ran(net._plan, blocks_before, warmups), (what, "the warm-up took another path", net._plan.resident_warmups())
    rows, t = [[] for _ in range(case.targets)], P
    for k, nb in enumerate(case.parts, blocks_before + 1):
        if case.kind == "s2s" and conds_d:
            # several frame inputs: the network adds them up and has no block path (generate_block declines), so step by step as the loop does
            assert nb == 1 and net.generate_block((*data, *conds_d), t, hop) is None
            data[0][:, t:t + hop] = net.generate_step(tuple(x[:, t - hop:t] for x in (*data, *conds_d)), t=t)
        else:
            assert net.generate_block((*data, *conds_d), t, nb * hop)
        t += nb * hop
        plan = net._plan
        assert case.ran(plan, k, warmups), (what, f"block {k}: the plan took another kernel", R.flags(case, plan))
        if waits(case, plan):
            plan.sync_status()                     # (the workgroups of these kernels wait for each other: a timed-out wait is an error here)
        if case.kind == "s2s_classes":
            rows[0].append(plan.last_logits(B).cpu())
        elif case.classes:
            for target in range(case.targets):
                rows[target].append(plan.last_logits(B, target).cpu())
        if after_block is not None:
            after_block(plan)
    net.after_generate(data, None)
    hist = tuple(x.cpu() for x in data)
    if not case.classes:
        return hist[0], hist[0][:, P:]
    dev = [torch.cat(r, 1) if case.kind == "s2s_classes" else torch.stack(r, 1) for r in rows]
    return (hist, dev) if case.multi else (hist[0], dev[0])
