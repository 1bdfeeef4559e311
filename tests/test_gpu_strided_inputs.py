"""Entry points with a strided input that no family file places: the surround rule of tests/strided_inputs.py on them."""
import numpy as np
import pytest
import torch

from mimikit_amd import native
from tests.f64_bounds import check_written
from tests.strided_inputs import FLOAT_SURROUNDS, Strided, surround_rule

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)


@surround_rule(*FLOAT_SURROUNDS)
def pack_call(w_np, device):
    """mmk_pack_weight_f32 on rows of a wider matrix (ldw = k + PAD, 4 bytes in) into a NaN-surrounded buffer"""
    n, k = w_np.shape
    w = Strided.of(w_np, 1, device)
    size = native.lib().mmk_packed_weight_floats(n, k)
    out = torch.full((size + 8,), float("nan"), dtype=torch.float32, device=device)
    native.check(native.lib().mmk_pack_weight_f32(w.ptr, w.stride, n, k, out.data_ptr() + 16, native.stream_ptr(device)), "mmk_pack_weight_f32")
    mask = torch.zeros(out.shape, dtype=torch.bool)
    mask[4:4 + size] = True
    check_written(out, mask, f"packed {n, k}")
    return out[4:4 + size].clone()


@pytest.mark.parametrize("n,k", [(1, 1), (3, 33), (17, 16), (65, 129)])
def test_pack_weight_rows_of_a_wider_matrix(device, n, k):
    """a row shorter than one 16-float chunk, a tail chunk, whole chunks, more rows than one tile: the packed floats are a permutation of
    the weights and zero padding, so the bits of the contiguous call whatever lies around the rows"""
    w = np.random.default_rng(100 * n + k).standard_normal((n, k)).astype(np.float32)
    got = pack_call(w, device)
    want = native.pack_weight(torch.from_numpy(w).to(device))
    assert torch.equal(got.view(torch.int32), want.view(torch.int32))
    print(f"pack_weight {n} x {k}: worst error / bound 0.000 (bits)")


# ====================================================================================================================== the plans
# The plans read the prompt and the conditioning in place.  Each input is a view of a wider buffer: LEAD elements in front of every clip's
# row and LEAD behind it.  The guards hold zeros (class 0) in one run and decoys in the other - classes of the case that differ from the
# row's first and last, +-1e3 alternating for the conditioning floats; never NaN: a plan's waiting kernels give some NaN payloads a
# meaning (csrc/wavenet_spipe.hip).  Histories and last_logits of the two runs are the same bits, and the guards are what they were.
LEAD = 4                                                     # (16 bytes of floats: the rows keep the alignment of a contiguous tensor's)
WAVENET_PLANS = ("launches", "persist", "chain-cond", "lpipe-cond", "spipe-cond", "bpipe-20")
SRNN_PLANS = ("launches", "resident-gru")


class Guarded:
    """place(host tensor, role) -> a (clips, steps, ...) device view with guards around every clip's row; decoys: what the guards hold"""

    def __init__(self, device, q, decoys):
        self.device, self.q, self.decoys, self.made = device, q, decoys, []

    def __call__(self, x, role):
        clips, cols = x.shape[0], x[0].numel()
        wide = torch.zeros((clips, cols + 2 * LEAD), dtype=x.dtype)
        flat = x.reshape(clips, cols)
        if self.decoys and x.dtype == torch.int64:
            step = torch.arange(1, LEAD + 1)
            wide[:, :LEAD] = (flat[:, :1] + step) % self.q                   # (q > LEAD: none of them is the class beside it)
            wide[:, LEAD + cols:] = (flat[:, -1:] + step) % self.q
        elif self.decoys:
            sign = 1.0 - 2.0 * (torch.arange(2 * LEAD) % 2)
            wide[:, :LEAD], wide[:, LEAD + cols:] = 1e3 * sign[:LEAD], 1e3 * sign[LEAD:]
        wide[:, LEAD:LEAD + cols] = flat
        wide = wide.to(self.device)
        self.made.append((wide, cols, wide.clone()))
        return wide[:, LEAD:LEAD + cols].unflatten(1, tuple(x.shape[1:]))

    def guards_kept(self):
        return all(torch.equal(w[:, :LEAD], b[:, :LEAD]) and torch.equal(w[:, LEAD + c:], b[:, LEAD + c:]) for w, c, b in self.made)


def _same(a, b):
    a, b = (tuple(x) if isinstance(x, (tuple, list)) else (x,) for x in (a, b))
    return len(a) == len(b) and all(x.dtype == y.dtype and torch.equal(x.contiguous().view(torch.int32), y.contiguous().view(torch.int32)) for x, y in zip(a, b))


def _plan_between_decoys(case, device, monkeypatch, what):
    from tests import plan_driver as D
    assert case.q[0] > LEAD + 1
    D.switch(monkeypatch, case)
    runs = []
    for decoys in (False, True):
        place = Guarded(device, case.q[0], decoys)
        runs.append(D.generate(case, device, f"{what}, decoys {decoys}", place=place))
        assert len(place.made) == len(case.q) + case.cond and place.guards_kept(), f"{what}: a guard was written"
    (hist0, dev0), (hist1, dev1) = runs
    first = hist0[0] if isinstance(hist0, (tuple, list)) else hist0
    assert bool(first[:, case.P:].any()), f"{what}: the steps were not written into the placed rows"
    assert _same(hist0, hist1), f"{what}: the history depends on what lies around the rows"
    assert _same(dev0, dev1), f"{what}: last_logits depends on what lies around the rows"
    print(f"{what}: {case.n} steps, {case.clips} clips, {case.cond} conditioning inputs: worst error / bound 0.000 (bits)")


@pytest.mark.parametrize("tag", WAVENET_PLANS)
def test_wavenet_prompt_and_conditioning_in_place_between_decoys(device, monkeypatch, tag):
    from tests import net_refs as R
    _plan_between_decoys({c.id: c for c in R.WAVENET_CASES}[tag], device, monkeypatch, f"wavenet {tag}")


@pytest.mark.parametrize("tag", SRNN_PLANS)
def test_sample_rnn_prompt_in_place_between_decoys(device, monkeypatch, tag):
    from tests import net_refs as R
    _plan_between_decoys({c.id: c for c in R.SRNN_CASES}[tag], device, monkeypatch, f"sample_rnn {tag}")


def test_transformer_prompt_in_place_between_decoys(device):
    """the smallest class case of tests/transformer_refs.py, its blocks as tests/test_gpu_transformer_f64.py runs them"""
    from tests import transformer_refs as TR
    case = next(c for c in TR.CASES if c.classes)
    prompt = case.inputs()
    q = int(prompt.max()) + 1                                 # (classes the prompt itself holds: in range whatever the case's count)
    assert q > LEAD + 1
    runs = []
    for decoys in (False, True):
        net = TR.build_case(case, device)
        place = Guarded(device, q, decoys)
        data = place(torch.cat([prompt, torch.zeros(case.clips, case.n, dtype=prompt.dtype)], 1), "data")
        net.before_generate((data[:, :case.prompt],), None)
        logits, t = [], case.prompt
        for nb in case.parts:
            assert net.generate_block((data,), t, nb) is True
            t += nb
            logits.append(net._plan.last_logits(case.clips).cpu())
        runs.append((data.cpu(), torch.stack(logits, 1)))
        assert place.guards_kept(), "a guard was written"
    assert bool(runs[0][0][:, case.prompt:].any()), "the steps were not written into the placed rows"
    assert _same(runs[0][0], runs[1][0]) and _same(runs[0][1], runs[1][1]), "the transformer's history or logits depend on what lies around the rows"
    print(f"transformer {case.tag}: {case.n} steps: worst error / bound 0.000 (bits)")
