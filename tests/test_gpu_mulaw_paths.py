"""The mu-law kernels on the device against the reference project's fp32 formula, on the crafted data of tests/mulaw_refs.py: every
threshold with its neighbours, at the lengths where mmk_mulaw_compress_f32_i64 changes kernels (csrc/features.hip) - one below the stream
kernel's threshold, on it, the three tail hand-offs, a partial last wave, whole waves past the end, and one input past the stream
kernel's grid cap.  In-range codes are exact at every q, 4096 and 65536 included; the oracle and the thresholds are computed on this host."""
import numpy as np
import pytest
import torch

from mimikit_amd import native
from mimikit_amd.features.functionals import mulaw_table
from oracle import torch_ref as O
from tests import mulaw_refs as R

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)
IDS = [f"q{q}-c{c}" for q, c in R.CASES]


def _kept(x, want, edges, what):
    """inputs on which this host's oracle and its threshold search agree (all of them, wherever this was measured); the share that is dropped
    is printed, and more than 0.1 % fails"""
    keep = want == torch.bucketize(x, edges, right=True)
    share = 1.0 - float(keep.double().mean())
    print(f"{what}: excluded share {share:.4%} ({int((~keep).sum())} of {keep.numel()} inputs)")
    assert share <= 1e-3
    return keep


def _compress_raw(x, q, c, edges):
    """through the C ABI, `edges` may be None"""
    out = torch.empty(x.shape, dtype=torch.int64, device=x.device)
    native.check(native.lib().mmk_mulaw_compress_f32_i64(native.ptr(x), native.ptr(out), x.numel(), q, c, native.ptr(edges),
                                                         native.stream_ptr(x.device)), "mmk_mulaw_compress_f32_i64")
    return out


@pytest.mark.parametrize("q,c", R.CASES, ids=IDS)
def test_codes_equal_the_oracle_at_every_length(device, q, c):
    d = R.crafted(q, c)
    keep = _kept(d.x, d.want, d.edges, f"mu-law q={q} c={c}").to(device)
    x, want, edges = d.x.to(device), d.want.to(device), d.edges.to(device)
    assert x.data_ptr() % 16 == 0
    got = {}
    for n in d.lengths:
        got[n] = native.mulaw_compress(x[:n], q, c, edges)
        assert got[n].dtype == torch.int64 and got[n].shape == (n,) and got[n].data_ptr() % 16 == 0
        bad = (got[n] != want[:n]) & keep[:n]
        if bool(bad.any()):
            i = int(bad.nonzero()[0])
            raise AssertionError(f"n={n}: {int(bad.sum())} codes differ from the oracle's; first at sample {i} (float4 {i // 4}, lane {(i // 4) % 64}): "
                                 f"x={float(x[i])!r}, got {int(got[n][i])}, want {int(want[i])}")
    a, b = R.LENGTHS[0], R.LENGTHS[1]          # the general kernel and the stream kernel on the same data
    assert torch.equal(got[a], got[b][:a])


def test_codes_equal_the_oracle_past_the_grid_cap(device):
    """n4 = 8192 x 1024 + 64 x 5 + 3: workgroup 0 of the stream kernel makes a second trip, five whole waves and a partial one; one sample for
    the general kernel.  The shuffled block is tiled on the device, the expected codes the same way: only the block crosses the bus"""
    q, c = 4096, 1.0
    d = R.crafted(q, c)
    keep = _kept(d.block, d.block_want, d.edges, f"mu-law q={q} c={c}, the block").to(device)
    reps = -(-R.GRID_CAP_N // d.block.numel())
    x = d.block.to(device).repeat(reps)[:R.GRID_CAP_N]
    got = native.mulaw_compress(x, q, c, d.edges.to(device))
    want = d.block_want.to(device).repeat(reps)[:R.GRID_CAP_N]
    bad = (got != want) & keep.repeat(reps)[:R.GRID_CAP_N]
    if bool(bad.any()):
        i = int(bad.nonzero()[0])
        raise AssertionError(f"{int(bad.sum())} codes differ; first at sample {i} (float4 {i // 4} of {R.GRID_CAP_N4}): got {int(got[i])}, want {int(want[i])}")


@pytest.mark.parametrize("n", [R.LENGTHS[4], R.PARTIAL_WAVE_N])
@pytest.mark.parametrize("q", [256, 4096])
def test_out_of_range_samples_among_lanes_that_exchange(device, q, n):
    """single samples outside [-1, 1], infinite or NaN (mulaw_refs.pokes): their wave keeps its own stores for that round, the waves around
    it exchange.  Every other sample stays exact; a finite out-of-range sample is within one code of the oracle (the bar of
    test_mulaw_golden_bit_exact: the direct formula with the device's log1pf) and negative where the oracle's is - a negative code must not go
    through the 16-bit exchange.  The codes of +-inf and NaN are not compared: the conversion is undefined on both sides."""
    c = 1.0
    d = R.crafted(q, c)
    x = d.x[:n].clone()
    pokes = R.pokes(n)
    at = torch.tensor([s for s, _ in pokes])
    x[at] = torch.tensor([v for _, v in pokes], dtype=torch.float32)
    want = O.mulaw_compress(x, q, c)               # one call over the whole tensor, as everywhere
    keep = _kept(d.x[:n], d.want[:n], d.edges, f"mu-law q={q} n={n}")
    keep[at] = False
    assert torch.equal(want[keep], d.want[:n][keep])
    got = native.mulaw_compress(x.to(device), q, c, d.edges.to(device)).cpu()
    bad = (got != want) & keep
    if bool(bad.any()):
        i = int(bad.nonzero()[0])
        raise AssertionError(f"{int(bad.sum())} untouched samples differ; first at sample {i} (float4 {i // 4}, lane {(i // 4) % 64}): got {int(got[i])}, "
                             f"want {int(want[i])}")
    finite = torch.isfinite(x[at])
    assert int(finite.sum()) == sum(np.isfinite(v) for _, v in pokes) >= 48
    g, w = got[at][finite], want[at][finite]
    print(f"mu-law q={q} n={n}: out-of-range codes, device - oracle: {sorted(set((g - w).tolist()))}; {int((w < 0).sum())} negative")
    assert int((g - w).abs().max()) <= 1, (x[at][finite][(g - w).abs() > 1].tolist(), g.tolist(), w.tolist())
    assert bool((w < 0).any()) and bool((g[w < 0] < 0).all())
    assert bool((w >= q).any())                    # and codes beyond the table, which the reference does not clamp


def test_no_table(device):
    """edges = NULL: the direct formula with the device's log1pf, 65539 samples.  Within one code of the oracle everywhere, equal wherever
    the sample lies more than 8 places of the fp32 number line from every threshold.  The crafted samples all lie within 2 places, so every
    second sample is replaced by a uniform random one; q = 256 and compression 1, the package's defaults"""
    q, c, n = 256, 1.0, R.LENGTHS[4]
    d = R.crafted(q, c)
    x = d.x[:n].clone()
    x[1::2] = (torch.rand(n // 2, generator=torch.Generator().manual_seed(5)) * 2 - 1)
    want = O.mulaw_compress(x, q, c)
    keep = _kept(x, want, d.edges, f"mu-law q={q}, no table")
    got = _compress_raw(x.to(device), q, c, None).cpu()
    far = torch.from_numpy(R.ulp_distance(x.numpy(), d.edges.numpy()) > 8)
    diff = (got - want)[keep]
    print(f"mu-law q={q}, no table: {int((diff != 0).sum())} of {diff.numel()} codes differ by one, {int(((got != want) & far & keep).sum())} of them "
          f"among the {int(far.sum())} samples more than 8 places from a threshold")
    assert int(far.sum()) > n // 3
    assert int(diff.abs().max()) <= 1
    assert torch.equal(got[far & keep], want[far & keep])


@pytest.mark.parametrize("q,n", [(256, 65537), (8192, 65537), (65536, 131073)])
def test_expand_views_and_codes_outside_the_table(device, q, n):
    """all q codes and -2, -1, q, q + 1 among them, an odd n; the 16-byte path, views one element off it, and no table at all"""
    c = 1.0
    codes = R.expand_codes(q, n)
    want = O.mulaw_expand(codes, q, c)
    inside = (codes >= 0) & (codes < q)
    table = mulaw_table(q, c)
    assert torch.equal(want[inside], table[codes[inside]])
    table = table.to(device)
    cbuf, obuf = torch.zeros(n + 1, dtype=torch.int64, device=device), torch.zeros(n + 1, dtype=torch.float32, device=device)
    assert cbuf.data_ptr() % 16 == 0 and obuf.data_ptr() % 16 == 0
    for coff, ooff, tab in ((0, 0, table), (1, 1, table), (0, 1, table), (0, 0, None), (1, 1, None)):
        cv, ov = cbuf[coff:coff + n], obuf[ooff:ooff + n]
        cbuf.fill_(0)
        obuf.fill_(float("nan"))
        cv.copy_(codes)
        native.check(native.lib().mmk_mulaw_expand_i64_f32(native.ptr(cv), native.ptr(ov), n, q, c, native.ptr(tab), native.stream_ptr(device)),
                     "mmk_mulaw_expand_i64_f32")
        got = ov.cpu()
        what = f"codes +{coff}, output +{ooff}, {'table' if tab is not None else 'no table'}"
        if tab is not None:
            assert torch.equal(got[inside], want[inside]), what
            assert torch.allclose(got[~inside], want[~inside], rtol=1e-5, atol=1e-7), what
        else:
            assert torch.allclose(got, want, rtol=1e-5, atol=1e-7), what
        rest = torch.cat([obuf[:ooff], obuf[ooff + n:]]).cpu()
        assert bool(torch.isnan(rest).all()), what + ": wrote outside its output"
    assert torch.equal(native.mulaw_expand(codes.to(device), q, c, table).cpu()[inside], want[inside])
