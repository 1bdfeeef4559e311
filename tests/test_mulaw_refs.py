"""CPU side of the mu-law kernels' tests: what tests/mulaw_refs.py hands test_gpu_mulaw_paths.py must hold for the reference alone.

The oracle (the reference project's fp32 formula, one call per tensor) equals a binary search over functionals.mulaw_edges on every
crafted input; the float64 formula is within one code of it and is not the contract; the crafted data leaves no room for a misdirected
exchange or a shifted store to hide (named defects, applied to the expected codes); and the dispatch thresholds the cases rely on are the
ones in csrc/features.hip."""
import os
import re

import numpy as np
import pytest
import torch

from oracle import torch_ref as O
from tests import mulaw_refs as R

HERE = os.path.dirname(os.path.abspath(__file__))
SOURCE = os.path.join(os.path.dirname(HERE), "mimikit_amd", "csrc", "features.hip")
IDS = [f"q{q}-c{c}" for q, c in R.CASES]


def test_number_line_steps():
    x = np.array([0.0, -0.0, 1e-45, -1e-45, 1.0, -1.0, 0.5], dtype=np.float32)
    assert np.array_equal(R.from_key(R.ordered_key(x))[2:], x[2:]) and (R.ordered_key(x)[:2] == 0).all()
    up = np.array([1e-45, 1e-45, 3e-45, 0.0, 1.0, np.nextafter(np.float32(-1), np.float32(0)), np.nextafter(np.float32(0.5), np.float32(1))],
                  dtype=np.float32)
    assert np.array_equal(R.step(x, 1), up)
    assert R.step(x, -2)[2] == np.float32(-1e-45) and R.step(x, -1)[5] == -1.0            # through zero; clamped
    e = np.array([-0.5, 0.25], dtype=np.float32)
    assert R.ulp_distance(R.step(e, 3), e).tolist() == [3, 3] and R.ulp_distance(R.step(e, -9), e).tolist() == [9, 9]


@pytest.mark.parametrize("q,c", R.CASES, ids=IDS)
def test_oracle_equals_the_threshold_search(q, c):
    """every threshold with its neighbours up to +-8 ulp, the special values and 4096 random samples: 0 mismatches"""
    d = R.crafted(q, c)
    e = d.edges
    assert e.dtype == torch.float32 and e.numel() == q - 1 and bool((e[1:] > e[:-1]).all()), "the edges are not strictly ascending"
    assert float(e.min()) > -1.0 and float(e.max()) <= 1.0
    wide = torch.from_numpy(R.crafted_block(q, c, ulps=8))
    rand = torch.rand(4096, generator=torch.Generator().manual_seed(q)) * 2 - 1
    for name, x in (("+-8 ulp", wide), ("random", rand), ("master", d.x)):
        assert bool((x.abs() <= 1).all())
        want = O.mulaw_compress(x, q, c)
        assert int((want != torch.bucketize(x, e, right=True)).sum()) == 0, name
        assert int(want.min()) >= 0 and int(want.max()) <= q - 1
        assert int((R.float64_codes(x, q, c) - want).abs().max()) <= 1, name
    differ = float((R.float64_codes(wide, q, c) != O.mulaw_compress(wide, q, c)).double().mean())
    print(f"mu-law q={q} c={c}: the float64 formula differs from the contract on {differ:.1%} of the +-8 ulp neighbours")


@pytest.mark.parametrize("q,c", R.CASES, ids=IDS)
def test_crafted_data_asks_for_every_code_and_neighbours_differ(q, c):
    d = R.crafted(q, c)
    assert d.x.numel() >= R.L_MAX and d.block.numel() == 5 * (q - 1) + 8
    assert torch.equal(torch.sort(d.x[:d.block.numel() * (d.x.numel() // d.block.numel())].view(torch.int32)).values,
                       torch.sort(d.block.view(torch.int32).repeat(d.x.numel() // d.block.numel())).values)      # tiled, -0 and all
    assert torch.equal(torch.bincount(d.block_want, minlength=q) > 0, torch.ones(q, dtype=torch.bool))
    # the shortest length already asks for every code while the block fits into it; beyond, the whole master is one of the lengths
    shortest = d.want[:min(d.lengths)] if q <= R.LDS_LEVELS + 1 else d.want
    assert int((torch.bincount(shortest, minlength=q) == 0).sum()) == 0
    assert (max(d.lengths) == d.x.numel()) == (q > R.LDS_LEVELS)
    shares = R.same_code_shares(d.want[:R.L_MAX])
    print(f"mu-law q={q} c={c}: same code {', '.join(f'{off}: {s:.2%}' for off, s in shares.items())} samples on")
    if q >= 64:
        assert max(shares.values()) <= 0.02, shares
        tiled = R.same_code_shares(d.block_want.repeat(3))               # the grid-capped input: the shuffled block, tiled
        assert max(tiled.values()) <= 0.02, tiled


@pytest.mark.parametrize("q,c", R.STREAM_CASES, ids=[f"q{q}-c{c}" for q, c in R.STREAM_CASES])
def test_defects_cannot_hide(q, c):
    """each defect changes at least one expected code in every whole window of 256 samples, at every length"""
    d = R.crafted(q, c)
    for n in R.LENGTHS:
        for name, defect in R.DEFECTS.items():
            if name == "high_byte_lost" and q != 4096:
                continue
            got = defect(d, n)
            assert got.shape == (n,)
            per_window = R.changed_per_window(got, d.want[:n])
            assert int(per_window.min()) >= 1, f"{name} at n={n}: a window of 256 samples in which it changes nothing"
        if n >= R.STREAM_MIN_N and n & 3 and q >= 64:
            # the tail hand-off: one to three samples, so one to three chances - with 2 or 3 levels they can agree by accident, from 64 levels
            # on the seeded data does not
            assert not torch.equal(R.defect_tail_from_start(d, n), d.want[:n]), f"tail_from_start at n={n}"


def test_lengths_reach_the_paths_they_are_named_for():
    assert R.LENGTHS[0] < R.STREAM_MIN_N == R.LENGTHS[1] and [n & 3 for n in R.LENGTHS[1:5]] == [0, 1, 2, 3]
    n4 = R.PARTIAL_WAVE_N >> 2
    assert n4 % 64 == 37 and R.PARTIAL_WAVE_N & 3 == 2 and n4 // 64 == 256
    n4 = R.WAVES_PAST_END_N >> 2
    assert n4 % R.STREAM_TILE == 192 and n4 % 64 == 0                    # the last workgroup: three waves of round 0, nothing after
    assert -(-R.GRID_CAP_N4 // R.STREAM_TILE) > R.STREAM_GRID_CAP        # capped: workgroup 0 makes a second trip
    assert (R.GRID_CAP_N4 - R.STREAM_GRID_CAP * R.STREAM_TILE) == 64 * 5 + 3 and R.GRID_CAP_N & 3 == 1
    assert R.GRID_CAP_N < 2 ** 31
    for q, c in R.CASES:
        assert (q <= R.STREAM_MAX_Q) == ((q, c) in R.STREAM_CASES)
    assert [q for q, _ in R.CASES if R.STREAM_MAX_Q < q <= R.LDS_LEVELS] == [4097, 8192] and [q for q, _ in R.CASES if q > R.LDS_LEVELS] == [8193, 65536]
    for n in (R.LENGTHS[4], R.PARTIAL_WAVE_N):
        p = R.pokes(n)
        assert len({s for s, _ in p}) == len(p) and all(0 <= s < n for s, _ in p)
        rounds = {s // 256 for s, _ in p}
        assert 255 in rounds and len(rounds) >= len(R.POKE_VALUES) * 8 and ((n >> 2) % 64 == 0 or 256 in rounds)
        assert {(s // 4) % 64 for s, _ in p} >= set(R.POKE_LANES) and {s % 4 for s, _ in p if s < 4 * 16384} == set(R.POKE_COMPONENTS)


def test_dispatch_thresholds_are_the_kernels():
    """the constants the cases are built on, read from the dispatcher's text: a changed threshold fails here instead of silently moving
    the cases to the other kernel"""
    text = open(SOURCE).read()
    start = text.index('extern "C" int mmk_mulaw_compress_f32_i64')
    body = text[start:text.index('extern "C"', start + 10)]
    assert int(re.search(r"constexpr int kMuLawLdsLevels = (\d+);", text).group(1)) == R.LDS_LEVELS == 8192
    cond = re.search(r"if \(edges && aligned && q_levels <= kMuLawLdsLevels / (\d+) && n >= \(1 << (\d+)\)\)", body)
    assert cond, "the stream kernel's dispatch condition changed"
    assert R.LDS_LEVELS // int(cond.group(1)) == R.STREAM_MAX_Q and 1 << int(cond.group(2)) == R.STREAM_MIN_N
    cap = re.search(r"sblocks = \(n4 \+ (\d+)\) / (\d+);\s*sblocks = sblocks > (\d+) \? (\d+) : sblocks;", body)
    assert cap and int(cap.group(1)) + 1 == int(cap.group(2)) == R.STREAM_TILE and int(cap.group(3)) == int(cap.group(4)) == R.STREAM_GRID_CAP
    assert "x += n4 * 4; codes += n4 * 4; n &= 3;" in body                  # the tail hand-off the lengths 65537 .. 65539 are for
    assert "q_levels <= kMuLawLdsLevels ? q_levels : 1" in body             # the general kernel's table: LDS up to LDS_LEVELS


def test_expand_codes():
    for q, n in ((256, 65537), (8192, 65537), (65536, 131073)):
        codes = R.expand_codes(q, n)
        assert codes.numel() == n and n % 2 == 1 and n >= 65537
        assert set(codes[(codes < 0) | (codes >= q)].tolist()) == {-2, -1, q, q + 1}
        assert int((torch.bincount(codes[(codes >= 0) & (codes < q)], minlength=q) == 0).sum()) == 0
