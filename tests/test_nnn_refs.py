"""NearestNextNeighbor without a GPU: the class and its event wiring exist, native mirrors the header's constants, include/mmk.h declares the
entry points, and the restatements of tests/nnn_refs.py are what they claim - a DTW worked by hand, first-minimum ties, the diagonal sweep
against the cell-by-cell loop, the cosine distance against sklearn's, and the planted cases well-posed in float64."""
import os
import re

import numpy as np
import pytest
import torch

import mimikit_amd as mmk
from mimikit_amd import native
from mimikit_amd.models import NearestNextNeighbor
from tests import nnn_refs as R

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "mmk.h")


def test_constants_mirror_the_header():
    text = open(HEADER).read()
    for name, value in (("MMK_NNN_MAX_ROWS", native.NNN_MAX_ROWS), ("MMK_NNN_ROW_PAD", native.NNN_ROW_PAD),
                        ("MMK_NNN_LOOKAHEAD", native.NNN_LOOKAHEAD)):
        found = re.search(rf"#define {name} (\d+)", text)
        assert found and int(found.group(1)) == value, name
    assert native.NNN_MAX_ROWS == 64 and native.NNN_MAX_ROWS % native.NNN_ROW_PAD == 0
    assert [native.nnn_n_pad(n) for n in (1, 16, 17, 63, 64)] == [16, 16, 32, 64, 64]
    assert "#define MMK_ABI_VERSION 6" in text and native.ABI_VERSION == 6


def test_header_declares_the_entry_points():
    text = open(HEADER).read()
    for name in ("mmk_inv_row_norm_f32", "mmk_cosine_cost_f32", "mmk_dtw_subseq_f32"):
        assert re.search(rf"\bint {name}\(", text), name
        assert name in native.EXPORTED_SYMBOLS


def test_event_accepts_a_nearest_next_neighbor():
    frames = torch.rand(12, 129)
    nnn = NearestNextNeighbor.from_frames(frames, feature=mmk.MagSpec(256, 64), sr=16000)
    assert mmk.NearestNextNeighbor is NearestNextNeighbor and nnn.shift == 16 and (nnn.n_frames, nnn.n_bins) == (12, 129)
    ev = mmk.Event(generator=nnn, seconds=0.1, temperature=0.5)
    assert ev.network() is nnn
    with pytest.raises(ValueError, match="sample rate"):
        mmk.Event(generator=NearestNextNeighbor.from_frames(frames, feature=mmk.MagSpec(256, 64)), seconds=0.1)
    with pytest.raises(ValueError, match="feature"):
        mmk.Event(generator=NearestNextNeighbor.from_frames(frames, sr=16000), seconds=0.1)
    with pytest.raises(TypeError):
        mmk.Event(generator=object(), seconds=0.1).network()


def test_class_refuses_what_it_does_not_align():
    nnn = NearestNextNeighbor.from_frames(torch.rand(12, 5))
    with pytest.raises(NotImplementedError, match="65.*64"):
        nnn.predict_start_frames(torch.rand(2, 65, 5))
    with pytest.raises(ValueError, match="bins"):
        nnn.predict_start_frames(torch.rand(2, 4, 6))
    with pytest.raises(ValueError):
        NearestNextNeighbor.from_frames(torch.rand(0, 5))
    with pytest.raises(ValueError):
        NearestNextNeighbor(mmk.MagSpec(256, 64), torch.rand(2, 100))
    with pytest.raises(RuntimeError):                      # no CPU fallback
        nnn.predict_start_frames(torch.rand(2, 4, 5))


def test_dtw_worked_by_hand():
    C = np.array([[1, 3, 0, 2, 1],
                  [2, 0, 4, 1, 1],
                  [3, 2, 1, 0, 5]], dtype=np.float64)
    # row 0 = C[0]; column 0 accumulates; the rest: C + min(diagonal, left, up)
    want = np.array([[1, 3, 0, 2, 1],
                     [3, 1, 4, 1, 2],
                     [6, 3, 2, 1, 6]], dtype=np.float64)
    assert np.array_equal(R.dtw_subseq(C), want)
    assert np.array_equal(R.dtw_last_row(C), want[-1])
    assert R.end_column(want[-1]) == 3
    assert np.array_equal(R.dtw_subseq(C.astype(np.float32)), want.astype(np.float32))


def test_first_minimum_wins_a_tie():
    C = np.ones((4, 9))
    assert np.array_equal(R.dtw_last_row(C), np.full(9, 4.0)) and R.end_column(R.dtw_last_row(C)) == 0
    C = np.ones((3, 12))
    for o in (2, 7):                                       # the same zero-cost diagonal twice
        C[np.arange(3), o + np.arange(3)] = 0
    last = R.dtw_last_row(C)
    assert last[4] == 0 and last[9] == 0 and R.end_column(last) == 4


@pytest.mark.parametrize("dtype", (np.float32, np.float64))
def test_sweep_is_the_loop_bit_for_bit(dtype):
    rng = np.random.default_rng(3)
    for n, m in ((1, 1), (1, 7), (5, 1), (2, 2), (7, 3), (3, 7), (16, 33), (17, 5)):
        C = rng.uniform(0, 2, size=(2, n, m)).astype(dtype)
        last = R.dtw_last_row(C)
        assert last.dtype == dtype
        for b in range(2):
            assert np.array_equal(last[b], R.dtw_subseq(C[b])[-1]), (n, m)


def test_float32_loop_within_the_dtw_bound_of_float64():
    rng = np.random.default_rng(4)
    for n, m in ((1, 9), (16, 64), (64, 17), (63, 257)):
        C = rng.uniform(0, 2, size=(n, m)).astype(np.float32)
        l32, l64 = R.dtw_last_row(C), R.dtw_last_row(C.astype(np.float64))
        assert not R.outside(l32, l64, R.dtw_bound(l64, n, 0.0)).any(), (n, m)


def test_cosine_restatement_against_sklearn():
    pairwise_distances = pytest.importorskip("sklearn.metrics").pairwise_distances
    for (batch, n, m, k) in ((1, 2, 63, 3), (3, 16, 65, 513), (1, 64, 2, 4)):
        x, y, want, _ = R.cost_case(batch, n, m, k)
        assert (np.abs(y).sum(-1) == 0).any() and (n == 1 or (np.abs(x).sum(-1) == 0).any())
        for b in range(batch):
            ref = pairwise_distances(np.abs(x[b]).astype(np.float64), np.abs(y).astype(np.float64), metric="cosine")
            assert np.abs(ref - want[b]).max() <= 1e-14
    zero = R.cosine_distances(np.zeros((1, 4)), np.ones((2, 4)))
    assert np.array_equal(zero, np.ones((1, 2)))


def test_cost_bound_holds_for_a_float32_restatement():
    """the kernel's arithmetic in numpy float32 (a sequential sum, not its order): inside the derived bound, so the bound is not vacuous-tight"""
    for (batch, n, m, k) in ((3, 16, 65, 513), (1, 63, 64, 1025), (1, 2, 2, 1)):
        x, y, want, bound = R.cost_case(batch, n, m, k)
        ax, ay = np.abs(x), np.abs(y)

        def inv(a):
            s = np.sqrt((a * a).sum(-1, dtype=np.float32))
            return np.divide(np.float32(1), s, out=np.zeros_like(s), where=s > 0)
        got = np.clip(np.float32(1) - (ax @ ay.T) * inv(ax)[..., None] * inv(ay)[None, None, :], 0, 2)
        assert got.dtype == np.float32 and not R.outside(got, want, bound).any()
        assert bound.max() <= R.gamma(2 * k + 12) * (1 + 1e-12) + R.U


@pytest.mark.parametrize("index", range(len(R.PLANTED)))
def test_planted_cases_are_well_posed(index):
    """in float64 alone: the planted end is the minimum, and the best column outside the planted segment is further than twice the bound"""
    _, _, last64, ends = R.planted_case(index)
    assert np.array_equal(R.end_column(last64), ends)
    gaps, twice = R.planted_gap(index)
    assert (gaps > twice).all(), (gaps, twice)
