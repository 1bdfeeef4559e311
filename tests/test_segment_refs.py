"""The float64 restatements and bounds of tests/segment_refs.py against the reference's own results (tests/golden/segment.npz, recorded from
mimikit/extract/segment.py by tests/golden/make_golden_segment.py) and against sklearn, the defects the bounds must catch, and the
robustness of every input the GPU cut tests use.  No GPU."""
import os
import re

import numpy as np
import pytest
from sklearn.metrics import pairwise_distances

import mimikit_amd as mmk
from mimikit_amd import build, native
from tests import segment_refs as R
from tests.golden import make_golden_segment as M

G = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "segment.npz"))


def test_checker_and_convolution_equal_the_reference():
    for h in M.CHECKERS:
        assert np.array_equal(R.checker64(h), G[f"checker_{h}"])
    for name, (_, h, n) in M.CONV.items():
        got = R.convolve_diagonals64(G[f"conv_{name}_diagonals"], R.checker64(h))
        assert got.shape == (n,) and np.abs(got - G[f"conv_{name}_out"]).max() <= 1e-12


@pytest.mark.parametrize("name", sorted(M.BANDS))
def test_band_and_raw_equal_the_reference(name):
    _, h, t, _ = M.BANDS[name]
    x = G[f"band_{name}_x"]
    assert x.shape[0] == t <= 2 * h and not x[t // 2].any()
    band = R.band64(x, 2 * h + 1)
    assert np.abs(band - G[f"band_{name}_diagonals"]).max() <= 1e-12
    sk = pairwise_distances(x.astype(np.float64), metric="cosine")
    assert np.abs(R.dist64(x) - sk).max() <= 1e-12
    for i in range(t):
        for j in range(t):
            assert abs(band[i, 2 * h + 1 + j - i] - sk[i, j]) <= 1e-12
    for hq in (h, M.BAND_SMALL[name]):
        want = G[f"band_{name}_raw_{hq}"]
        assert np.abs(R.raw64(x, hq) - want).max() <= 1e-12                      # the direct double sum
        assert np.abs(R.raw_by_parts(x, hq, h) - want).max() <= 1e-12             # the reference's assembly from the restated parts


def test_direct_sum_equals_the_assembly_beyond_the_reference_sizes():
    """T > k - 1, where the reference's pwdk_cosine cannot run outside numba: the restated parts, assembled as segment.py:120-130 does,
    equal the direct double sum over the (T, T) matrix"""
    x = R.frames_case(R.TILE + 1, 33)[0]
    for h, h_max in ((1, 6), (6, 6), (6, 12), (R.MAX_HALF, R.MAX_HALF)):
        assert np.abs(R.raw64(x, h) - R.raw_by_parts(x, h, h_max)).max() <= 1e-12


@pytest.mark.parametrize("defect", ["centre_ii", "no_diag_zero", "zero_row_d0", "edge_pad"])
def test_bound_catches(defect):
    x = R.frames_case(2 * R.TILE + 3, 33)[0]
    assert not x[0].any() and not x[x.shape[0] // 2].any()
    for halves in ([6], [1, 6, R.MAX_HALF]):
        raw, scores, dg, rb, sb, gb = R.bounds(x, halves)
        raw_d, scores_d, dg_d = R.scores64(x, halves, defect)
        q = halves.index(6)
        assert R.outside(raw_d[q], raw[q], rb[q]).any(), f"{defect}: raw stays inside the bound - the bound is too loose"
        assert R.outside(scores_d[q], scores[q], sb[q]).any() and R.outside(dg_d, dg, gb).any()


@pytest.mark.parametrize("T", R.TS)
def test_fp32_numpy_stays_inside(T):
    for D in R.DS:
        x = R.frames_case(T, D)[0]
        for halves in R.HALVES:
            raw, _, _, rb, _, _ = R.bounds(x, halves)
            for q, h in enumerate(halves):
                R.assert_inside(R.raw32_numpy(x, h), raw[q], rb[q], f"fp32 numpy T {T} D {D} h {h}")


def test_cut_inputs_are_robust():
    x = R.corpus_case()
    assert x.shape == (293, 33) and (x >= 0).all()
    for halves in (R.CORPUS_HALVES, [int(f * 6) for f in (1., 2.)], [6]):
        _, _, dg, _, _, gb = R.bounds(x, halves)
        assert R.robust(dg, gb, R.CORPUS_MIN_DUR, R.CORPUS_MIN_DUR, R.CORPUS_MIN_STRENGTH), halves
        assert R.cuts64(dg, R.CORPUS_MIN_DUR, R.CORPUS_MIN_STRENGTH).tolist() == R.CORPUS_BOUNDS, halves
    assert not R.robust(dg, 0.1 * dg.max(), R.CORPUS_MIN_DUR, R.CORPUS_MIN_DUR, R.CORPUS_MIN_STRENGTH)
    for name, (_, n, wb, wa, ms) in M.PICKS.items():
        assert R.robust(G[f"pick_{name}_x"].astype(np.float64), 1e-9, wb, wa, ms), name


def test_picker_equals_the_reference():
    for name, (_, n, wb, wa, ms) in M.PICKS.items():
        x = G[f"pick_{name}_x"]
        assert x.dtype == np.float32 and x.shape == (n,)
        assert np.array_equal(R.picker64(x, wb, wa, ms), G[f"pick_{name}_out"]), name
    # equal values: the lower index first; a constant series: nothing
    x = np.array([0, 3, 0, 3, 0, 0, 0, 0], dtype=np.float64)
    assert R.picker64(x, 3, 3, 0.02).tolist() == [1] and R.picker64(np.ones(9), 2, 2).tolist() == []
    c = R.constant_case()
    _, _, dg = R.scores64(c, [6, 12])
    assert not dg.any() and R.cuts64(dg, 4, 0.03).tolist() == []


def test_exports_and_constants():
    header = open(os.path.join(os.path.dirname(native._HERE), "include", "mmk.h")).read()
    for name in ("TILE", "MAX_KERNELS", "MAX_HALF", "MAX_WAIT"):
        assert f"#define MMK_NOVELTY_{name} {getattr(native, 'NOVELTY_' + name)}\n" in header
    assert native.NOVELTY_MAX_HALF == 32 and native.NOVELTY_MAX_KERNELS == 8
    assert int(re.search(r"#define MMK_ABI_VERSION (\d+)", header).group(1)) == native.ABI_VERSION
    assert "novelty.hip" in build.SOURCES
    lib = native.load_library()
    for sym in ("mmk_novelty_f32", "mmk_novelty_finish_workspace_floats", "mmk_novelty_finish_f32", "mmk_pick_peaks_workspace_bytes",
                "mmk_pick_peaks_f32"):
        assert sym in native.EXPORTED_SYMBOLS and hasattr(lib, sym) and f" {sym}(" in header
    assert lib.mmk_novelty_finish_workspace_floats(2, 3, 4097) == 12 and lib.mmk_pick_peaks_workspace_bytes(10) == 48
    for name in ("discontinuity_scores", "pick_globally_sorted_maxes", "from_recurrence_matrix", "CutsFromRecurrenceMatrix"):
        assert name in mmk.extract.segment.__all__ and getattr(mmk, name) is getattr(mmk.extract.segment, name)
    assert mmk.CutsFromRecurrenceMatrix(6, [1., 2.]).kernel_sizes == [6, 12]


def test_argument_checks_need_no_device():
    import torch
    x = torch.zeros(10, 4)
    with pytest.raises(ValueError):
        mmk.discontinuity_scores(torch.zeros(1, 4), [6])
    with pytest.raises(TypeError):
        native.novelty(x.double(), [6])
    with pytest.raises(NotImplementedError):
        native.novelty(x, [native.NOVELTY_MAX_HALF + 1])
    with pytest.raises(NotImplementedError):
        native.novelty(x, [1] * (native.NOVELTY_MAX_KERNELS + 1))
    with pytest.raises(ValueError):
        native.novelty(x, [0])
    with pytest.raises(NotImplementedError):
        native.pick_peaks(x[:, 0], native.NOVELTY_MAX_WAIT + 1, 1)
    with pytest.raises(Exception):
        native.novelty(x, [6])            # a CPU tensor: no CPU path
