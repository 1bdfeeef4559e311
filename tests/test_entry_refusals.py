"""The refusals of the feature and corpus entry points, pinned: return code AND the whole text of mmk_last_error().

The host half of these entry points (alignment tests, the workspace refusal, the shared row checks) goes through csrc/entry_util.h.  Every
row below is a call that one of those checks - or a check that stands in front of one, so that a changed ORDER shows - refuses before
any launch: the pointers are host memory, and the expected code is never 0 (it ran) or -2 (it reached the HIP runtime).  The texts are
literals recorded from the library as it was before entry_util.h existed; a row that changes is a changed contract, not a stale test.

No GPU is needed: nothing here gets as far as the device.
"""
import ctypes as C
import math

import pytest

from mimikit_amd import native


class _At:
    """an address inside the test's buffer, as an offset in bytes until the row runs"""

    def __init__(self, off=0):
        self.off = off

    def __add__(self, k):
        return _At(self.off + k)

    def __repr__(self):
        return f"P + {self.off}" if self.off else "P"


P = _At()                 # the buffer: 64 doubles, 64-byte aligned (so P + 2 misses 4 bytes, P + 4 misses 8, P + 8 misses 16)
COEFS = P + 256           # six pointers to P: the per-level spline tables of samplify_cuts, which the entry point reads on the host
SKEWED = P + 320          # six pointers to P + 4: the same with every table off its 8-byte boundary
KNOTS = P + 384           # six int64 knot counts of 8
BIG = 1 << 30             # a workspace size that is never too small
INF = math.inf
NAN = math.nan

_buffer = None


def _base() -> int:
    global _buffer
    if _buffer is None:
        raw = (C.c_double * (64 + 8))()
        base = (C.addressof(raw) + 63) // 64 * 64
        words = (C.c_uint64 * 64).from_address(base)
        for i in range(6):
            words[(COEFS.off >> 3) + i] = base
            words[(SKEWED.off >> 3) + i] = base + 4
            words[(KNOTS.off >> 3) + i] = 8
        _buffer = (raw, base)
    return _buffer[1]


def call(name: str, args):
    lib = native.load_library()
    base = _base()
    rc = getattr(lib, name)(*[base + a.off if isinstance(a, _At) else a for a in args])
    return rc, lib.mmk_last_error().decode()


# (entry point, arguments, return code, mmk_last_error()); sizes are tiny (n = 8, d = 8, k = 2, t = 2), the stream is None
ROWS = [
    # ---- filters.hip
    ("mmk_lfilter1_f32", (None, 8, 1, 8, 1.0, 0.0, 0.0, P, 8, None, None), -1, 'lfilter1: bad arguments (batch=1, n=8, row strides 8 / 8)'),
    ("mmk_lfilter1_f32", (P, 8, 1, 8, 1.0, 0.0, 0.0, None, 8, None, None), -1, 'lfilter1: bad arguments (batch=1, n=8, row strides 8 / 8)'),
    ("mmk_lfilter1_f32", (P, 8, 0, 8, 1.0, 0.0, 0.0, P, 8, None, None), -1, 'lfilter1: bad arguments (batch=0, n=8, row strides 8 / 8)'),
    ("mmk_lfilter1_f32", (P, 8, 1, 0, 1.0, 0.0, 0.0, P, 8, None, None), -1, 'lfilter1: bad arguments (batch=1, n=0, row strides 8 / 8)'),
    ("mmk_lfilter1_f32", (P, -1, 2, 8, 1.0, 0.0, 0.0, P, 8, None, None), -1, 'lfilter1: bad arguments (batch=2, n=8, row strides -1 / 8)'),
    ("mmk_lfilter1_f32", (P, 8, 2, 8, 1.0, 0.0, 0.0, P, 7, None, None), -1, 'lfilter1: bad arguments (batch=2, n=8, row strides 8 / 7)'),
    ("mmk_lfilter1_f32", (P + 2, 8, 1, 8, 1.0, 0.0, 0.0, P, 8, None, None), -1, 'lfilter1: x and y must be 4-byte aligned'),
    ("mmk_lfilter1_f32", (P, 8, 1, 8, 1.0, 0.0, 0.0, P + 2, 8, None, None), -1, 'lfilter1: x and y must be 4-byte aligned'),
    ("mmk_lfilter1_f32", (P, 8, 1, 8, 1.0, 0.0, 2.0, P, 8, None, None), -3, 'lfilter1: |a1| = 2 > 1 (the chunk powers a1^4096 .. of an unstable section overflow)'),
    ("mmk_row_normalize_f32", (None, 8, 1, 8, 2, 1e-12, P, 8, P, None), -1, 'row_normalize: bad arguments (batch=1, n=8, row strides 8 / 8)'),
    ("mmk_row_normalize_f32", (P, 8, 1, 8, 2, 1e-12, None, 8, P, None), -1, 'row_normalize: bad arguments (batch=1, n=8, row strides 8 / 8)'),
    ("mmk_row_normalize_f32", (P, 8, 0, 8, 2, 1e-12, P, 8, P, None), -1, 'row_normalize: bad arguments (batch=0, n=8, row strides 8 / 8)'),
    ("mmk_row_normalize_f32", (P, 8, 1, 0, 2, 1e-12, P, 8, P, None), -1, 'row_normalize: bad arguments (batch=1, n=0, row strides 8 / 8)'),
    ("mmk_row_normalize_f32", (P, 8, 2, 8, 2, 1e-12, P, 7, P, None), -1, 'row_normalize: bad arguments (batch=2, n=8, row strides 8 / 7)'),
    ("mmk_row_normalize_f32", (P + 2, 8, 1, 8, 2, 1e-12, P, 8, P, None), -1, 'row_normalize: x and y must be 4-byte aligned'),
    ("mmk_row_normalize_f32", (P, 8, 1, 8, 2, 1e-12, P + 1, 8, P, None), -1, 'row_normalize: x and y must be 4-byte aligned'),
    ("mmk_row_normalize_f32", (P, 8, 1, 8, 3, 1e-12, P, 8, P, None), -3, 'row_normalize: p must be 0 (inf), 1 or 2, got 3'),
    ("mmk_row_normalize_f32", (P, 8, 1, 8, 2, 1e-12, P, 8, None, None), -4, 'row_normalize: needs mmk_row_normalize_workspace_floats() floats'),
    # ---- envelope.hip
    ("mmk_interp1d_f32", (None, 8, 1, 8, P, 8, 8, 0, 1, None), -1, 'interp1d: bad arguments (batch=1, n=8, row strides 8 / 8)'),
    ("mmk_interp1d_f32", (P, 8, 1, 8, None, 8, 8, 0, 1, None), -1, 'interp1d: bad arguments (batch=1, n=8, row strides 8 / 8)'),
    ("mmk_interp1d_f32", (P, 8, 0, 8, P, 8, 8, 0, 1, None), -1, 'interp1d: bad arguments (batch=0, n=8, row strides 8 / 8)'),
    ("mmk_interp1d_f32", (P, -1, 2, 8, P, 8, 8, 0, 1, None), -1, 'interp1d: bad arguments (batch=2, n=8, row strides -1 / 8)'),
    ("mmk_interp1d_f32", (P, 8, 2, 8, P, 7, 8, 0, 1, None), -1, 'interp1d: bad arguments (batch=2, n=8, row strides 8 / 7)'),
    ("mmk_interp1d_f32", (P + 2, 8, 1, 8, P, 8, 8, 0, 1, None), -1, 'interp1d: x and y must be 4-byte aligned'),
    ("mmk_interp1d_f32", (P, 8, 1, 8, P + 3, 8, 8, 0, 1, None), -1, 'interp1d: x and y must be 4-byte aligned'),
    ("mmk_interp1d_f32", (P, 8, 65536, 8, P, 8, 8, 0, 1, None), -3, 'interp1d: 65536 rows are more than one launch takes (65535)'),
    ("mmk_interp1d_f32", (P, 8, 1, 0, P, 8, 8, 0, 1, None), -1, 'interp1d: needs n >= 2 knots and n_out >= 1 points, got 0 and 8'),
    ("mmk_derivative_f32", (None, 8, 1, 8, 2, P, 8, None), -1, 'derivative: bad arguments (batch=1, n=8, row strides 8 / 8)'),
    ("mmk_derivative_f32", (P, 8, 0, 8, 2, P, 8, None), -1, 'derivative: bad arguments (batch=0, n=8, row strides 8 / 8)'),
    ("mmk_derivative_f32", (P, 8, 2, 8, 2, P, 7, None), -1, 'derivative: bad arguments (batch=2, n=8, row strides 8 / 7)'),
    ("mmk_derivative_f32", (P + 2, 8, 1, 8, 2, P, 8, None), -1, 'derivative: x and y must be 4-byte aligned'),
    ("mmk_derivative_f32", (P, 8, 1, 8, 2, P + 2, 8, None), -1, 'derivative: x and y must be 4-byte aligned'),
    ("mmk_derivative_f32", (P, 8, 65536, 8, 2, P, 8, None), -3, 'derivative: 65536 rows are more than one launch takes (65535)'),
    ("mmk_derivative_f32", (P, 8, 1, 0, 2, P, 8, None), -1, 'derivative: the odd reflection of max_lag = 2 needs more than 2 samples, got 0'),
    # ---- nnn.hip
    ("mmk_inv_row_norm_f32", (P, 64, 8, 0, 8, 8, P, None), -1, 'inv_row_norm: batch = 0 < 1'),
    ("mmk_inv_row_norm_f32", (P, 64, 8, 1, 0, 8, P, None), -1, 'inv_row_norm: rows = 0 < 1'),
    ("mmk_inv_row_norm_f32", (P, 64, 8, 1, 8, 0, P, None), -1, 'inv_row_norm: k = 0 < 1 (bins)'),
    ("mmk_inv_row_norm_f32", (None, 64, 8, 1, 8, 8, P, None), -1, 'inv_row_norm: bad arguments (null or misaligned pointer, negative stride 64 / 8)'),
    ("mmk_inv_row_norm_f32", (P, 64, -8, 1, 8, 8, P, None), -1, 'inv_row_norm: bad arguments (null or misaligned pointer, negative stride 64 / -8)'),
    ("mmk_inv_row_norm_f32", (P + 2, 64, 8, 1, 8, 8, P, None), -1, 'inv_row_norm: bad arguments (null or misaligned pointer, negative stride 64 / 8)'),
    ("mmk_inv_row_norm_f32", (P, 64, 8, 1, 8, 8, P + 2, None), -1, 'inv_row_norm: bad arguments (null or misaligned pointer, negative stride 64 / 8)'),
    ("mmk_cosine_cost_f32", (P, 64, 8, P, 0, 8, P, 8, P, 8, 8, P, None), -1, 'cosine_cost: batch = 0 < 1'),
    ("mmk_cosine_cost_f32", (P, 64, 8, P, (1 << 24) + 1, 8, P, 8, P, 8, 8, P, None), -3, 'cosine_cost: batch = 16777217 clips are more than one launch takes'),
    ("mmk_cosine_cost_f32", (P, 64, 8, P, 1, 0, P, 8, P, 8, 8, P, None), -1, 'cosine_cost: n = 0 < 1 (prompt frames)'),
    ("mmk_cosine_cost_f32", (P, 64, 8, P, 1, 65, P, 8, P, 8, 8, P, None), -3, 'cosine_cost: n = 65 prompt frames, more than the 64 (MMK_NNN_MAX_ROWS) one wave aligns'),
    ("mmk_cosine_cost_f32", (P, 64, 8, P, 1, 8, P, 8, P, 0, 8, P, None), -1, 'cosine_cost: m = 0 < 1 (corpus frames)'),
    ("mmk_cosine_cost_f32", (P, 64, 8, P, 1, 8, P, 8, P, 1 << 31, 8, P, None), -3, 'cosine_cost: m = 2147483648 corpus frames: columns are counted in 32 bits'),
    ("mmk_cosine_cost_f32", (P, 64, 8, P, 1, 8, P, 8, P, 8, 0, P, None), -1, 'cosine_cost: k = 0 < 1 (bins)'),
    ("mmk_cosine_cost_f32", (P, 64, 8, P, 1, 8, P, 8, P, 8, 8, None, None), -1, 'cosine_cost: bad arguments (null pointer or negative stride 64 / 8 / 8)'),
    ("mmk_cosine_cost_f32", (P, 64, 8, P, 1, 8, P, -8, P, 8, 8, P, None), -1, 'cosine_cost: bad arguments (null pointer or negative stride 64 / 8 / -8)'),
    ("mmk_cosine_cost_f32", (P + 2, 64, 8, P, 1, 8, P, 8, P, 8, 8, P, None), -1, 'cosine_cost: x, y, rx and ry must be 4-byte aligned'),
    ("mmk_cosine_cost_f32", (P, 64, 8, P, 1, 8, P, 8, P + 2, 8, 8, P, None), -1, 'cosine_cost: x, y, rx and ry must be 4-byte aligned'),
    ("mmk_cosine_cost_f32", (P, 64, 8, P, 1, 8, P, 8, P, 8, 8, P + 8, None), -1, 'cosine_cost: cost must be 16-byte aligned'),
    ("mmk_cosine_cost_f32", (P, 64, 8, P, 1, 8, P, 8, P, 8, 8, P + 4, None), -1, 'cosine_cost: cost must be 16-byte aligned'),
    ("mmk_dtw_subseq_f32", (P, 0, 8, 8, P, P, None, None), -1, 'dtw_subseq: batch = 0 < 1'),
    ("mmk_dtw_subseq_f32", (P, 1, 0, 8, P, P, None, None), -1, 'dtw_subseq: n = 0 < 1 (prompt frames)'),
    ("mmk_dtw_subseq_f32", (P, 1, 65, 8, P, P, None, None), -3, 'dtw_subseq: n = 65 prompt frames, more than the 64 (MMK_NNN_MAX_ROWS) one wave aligns'),
    ("mmk_dtw_subseq_f32", (P, 1, 8, 0, P, P, None, None), -1, 'dtw_subseq: m = 0 < 1 (corpus frames)'),
    ("mmk_dtw_subseq_f32", (P, 1, 8, 1 << 31, P, P, None, None), -3, 'dtw_subseq: m = 2147483648 corpus frames: columns are counted in 32 bits'),
    ("mmk_dtw_subseq_f32", (None, 1, 8, 8, P, P, None, None), -1, 'dtw_subseq: cost, end_col and end_val must not be null'),
    ("mmk_dtw_subseq_f32", (P, 1, 8, 8, None, P, None, None), -1, 'dtw_subseq: cost, end_col and end_val must not be null'),
    ("mmk_dtw_subseq_f32", (P + 2, 1, 8, 8, P, P, None, None), -1, 'dtw_subseq: cost, end_val and last_row must be 4-byte aligned'),
    ("mmk_dtw_subseq_f32", (P, 1, 8, 8, P, P + 2, None, None), -1, 'dtw_subseq: cost, end_val and last_row must be 4-byte aligned'),
    ("mmk_dtw_subseq_f32", (P, 1, 8, 8, P, P, P + 2, None), -1, 'dtw_subseq: cost, end_val and last_row must be 4-byte aligned'),
    ("mmk_dtw_subseq_f32", (P, 1, 8, 8, P + 4, P, None, None), -1, 'dtw_subseq: end_col must be 8-byte aligned'),
    # ---- neighbors.hip
    ("mmk_nn_cosine_f32", (P, 8, P, 0, P, 8, P, 8, 8, P, P, P, BIG, None), -1, 'nn_cosine: rows = 0 < 1 (query frames)'),
    ("mmk_nn_cosine_f32", (P, 8, P, 8, P, 8, P, 0, 8, P, P, P, BIG, None), -1, 'nn_cosine: m = 0 < 1 (corpus frames)'),
    ("mmk_nn_cosine_f32", (P, 8, P, 8, P, 8, P, 8, 0, P, P, P, BIG, None), -1, 'nn_cosine: k = 0 < 1 (bins)'),
    ("mmk_nn_cosine_f32", (P, 8, P, 8, P, 8, P, 1 << 31, 8, P, P, P, BIG, None), -3, 'nn_cosine: m = 2147483648 corpus frames: indices are kept in 32 bits across the spans'),
    ("mmk_nn_cosine_f32", (P, 8, P, 8, P, 8, P, 8, 8, P, P, None, BIG, None), -1, 'nn_cosine: bad arguments (null pointer or negative stride 8 / 8)'),
    ("mmk_nn_cosine_f32", (P, 8, P, 8, P, -1, P, 8, 8, P, P, P, BIG, None), -1, 'nn_cosine: bad arguments (null pointer or negative stride 8 / -1)'),
    ("mmk_nn_cosine_f32", (P + 2, 8, P, 8, P, 8, P, 8, 8, P, P, P, BIG, None), -1, 'nn_cosine: x, y, rx, ry, cos_best and the workspace must be 4-byte aligned'),
    ("mmk_nn_cosine_f32", (P, 8, P, 8, P, 8, P, 8, 8, P, P, P + 2, BIG, None), -1, 'nn_cosine: x, y, rx, ry, cos_best and the workspace must be 4-byte aligned'),
    ("mmk_nn_cosine_f32", (P, 8, P, 8, P, 8, P, 8, 8, P + 4, P, P, BIG, None), -1, 'nn_cosine: index must be 8-byte aligned'),
    ("mmk_nn_cosine_f32", (P, 8, P, 8, P, 8, P, 8, 8, P, P, P, 8, None), -4, 'nn_cosine: the workspace has 8 bytes, 64 are needed'),
    ("mmk_nn_cosine_f32", (P, 8, P, 8, P, 8, P, 8, 8, P, P, P, 0, None), -4, 'nn_cosine: the workspace has 0 bytes, 64 are needed'),
    ("mmk_nn_cosine_self_f32", (P, 8, P, 1, 8, P, P, P, BIG, None), -1, 'nn_cosine_self: rows = 1 < 2 (a frame needs another one)'),
    ("mmk_nn_cosine_self_f32", (P, 8, P, 8, 0, P, P, P, BIG, None), -1, 'nn_cosine_self: k = 0 < 1 (bins)'),
    ("mmk_nn_cosine_self_f32", (P, 8, P, 1 << 31, 8, P, P, P, BIG, None), -3, 'nn_cosine_self: 2147483648 frames: indices are kept in 32 bits across the spans'),
    ("mmk_nn_cosine_self_f32", (P, 8, P, 8, 8, P, P, None, BIG, None), -1, 'nn_cosine_self: bad arguments (null pointer or negative stride 8)'),
    ("mmk_nn_cosine_self_f32", (P, -8, P, 8, 8, P, P, P, BIG, None), -1, 'nn_cosine_self: bad arguments (null pointer or negative stride -8)'),
    ("mmk_nn_cosine_self_f32", (P, 8, P + 2, 8, 8, P, P, P, BIG, None), -1, 'nn_cosine_self: x, rx, cos_best and the workspace must be 4-byte aligned'),
    ("mmk_nn_cosine_self_f32", (P, 8, P, 8, 8, P, P, P + 2, BIG, None), -1, 'nn_cosine_self: x, rx, cos_best and the workspace must be 4-byte aligned'),
    ("mmk_nn_cosine_self_f32", (P, 8, P, 8, 8, P + 4, P, P, BIG, None), -1, 'nn_cosine_self: index must be 8-byte aligned'),
    ("mmk_nn_cosine_self_f32", (P, 8, P, 8, 8, P, P, P, 63, None), -4, 'nn_cosine_self: the workspace has 63 bytes, 64 are needed'),
    ("mmk_cum_entropy_i64", (P, 8, 0, 8, P, None, 0, None), -1, 'cum_entropy: batch = 0 < 1'),
    ("mmk_cum_entropy_i64", (P, 8, 1, 0, P, None, 0, None), -1, 'cum_entropy: t = 0 < 1 (items per row)'),
    ("mmk_cum_entropy_i64", (P, 8, 1, 32769, P, None, 0, None), -3, 'cum_entropy: t = 32769 items per row, more than the 32768 (MMK_CUM_ENTROPY_MAX_T) one workgroup ranks'),
    ("mmk_cum_entropy_i64", (None, 8, 1, 8, P, None, 0, None), -1, 'cum_entropy: bad arguments (null or misaligned pointer, negative stride 8 / 0)'),
    ("mmk_cum_entropy_i64", (P, -8, 1, 8, P, None, 0, None), -1, 'cum_entropy: bad arguments (null or misaligned pointer, negative stride -8 / 0)'),
    ("mmk_cum_entropy_i64", (P + 4, 8, 1, 8, P, None, 0, None), -1, 'cum_entropy: bad arguments (null or misaligned pointer, negative stride 8 / 0)'),
    ("mmk_cum_entropy_i64", (P, 8, 1, 8, P + 2, None, 0, None), -1, 'cum_entropy: bad arguments (null or misaligned pointer, negative stride 8 / 0)'),
    ("mmk_cum_entropy_i64", (P, 8, 1, 8, P, P + 2, 8, None), -1, 'cum_entropy: bad arguments (null or misaligned pointer, negative stride 8 / 8)'),
    # ---- hcluster.hip
    ("mmk_nn_components_i64", (P, 0, P, P, P, BIG, None), -1, 'nn_components: n = 0 < 1 (nodes)'),
    ("mmk_nn_components_i64", (P, 1 << 31, P, P, P, BIG, None), -3, 'nn_components: n = 2147483648 nodes: indices are kept in 32 bits'),
    ("mmk_nn_components_i64", (P, 8, P, P, None, BIG, None), -1, 'nn_components: bad arguments (null pointer)'),
    ("mmk_nn_components_i64", (P + 4, 8, P, P, P, BIG, None), -1, 'nn_components: nearest, labels and n_components must be 8-byte aligned'),
    ("mmk_nn_components_i64", (P, 8, P, P + 4, P, BIG, None), -1, 'nn_components: nearest, labels and n_components must be 8-byte aligned'),
    ("mmk_nn_components_i64", (P, 8, P, P, P + 2, BIG, None), -1, 'nn_components: the workspace must be 4-byte aligned'),
    ("mmk_nn_components_i64", (P, 8, P, P, P + 4, 8, None), -4, 'nn_components: the workspace has 8 bytes, 164 are needed'),
    ("mmk_nn_components_i64", (P, 8, P, P, P, 0, None), -4, 'nn_components: the workspace has 0 bytes, 164 are needed'),
    ("mmk_edge_components_i64", (P, P, 2, 0, P, P, P, BIG, None), -1, 'edge_components: n = 0 < 1 (nodes)'),
    ("mmk_edge_components_i64", (P, P, -1, 8, P, P, P, BIG, None), -1, 'edge_components: n_edges = -1 < 0'),
    ("mmk_edge_components_i64", (P, P, 2, 1 << 31, P, P, P, BIG, None), -3, 'edge_components: n = 2147483648 nodes: indices are kept in 32 bits'),
    ("mmk_edge_components_i64", (P, P, 1 << 40, 8, P, P, P, BIG, None), -3, 'edge_components: 1099511627776 edges are more than one launch takes'),
    ("mmk_edge_components_i64", (None, P, 2, 8, P, P, P, BIG, None), -1, 'edge_components: bad arguments (null pointer)'),
    ("mmk_edge_components_i64", (P, P, 2, 8, P, P, None, BIG, None), -1, 'edge_components: bad arguments (null pointer)'),
    ("mmk_edge_components_i64", (P, P + 4, 2, 8, P, P, P, BIG, None), -1, 'edge_components: src, dst, labels and n_components must be 8-byte aligned'),
    ("mmk_edge_components_i64", (P, P, 2, 8, P + 4, P, P, BIG, None), -1, 'edge_components: src, dst, labels and n_components must be 8-byte aligned'),
    ("mmk_edge_components_i64", (P, P, 2, 8, P, P, P + 2, BIG, None), -1, 'edge_components: the workspace must be 4-byte aligned'),
    ("mmk_edge_components_i64", (P, P, 2, 8, P, P, P + 4, 8, None), -4, 'edge_components: the workspace has 8 bytes, 104 are needed'),
    ("mmk_segment_mean_f32", (P, 8, 0, 8, P, P, 2, P, 8, None), -1, 'segment_mean: n = 0 < 1 (rows)'),
    ("mmk_segment_mean_f32", (P, 8, 8, 0, P, P, 2, P, 8, None), -1, 'segment_mean: k = 0 < 1 (bins)'),
    ("mmk_segment_mean_f32", (P, 8, 8, 8, P, P, 9, P, 8, None), -1, 'segment_mean: 9 segments of 8 rows (every segment has a member)'),
    ("mmk_segment_mean_f32", (P, 8, 1 << 32, 8, P, P, 1 << 32, P, 8, None), -3, 'segment_mean: 4294967296 segments are more than one launch takes'),
    ("mmk_segment_mean_f32", (P, 8, 8, 8, None, P, 2, P, 8, None), -1, 'segment_mean: bad arguments (null pointer or negative stride 8 / 8)'),
    ("mmk_segment_mean_f32", (P, 8, 8, 8, P, P, 2, P, -8, None), -1, 'segment_mean: bad arguments (null pointer or negative stride 8 / -8)'),
    ("mmk_segment_mean_f32", (P + 2, 8, 8, 8, P, P, 2, P, 8, None), -1, 'segment_mean: x and out must be 4-byte aligned'),
    ("mmk_segment_mean_f32", (P, 8, 8, 8, P, P, 2, P + 2, 8, None), -1, 'segment_mean: x and out must be 4-byte aligned'),
    ("mmk_segment_mean_f32", (P, 8, 8, 8, P + 4, P, 2, P, 8, None), -1, 'segment_mean: order and offsets must be 8-byte aligned'),
    ("mmk_segment_mean_f32", (P, 8, 8, 8, P, P + 4, 2, P, 8, None), -1, 'segment_mean: order and offsets must be 8-byte aligned'),
    # ---- qcluster.hip
    ("mmk_nn_topk_f32", (P, 8, P, 0, P, 8, P, P, -INF, INF, 8, 8, 2, 0, P, P, P, BIG, None), -1, 'nn_topk: rows = 0 < 1 (query frames)'),
    ("mmk_nn_topk_f32", (P, 8, P, 8, P, 8, P, P, -INF, INF, 0, 8, 2, 0, P, P, P, BIG, None), -1, 'nn_topk: m = 0 < 1 (corpus frames)'),
    ("mmk_nn_topk_f32", (P, 8, P, 8, P, 8, P, P, -INF, INF, 8, 0, 2, 0, P, P, P, BIG, None), -1, 'nn_topk: k = 0 < 1 (bins)'),
    ("mmk_nn_topk_f32", (P, 8, P, 8, P, 8, P, P, -INF, INF, 8, 8, 0, 0, P, P, P, BIG, None), -1, 'nn_topk: t = 0 < 1 (neighbours kept per row)'),
    ("mmk_nn_topk_f32", (P, 8, P, 8, P, 8, P, P, 1.0, 1.0, 8, 8, 2, 0, P, P, P, BIG, None), -1, 'nn_topk: key_min = 1 must lie below key_max = 1 (-inf and +inf: no clamp)'),
    ("mmk_nn_topk_f32", (P, 8, P, 8, P, 8, P, P, -INF, INF, 8, 8, 17, 0, P, P, P, BIG, None), -3, 'nn_topk: t = 17 neighbours per row, more than the 16 (MMK_NN_TOPK_MAX) a lane keeps in registers'),
    ("mmk_nn_topk_f32", (P, 8, P, 8, P, 8, P, P, -INF, INF, 1 << 31, 8, 2, 0, P, P, P, BIG, None), -3, 'nn_topk: m = 2147483648 corpus frames: indices are kept in 32 bits across the spans'),
    ("mmk_nn_topk_f32", (P, 8, P, 8, P, 8, P, P, -INF, INF, 9, 8, 2, 1, P, P, P, BIG, None), -1, 'nn_topk: self_exclude takes the corpus = the queries (y == x, the same stride, m == rows = 8, got m = 9)'),
    ("mmk_nn_topk_f32", (P, 8, P, 8, P, 8, P, P, -INF, INF, 8, 8, 2, 0, P, P, None, BIG, None), -1, 'nn_topk: bad arguments (null pointer or negative stride 8 / 8)'),
    ("mmk_nn_topk_f32", (P, 8, P, 8, P, -8, P, P, -INF, INF, 8, 8, 2, 0, P, P, P, BIG, None), -1, 'nn_topk: bad arguments (null pointer or negative stride 8 / -8)'),
    ("mmk_nn_topk_f32", (P + 2, 8, P, 8, P, 8, P, P, -INF, INF, 8, 8, 2, 0, P, P, P, BIG, None), -1, 'nn_topk: x, y, qscale, cscale, cshift, key and the workspace must be 4-byte aligned'),
    ("mmk_nn_topk_f32", (P, 8, P, 8, P, 8, P, P + 2, -INF, INF, 8, 8, 2, 0, P, P, P, BIG, None), -1, 'nn_topk: x, y, qscale, cscale, cshift, key and the workspace must be 4-byte aligned'),
    ("mmk_nn_topk_f32", (P, 8, P, 8, P, 8, P, P, -INF, INF, 8, 8, 2, 0, P, P, P + 2, BIG, None), -1, 'nn_topk: x, y, qscale, cscale, cshift, key and the workspace must be 4-byte aligned'),
    ("mmk_nn_topk_f32", (P, 8, P, 8, P, 8, P, P, -INF, INF, 8, 8, 2, 0, P + 4, P, P, BIG, None), -1, 'nn_topk: index must be 8-byte aligned'),
    ("mmk_nn_topk_f32", (P, 8, P, 8, P, 8, P, P, -INF, INF, 8, 8, 2, 0, P, P, P, 8, None), -4, 'nn_topk: the workspace has 8 bytes, 128 are needed'),
    ("mmk_nn_topk_f32", (P, 8, P, 8, P, 8, P, P, -INF, INF, 8, 8, 2, 0, P, P, P + 4, 0, None), -4, 'nn_topk: the workspace has 0 bytes, 128 are needed'),
    ("mmk_half_neg_sqnorm_f32", (P, 8, 0, 8, P, None), -1, 'half_neg_sqnorm: rows = 0, k = 8 (both at least 1)'),
    ("mmk_half_neg_sqnorm_f32", (P, 8, 8, 0, P, None), -1, 'half_neg_sqnorm: rows = 8, k = 0 (both at least 1)'),
    ("mmk_half_neg_sqnorm_f32", (P, 8, 1 << 34, 8, P, None), -3, 'half_neg_sqnorm: 17179869184 rows are more than one launch takes'),
    ("mmk_half_neg_sqnorm_f32", (None, 8, 8, 8, P, None), -1, 'half_neg_sqnorm: bad arguments (null or misaligned pointer, negative stride 8)'),
    ("mmk_half_neg_sqnorm_f32", (P, -8, 8, 8, P, None), -1, 'half_neg_sqnorm: bad arguments (null or misaligned pointer, negative stride -8)'),
    ("mmk_half_neg_sqnorm_f32", (P + 2, 8, 8, 8, P, None), -1, 'half_neg_sqnorm: bad arguments (null or misaligned pointer, negative stride 8)'),
    ("mmk_half_neg_sqnorm_f32", (P, 8, 8, 8, P + 2, None), -1, 'half_neg_sqnorm: bad arguments (null or misaligned pointer, negative stride 8)'),
    # ---- kmeans.hip
    ("mmk_kmeans_assign_f32", (P, 8, None, 0, 8, P, 8, P, 2, P, None, None, None), -1, 'kmeans_assign: n = 0, d = 8, k = 2 (all at least 1)'),
    ("mmk_kmeans_assign_f32", (P, 8, None, 8, 8, P, 8, P, 257, P, None, None, None), -3, 'kmeans_assign: k = 257 centres, more than the 256 (MMK_KMEANS_MAX_K) of the widest centre tile'),
    ("mmk_kmeans_assign_f32", (P, 8, None, 8, 8, None, 8, P, 2, P, None, None, None), -1, 'kmeans_assign: bad arguments (null pointer or negative stride 8 / 8)'),
    ("mmk_kmeans_assign_f32", (P, 8, None, 8, 8, P, -8, P, 2, P, None, None, None), -1, 'kmeans_assign: bad arguments (null pointer or negative stride 8 / -8)'),
    ("mmk_kmeans_assign_f32", (P + 2, 8, None, 8, 8, P, 8, P, 2, P, None, None, None), -1, 'kmeans_assign: x, offset, centres, shift, labels and key must be 4-byte aligned'),
    ("mmk_kmeans_assign_f32", (P, 8, P + 2, 8, 8, P, 8, P, 2, P, None, None, None), -1, 'kmeans_assign: x, offset, centres, shift, labels and key must be 4-byte aligned'),
    ("mmk_kmeans_assign_f32", (P, 8, None, 8, 8, P, 8, P, 2, P, P + 2, None, None), -1, 'kmeans_assign: x, offset, centres, shift, labels and key must be 4-byte aligned'),
    ("mmk_kmeans_assign_f32", (P, 8, None, 8, 8, P, 8, P, 2, P, None, P + 4, None), -1, 'kmeans_assign: changed must be 8-byte aligned'),
    ("mmk_kmeans_label_sums_f64", (P, 8, None, 0, 8, P, 2, P, P, None, 0, None, None, P, BIG, None), -1, 'kmeans_label_sums: n = 0, d = 8, k = 2 (all at least 1)'),
    ("mmk_kmeans_label_sums_f64", (P, 8, None, 8, 8, None, 2, P, P, None, 0, None, None, P, BIG, None), -1, 'kmeans_label_sums: bad arguments (null pointer or negative stride 8 / 0)'),
    ("mmk_kmeans_label_sums_f64", (P, -8, None, 8, 8, P, 2, P, P, None, 0, None, None, P, BIG, None), -1, 'kmeans_label_sums: bad arguments (null pointer or negative stride -8 / 0)'),
    ("mmk_kmeans_label_sums_f64", (P, 8, None, 8, 8, P, 2, P, P, None, 0, P, None, P, BIG, None), -1, 'kmeans_label_sums: row_d2 and inertia need the centres'),
    ("mmk_kmeans_label_sums_f64", (P + 2, 8, None, 8, 8, P, 2, P, P, None, 0, None, None, P, BIG, None), -1, 'kmeans_label_sums: x, offset, labels and centres must be 4-byte aligned'),
    ("mmk_kmeans_label_sums_f64", (P, 8, None, 8, 8, P, 2, P, P, P + 2, 8, None, None, P, BIG, None), -1, 'kmeans_label_sums: x, offset, labels and centres must be 4-byte aligned'),
    ("mmk_kmeans_label_sums_f64", (P, 8, None, 8, 8, P, 2, P + 4, P, None, 0, None, None, P, BIG, None), -1, 'kmeans_label_sums: sums, counts, row_d2 and inertia must be 8-byte aligned'),
    ("mmk_kmeans_label_sums_f64", (P, 8, None, 8, 8, P, 2, P, P, P, 8, None, P + 4, P, BIG, None), -1, 'kmeans_label_sums: sums, counts, row_d2 and inertia must be 8-byte aligned'),
    ("mmk_kmeans_label_sums_f64", (P, 8, None, 8, 8, P, 1 << 20, P, P, None, 0, None, None, P, 1 << 40, None), -3, "kmeans_label_sums: k = 1048576 labels: their counts alone do not fit a wave's 60000 bytes of LDS"),
    ("mmk_kmeans_label_sums_f64", (P, 8, None, 8, 8, P, 2, P, P, None, 0, None, None, None, BIG, None), -4, 'kmeans_label_sums: the workspace has 1073741824 bytes, 8336 are needed, 8-byte aligned'),
    ("mmk_kmeans_label_sums_f64", (P, 8, None, 8, 8, P, 2, P, P, None, 0, None, None, P + 4, BIG, None), -4, 'kmeans_label_sums: the workspace has 1073741824 bytes, 8336 are needed, 8-byte aligned'),
    ("mmk_kmeans_label_sums_f64", (P, 8, None, 8, 8, P, 2, P, P, None, 0, None, None, P, 8, None), -4, 'kmeans_label_sums: the workspace has 8 bytes, 8336 are needed, 8-byte aligned'),
    ("mmk_kmeans_pp_step_f64", (P, 8, None, 0, 8, P, 2, P, P, P, P, BIG, None), -1, 'kmeans_pp_step: n = 0, d = 8, t = 2 (all at least 1)'),
    ("mmk_kmeans_pp_step_f64", (P, 8, None, 8, 8, P, 9, P, P, P, P, BIG, None), -3, 'kmeans_pp_step: t = 9 candidates, more than 8 (MMK_KMEANS_PP_MAX_TRIALS)'),
    ("mmk_kmeans_pp_step_f64", (P, 8, None, 8, 8, None, 2, P, P, P, P, BIG, None), -1, 'kmeans_pp_step: bad arguments (null pointer or negative stride 8)'),
    ("mmk_kmeans_pp_step_f64", (P, -8, None, 8, 8, P, 2, P, P, P, P, BIG, None), -1, 'kmeans_pp_step: bad arguments (null pointer or negative stride -8)'),
    ("mmk_kmeans_pp_step_f64", (P + 2, 8, None, 8, 8, P, 2, P, P, P, P, BIG, None), -1, 'kmeans_pp_step: x and offset must be 4-byte aligned'),
    ("mmk_kmeans_pp_step_f64", (P, 8, P + 2, 8, 8, P, 2, P, P, P, P, BIG, None), -1, 'kmeans_pp_step: x and offset must be 4-byte aligned'),
    ("mmk_kmeans_pp_step_f64", (P, 8, None, 8, 8, P + 4, 2, P, P, P, P, BIG, None), -1, 'kmeans_pp_step: cand, closest, pot and chosen must be 8-byte aligned'),
    ("mmk_kmeans_pp_step_f64", (P, 8, None, 8, 8, P, 2, P, P, P + 4, P, BIG, None), -1, 'kmeans_pp_step: cand, closest, pot and chosen must be 8-byte aligned'),
    ("mmk_kmeans_pp_step_f64", (P, 8, None, 8, 8, P, 2, P, P, P, None, BIG, None), -4, 'kmeans_pp_step: the workspace has 1073741824 bytes, 65544 are needed, 8-byte aligned'),
    ("mmk_kmeans_pp_step_f64", (P, 8, None, 8, 8, P, 2, P, P, P, P + 4, BIG, None), -4, 'kmeans_pp_step: the workspace has 1073741824 bytes, 65544 are needed, 8-byte aligned'),
    ("mmk_kmeans_pp_step_f64", (P, 8, None, 8, 8, P, 2, P, P, P, P, 64, None), -4, 'kmeans_pp_step: the workspace has 64 bytes, 65544 are needed, 8-byte aligned'),
    # ---- nn_filter.hip
    ("mmk_nn_aggregate_f32", (P, 8, 0, 8, P, 2, 1, 0, P + 256, 8, None, None), -1, 'nn_aggregate: n = 0, d = 8, t = 2 (all at least 1)'),
    ("mmk_nn_aggregate_f32", (P, 8, 8, 8, P, 17, 1, 0, P + 256, 8, None, None), -3, 'nn_aggregate: t = 17 slots per row, more than the 16 (MMK_NN_TOPK_MAX) a wave keeps in registers'),
    ("mmk_nn_aggregate_f32", (P, 8, 8, 8, P, 2, 1, 99, P + 256, 8, None, None), -3, 'nn_aggregate: op = 99 is none of MMK_NN_AGG_MEDIAN, _MEAN, _MAX, _MIN'),
    ("mmk_nn_aggregate_f32", (P, 8, 8, 8, None, 2, 1, 0, P + 256, 8, None, None), -1, 'nn_aggregate: bad arguments (null pointer, x_row_stride 8 < 0 or out_row_stride 8 < d = 8)'),
    ("mmk_nn_aggregate_f32", (P, 8, 8, 8, P, 2, 1, 0, P + 256, 7, None, None), -1, 'nn_aggregate: bad arguments (null pointer, x_row_stride 8 < 0 or out_row_stride 7 < d = 8)'),
    ("mmk_nn_aggregate_f32", (P + 2, 8, 8, 8, P, 2, 1, 0, P + 256, 8, None, None), -1, 'nn_aggregate: x, out and count must be 4-byte aligned'),
    ("mmk_nn_aggregate_f32", (P, 8, 8, 8, P, 2, 1, 0, P + 258, 8, None, None), -1, 'nn_aggregate: x, out and count must be 4-byte aligned'),
    ("mmk_nn_aggregate_f32", (P, 8, 8, 8, P, 2, 1, 0, P + 256, 8, P + 2, None), -1, 'nn_aggregate: x, out and count must be 4-byte aligned'),
    ("mmk_nn_aggregate_f32", (P, 8, 8, 8, P + 4, 2, 1, 0, P + 256, 8, None, None), -1, 'nn_aggregate: index must be 8-byte aligned'),
    ("mmk_nn_aggregate_f32", (P, 8, 8, 8, P, 2, 1, 0, P, 8, None, None), -1, 'nn_aggregate: out must not alias x'),
    # ---- pca.hip
    ("mmk_pca_colstats_f64", (P, 8, 0, 8, P, P, P, BIG, None), -1, 'pca_colstats: n = 0 rows, d = 8 columns (both at least 1)'),
    ("mmk_pca_colstats_f64", (P, 8, 8, 4097, P, P, P, BIG, None), -3, 'pca_colstats: d = 4097 columns, the limit is 4096 (MMK_PCA_MAX_D)'),
    ("mmk_pca_colstats_f64", (P, 8, 8, 8, P, P, None, BIG, None), -1, 'pca_colstats: bad arguments (null pointer or negative stride 8)'),
    ("mmk_pca_colstats_f64", (P, -8, 8, 8, P, P, P, BIG, None), -1, 'pca_colstats: bad arguments (null pointer or negative stride -8)'),
    ("mmk_pca_colstats_f64", (P + 2, 8, 8, 8, P, P, P, BIG, None), -1, 'pca_colstats: x must be 4-byte aligned, mean, scale and the workspace 8-byte aligned'),
    ("mmk_pca_colstats_f64", (P + 4, 8, 8, 8, P, P + 4, P, BIG, None), -1, 'pca_colstats: x must be 4-byte aligned, mean, scale and the workspace 8-byte aligned'),
    ("mmk_pca_colstats_f64", (P, 8, 8, 8, P, P, P + 4, BIG, None), -1, 'pca_colstats: x must be 4-byte aligned, mean, scale and the workspace 8-byte aligned'),
    ("mmk_pca_colstats_f64", (P + 4, 8, 8, 8, P, P, P, 8, None), -4, 'pca_colstats: the workspace has 8 bytes, 128 are needed'),
    ("mmk_pca_colstats_f64", (P, 8, 8, 8, P, P, P, 0, None), -4, 'pca_colstats: the workspace has 0 bytes, 128 are needed'),
    ("mmk_pca_cov_f64", (P, 8, 1, 8, P, P, P, P, BIG, None), -1, 'pca_cov: n = 1 rows (at least 2), d = 8 columns (at least 1)'),
    ("mmk_pca_cov_f64", (P, 8, 8, 4097, P, P, P, P, BIG, None), -3, 'pca_cov: d = 4097 columns, the limit is 4096 (MMK_PCA_MAX_D)'),
    ("mmk_pca_cov_f64", (P, 8, 8, 8, P, P, P, None, BIG, None), -1, 'pca_cov: bad arguments (null pointer or negative stride 8)'),
    ("mmk_pca_cov_f64", (P, -8, 8, 8, P, P, P, P, BIG, None), -1, 'pca_cov: bad arguments (null pointer or negative stride -8)'),
    ("mmk_pca_cov_f64", (P + 2, 8, 8, 8, P, P, P, P, BIG, None), -1, 'pca_cov: x must be 4-byte aligned, mean, scale, c and the workspace 8-byte aligned'),
    ("mmk_pca_cov_f64", (P, 8, 8, 8, P, P, P + 4, P, BIG, None), -1, 'pca_cov: x must be 4-byte aligned, mean, scale, c and the workspace 8-byte aligned'),
    ("mmk_pca_cov_f64", (P, 8, 8, 8, P, P, P, P + 4, BIG, None), -1, 'pca_cov: x must be 4-byte aligned, mean, scale, c and the workspace 8-byte aligned'),
    ("mmk_pca_cov_f64", (P + 4, 8, 8, 8, P, P, P, P, 8, None), -4, 'pca_cov: the workspace has 8 bytes, 32768 are needed'),
    ("mmk_pca_eig_f64", (P, 8, 9, 0, P, P, P, P, BIG, None), -1, 'pca_eig: n_components = 9 must lie in [1, d = 8]'),
    ("mmk_pca_eig_f64", (P, 4097, 2, 0, P, P, P, P, BIG, None), -3, 'pca_eig: d = 4097 columns, the limit is 4096 (MMK_PCA_MAX_D)'),
    ("mmk_pca_eig_f64", (P, 128, 65, 0, P, P, P, P, BIG, None), -3, "pca_eig: n_components = 65, the limit is 64 (MMK_PCA_MAX_COMPONENTS: the Jacobi step's block fits LDS)"),
    ("mmk_pca_eig_f64", (P, 8, 2, -1, P, P, P, P, BIG, None), -1, 'pca_eig: max_iter = -1 < 0 (0: MMK_PCA_MAX_ITER)'),
    ("mmk_pca_eig_f64", (P, 8, 2, 0, P, P, None, P, BIG, None), -1, 'pca_eig: bad arguments (null pointer)'),
    ("mmk_pca_eig_f64", (P + 4, 8, 2, 0, P, P, P, P, BIG, None), -1, 'pca_eig: c, components, variance and the workspace must be 8-byte aligned'),
    ("mmk_pca_eig_f64", (P, 8, 2, 0, P, P, P, P + 4, BIG, None), -1, 'pca_eig: c, components, variance and the workspace must be 8-byte aligned'),
    ("mmk_pca_eig_f64", (P, 8, 2, 0, P, P, P + 4, P, 8, None), -4, 'pca_eig: the workspace has 8 bytes, 3760 are needed'),
    ("mmk_pca_project_f32", (P, 8, 0, 8, P, P, P, 2, P, 2, None), -1, 'pca_project: m = 0 rows, d = 8 columns, n_components = 2 (all at least 1)'),
    ("mmk_pca_project_f32", (P, 8, 8, 4097, P, P, P, 2, P, 2, None), -3, 'pca_project: d = 4097 columns, the limit is 4096 (MMK_PCA_MAX_D)'),
    ("mmk_pca_project_f32", (P, 8, 8, 8, P, P, P, 65, P, 65, None), -3, 'pca_project: n_components = 65, the limit is 64 (MMK_PCA_MAX_COMPONENTS)'),
    ("mmk_pca_project_f32", (P, 8, 1 << 40, 8, P, P, P, 2, P, 2, None), -3, 'pca_project: 1099511627776 rows are more than one launch takes'),
    ("mmk_pca_project_f32", (P, 8, 8, 8, None, P, P, 2, P, 2, None), -1, 'pca_project: bad arguments (null pointer, negative stride 8 or an output stride 2 below n_components)'),
    ("mmk_pca_project_f32", (P, 8, 8, 8, P, P, P, 2, P, 1, None), -1, 'pca_project: bad arguments (null pointer, negative stride 8 or an output stride 1 below n_components)'),
    ("mmk_pca_project_f32", (P + 2, 8, 8, 8, P, P, P, 2, P, 2, None), -1, 'pca_project: y and out must be 4-byte aligned, mean, scale and components 8-byte aligned'),
    ("mmk_pca_project_f32", (P + 4, 8, 8, 8, P, P, P, 2, P + 2, 2, None), -1, 'pca_project: y and out must be 4-byte aligned, mean, scale and components 8-byte aligned'),
    ("mmk_pca_project_f32", (P, 8, 8, 8, P + 4, P, P, 2, P, 2, None), -1, 'pca_project: y and out must be 4-byte aligned, mean, scale and components 8-byte aligned'),
    ("mmk_pca_project_f32", (P, 8, 8, 8, P, P, P + 4, 2, P + 4, 2, None), -1, 'pca_project: y and out must be 4-byte aligned, mean, scale and components 8-byte aligned'),
    # ---- nmf.hip
    ("mmk_nmf_start_f64", (P, 8, 0, 8, 2, P, P, P, P, P, P, BIG, None), -1, 'nmf_start: n = 0 rows, d = 8 columns (both at least 1)'),
    ("mmk_nmf_start_f64", (P, 8, 8, 4097, 2, P, P, P, P, P, P, BIG, None), -3, 'nmf_start: d = 4097 columns, the limit is 4096 (MMK_NMF_MAX_D)'),
    ("mmk_nmf_start_f64", (P, 8, 128, 128, 65, P, P, P, P, P, P, BIG, None), -3, "nmf_start: n_components = 65, the limit is 64 (MMK_NMF_MAX_COMPONENTS: a row of W lives in one lane's registers)"),
    ("mmk_nmf_start_f64", (P, 8, 8, 8, 0, P, P, P, P, P, P, BIG, None), -1, 'nmf_start: n_components = 0 must be at least 1'),
    ("mmk_nmf_start_f64", (P, 8, 8, 8, 9, P, P, P, P, P, P, BIG, None), -1, 'nmf_start: n_components = 9 must lie in [1, min(n, d) = 8]'),
    ("mmk_nmf_start_f64", (P, 8, 1 << 40, 8, 2, P, P, P, P, P, P, BIG, None), -3, 'nmf_start: 1099511627776 rows are more than one launch takes'),
    ("mmk_nmf_start_f64", (P, 8, 1, 1, 1, P, P, P, P, P, P, BIG, None), -1, 'nmf_start: n = 1 rows, at least 2 are needed (the Gram matrix comes from the covariance kernel)'),
    ("mmk_nmf_start_f64", (P, 8, 8, 8, 2, P, P, P, P, None, P, BIG, None), -1, 'nmf_start: bad arguments (null pointer or negative stride 8)'),
    ("mmk_nmf_start_f64", (P, -8, 8, 8, 2, P, P, P, P, P, P, BIG, None), -1, 'nmf_start: bad arguments (null pointer or negative stride -8)'),
    ("mmk_nmf_start_f64", (P + 2, 8, 8, 8, 2, P, P, P, P, P, P, BIG, None), -1, 'nmf_start: x and part must be 4-byte aligned, w, ht, s, v and the workspace 8-byte aligned'),
    ("mmk_nmf_start_f64", (P + 4, 8, 8, 8, 2, P, P, P, P, P + 2, P, BIG, None), -1, 'nmf_start: x and part must be 4-byte aligned, w, ht, s, v and the workspace 8-byte aligned'),
    ("mmk_nmf_start_f64", (P, 8, 8, 8, 2, P + 4, P, P, P, P + 4, P, BIG, None), -1, 'nmf_start: x and part must be 4-byte aligned, w, ht, s, v and the workspace 8-byte aligned'),
    ("mmk_nmf_start_f64", (P, 8, 8, 8, 2, P, P, P, P, P, P + 4, BIG, None), -1, 'nmf_start: x and part must be 4-byte aligned, w, ht, s, v and the workspace 8-byte aligned'),
    ("mmk_nmf_start_f64", (P + 4, 8, 8, 8, 2, P, P, P, P, P + 4, P, 8, None), -4, 'nmf_start: the workspace has 8 bytes, 37328 are needed'),
    ("mmk_nmf_w_half_f64", (P, 8, 0, 8, 2, P, P, P, P, BIG, None), -1, 'nmf_w_half: n = 0 rows, d = 8 columns (both at least 1)'),
    ("mmk_nmf_w_half_f64", (P, 8, 8, 8, 65, P, P, P, P, BIG, None), -3, "nmf_w_half: n_components = 65, the limit is 64 (MMK_NMF_MAX_COMPONENTS: a row of W lives in one lane's registers)"),
    ("mmk_nmf_w_half_f64", (P, 8, 8, 8, 2, P, P, None, P, BIG, None), -1, 'nmf_w_half: bad arguments (null pointer or negative stride 8)'),
    ("mmk_nmf_w_half_f64", (P, -8, 8, 8, 2, P, P, P, P, BIG, None), -1, 'nmf_w_half: bad arguments (null pointer or negative stride -8)'),
    ("mmk_nmf_w_half_f64", (P + 2, 8, 8, 8, 2, P, P, P, P, BIG, None), -1, 'nmf_w_half: x must be 4-byte aligned, w, ht, violation and the workspace 8-byte aligned'),
    ("mmk_nmf_w_half_f64", (P, 8, 8, 8, 2, P, P, P + 4, P, BIG, None), -1, 'nmf_w_half: x must be 4-byte aligned, w, ht, violation and the workspace 8-byte aligned'),
    ("mmk_nmf_w_half_f64", (P, 8, 8, 8, 2, P, P, P, P + 4, BIG, None), -1, 'nmf_w_half: x must be 4-byte aligned, w, ht, violation and the workspace 8-byte aligned'),
    ("mmk_nmf_w_half_f64", (P + 4, 8, 8, 8, 2, P, P, P, P, 8, None), -4, 'nmf_w_half: the workspace has 8 bytes, 208 are needed'),
    ("mmk_nmf_h_half_f64", (P, 8, 8, 0, 2, P, P, P, P, BIG, None), -1, 'nmf_h_half: n = 8 rows, d = 0 columns (both at least 1)'),
    ("mmk_nmf_h_half_f64", (P, 8, 8, 8, 2, None, P, P, P, BIG, None), -1, 'nmf_h_half: bad arguments (null pointer or negative stride 8)'),
    ("mmk_nmf_h_half_f64", (P + 2, 8, 8, 8, 2, P, P, P, P, BIG, None), -1, 'nmf_h_half: x must be 4-byte aligned, w, ht, violation and the workspace 8-byte aligned'),
    ("mmk_nmf_h_half_f64", (P, 8, 8, 8, 2, P + 4, P, P, P, BIG, None), -1, 'nmf_h_half: x must be 4-byte aligned, w, ht, violation and the workspace 8-byte aligned'),
    ("mmk_nmf_h_half_f64", (P, 8, 8, 8, 2, P, P, P, P, 8, None), -4, 'nmf_h_half: the workspace has 8 bytes, 208 are needed'),
    ("mmk_nmf_solve_f64", (P, 8, 8, 8, 0, P, P, 1, 1e-4, 10, 0, 0, P, P, BIG, None), -1, 'nmf_solve: n_components = 0 must be at least 1'),
    ("mmk_nmf_solve_f64", (P, 8, 8, 8, 2, P, P, 1, 1e-4, 10, 0, 0, P, None, BIG, None), -1, 'nmf_solve: bad arguments (null pointer or negative stride 8)'),
    ("mmk_nmf_solve_f64", (P + 2, 8, 8, 8, 2, P, P, 1, 1e-4, 10, 0, 0, P, P, BIG, None), -1, 'nmf_solve: x must be 4-byte aligned, w, ht, violation and the workspace 8-byte aligned'),
    ("mmk_nmf_solve_f64", (P, 8, 8, 8, 2, P, P + 4, 1, 1e-4, 10, 0, 0, P, P, BIG, None), -1, 'nmf_solve: x must be 4-byte aligned, w, ht, violation and the workspace 8-byte aligned'),
    ("mmk_nmf_solve_f64", (P, 8, 8, 8, 2, P, P, 1, 1e-4, 10, 0, 0, P, P + 4, BIG, None), -1, 'nmf_solve: x must be 4-byte aligned, w, ht, violation and the workspace 8-byte aligned'),
    ("mmk_nmf_solve_f64", (P, 8, 8, 8, 2, P, P, 1, 1e-4, 10, 0, 0, P, P, 8, None), -4, 'nmf_solve: the workspace has 8 bytes, 272 are needed'),
    # ---- samplify.hip
    ("mmk_spline2_coef_f64", (None, 8, 1, 8, P, 8, None), -1, 'spline2_coef: bad arguments (batch=1, n=8, row strides 8 / 8)'),
    ("mmk_spline2_coef_f64", (P, 8, 2, 8, P, 7, None), -1, 'spline2_coef: bad arguments (batch=2, n=8, row strides 8 / 7)'),
    ("mmk_spline2_coef_f64", (P + 2, 8, 1, 8, P, 8, None), -1, 'spline2_coef: y must be 4-byte and coef 8-byte aligned'),
    ("mmk_spline2_coef_f64", (P + 4, 8, 1, 8, P + 4, 8, None), -1, 'spline2_coef: y must be 4-byte and coef 8-byte aligned'),
    ("mmk_spline2_coef_f64", (P + 4, 8, 1, 2, P, 8, None), -1, 'spline2_coef: a quadratic spline needs n >= 3 knots, got 2'),
    ("mmk_spline2_eval_f32", (None, 8, 1, 8, P, 8, 8, None), -1, 'spline2_eval: bad arguments (batch=1, n=8, n_out=8, row strides 8 / 8)'),
    ("mmk_spline2_eval_f32", (P, 8, 2, 8, P, 7, 8, None), -1, 'spline2_eval: bad arguments (batch=2, n=8, n_out=8, row strides 8 / 7)'),
    ("mmk_spline2_eval_f32", (P, 8, 1, 8, P + 2, 8, 8, None), -1, 'spline2_eval: out must be 4-byte aligned'),
    ("mmk_spline2_eval_f32", (P + 4, 8, 1, 8, P + 4, 8, 8, None), -1, 'spline2_eval: the coefficients must be a float64 device pointer, 8-byte aligned'),
    ("mmk_spline2_eval_f32", (P, 8, 1, 2, P, 8, 8, None), -1, 'spline2_eval: a quadratic spline needs n >= 3 knots, got 2'),
    ("mmk_periods_count_i64", (P, 8, P, 8, P, P, BIG, None), -1, 'periods_count: exactly one of coef (a spline) and row (its samples) must be given'),
    ("mmk_periods_count_i64", (None, 8, None, 8, P, P, BIG, None), -1, 'periods_count: exactly one of coef (a spline) and row (its samples) must be given'),
    ("mmk_periods_count_i64", (P + 4, 8, None, 8, P, P, BIG, None), -1, 'periods_count: the coefficients must be a float64 device pointer, 8-byte aligned'),
    ("mmk_periods_count_i64", (P, 2, None, 8, P, P, BIG, None), -1, 'periods_count: a quadratic spline needs n >= 3 knots, got 2'),
    ("mmk_periods_count_i64", (None, 8, P + 2, 8, P, P, BIG, None), -1, 'periods_count: row must be a float32 device pointer, 4-byte aligned'),
    ("mmk_periods_count_i64", (P, 8, None, 0, P, P, BIG, None), -1, 'periods_count: n_samples = 0 < 1'),
    ("mmk_periods_count_i64", (P, 8, None, 1 << 42, P, P, BIG, None), -3, 'periods_count: 4294967296 tiles of 1024 samples are more than one launch takes'),
    ("mmk_periods_count_i64", (P, 8, None, 8, P, None, BIG, None), -4, 'periods_count: 16 bytes of 8-byte aligned workspace are needed, got 1073741824'),
    ("mmk_periods_count_i64", (None, 8, P + 4, 8, P, P + 4, BIG, None), -4, 'periods_count: 16 bytes of 8-byte aligned workspace are needed, got 1073741824'),
    ("mmk_periods_count_i64", (P, 8, None, 8, P, P, 8, None), -4, 'periods_count: 16 bytes of 8-byte aligned workspace are needed, got 8'),
    ("mmk_periods_count_i64", (P, 8, None, 8, None, P, BIG, None), -1, 'periods_count: counts must be an int64[2] device pointer'),
    ("mmk_periods_count_i64", (P, 8, None, 8, P + 4, P, BIG, None), -1, 'periods_count: counts must be an int64[2] device pointer'),
    ("mmk_periods_fill_i64", (P + 4, 8, None, 8, P, BIG, 2, 2, P, P, P, None), -1, 'periods_fill: the coefficients must be a float64 device pointer, 8-byte aligned'),
    ("mmk_periods_fill_i64", (P, 8, None, 8, P + 4, BIG, 2, 2, P, P, P, None), -4, 'periods_fill: 16 bytes of 8-byte aligned workspace are needed, got 1073741824'),
    ("mmk_periods_fill_i64", (P, 8, None, 8, P, 8, 2, 2, P, P, P, None), -4, 'periods_fill: 16 bytes of 8-byte aligned workspace are needed, got 8'),
    ("mmk_periods_fill_i64", (P, 8, None, 8, P, BIG, -1, 2, P, P, P, None), -1, 'periods_fill: n_att = -1 / n_peak = 2 of 8 samples (two of a kind are at least two samples apart)'),
    ("mmk_periods_fill_i64", (P, 8, None, 8, P, BIG, 2, 2, None, P, P, None), -1, 'periods_fill: att, dec and peaks must be int64 device pointers'),
    ("mmk_periods_fill_i64", (P, 8, None, 8, P, BIG, 2, 2, P + 4, P, P, None), -1, 'periods_fill: att, dec and peaks must be int64 device pointers'),
    ("mmk_periods_fill_i64", (P, 8, None, 8, P, BIG, 2, 2, P, P + 4, P, None), -1, 'periods_fill: att, dec and peaks must be int64 device pointers'),
    ("mmk_periods_fill_i64", (P, 8, None, 8, P, BIG, 2, 2, P, P, P + 4, None), -1, 'periods_fill: att, dec and peaks must be int64 device pointers'),
    ("mmk_samplify_scores_f32", (None, 8, 8, P, P, 2, 0.0, P, P, P, P, None), -1, 'samplify_scores: the coefficients must be a float64 device pointer, 8-byte aligned'),
    ("mmk_samplify_scores_f32", (P + 4, 8, 8, P, P, 2, 0.0, P, P, P, P, None), -1, 'samplify_scores: the coefficients must be a float64 device pointer, 8-byte aligned'),
    ("mmk_samplify_scores_f32", (P, 2, 8, P, P, 2, 0.0, P, P, P, P, None), -1, 'samplify_scores: a quadratic spline needs n >= 3 knots, got 2'),
    ("mmk_samplify_scores_f32", (P, 8, 0, P, P, 2, 0.0, P, P, P, P, None), -1, 'samplify_scores: n_samples = 0, count = 2'),
    ("mmk_samplify_scores_f32", (P, 8, 8, P, P, 2, 0.0, P, P, P, None, None), -1, 'samplify_scores: att / dec must be int64, scores / env_att / env_dec float32 and keep uint8 device pointers'),
    ("mmk_samplify_scores_f32", (P, 8, 8, P + 4, P, 2, 0.0, P, P, P, P, None), -1, 'samplify_scores: att / dec must be int64, scores / env_att / env_dec float32 and keep uint8 device pointers'),
    ("mmk_samplify_scores_f32", (P, 8, 8, P, P + 4, 2, 0.0, P, P, P, P, None), -1, 'samplify_scores: att / dec must be int64, scores / env_att / env_dec float32 and keep uint8 device pointers'),
    ("mmk_samplify_scores_f32", (P, 8, 8, P, P, 2, 0.0, P + 2, P, P, P, None), -1, 'samplify_scores: att / dec must be int64, scores / env_att / env_dec float32 and keep uint8 device pointers'),
    ("mmk_samplify_scores_f32", (P, 8, 8, P, P, 2, 0.0, P, P, P + 2, P, None), -1, 'samplify_scores: att / dec must be int64, scores / env_att / env_dec float32 and keep uint8 device pointers'),
    ("mmk_samplify_cuts_i64", (P, 8, COEFS, COEFS, KNOTS, 0, P, P, 2, P, None, P, None), -1, 'samplify_cuts: levels = 0, 1 .. 6 (MMK_SAMPLIFY_MAX_LEVELS) are taken'),
    ("mmk_samplify_cuts_i64", (P, 8, COEFS, COEFS, KNOTS, 7, P, P, 2, P, None, P, None), -3, 'samplify_cuts: levels = 7, 1 .. 6 (MMK_SAMPLIFY_MAX_LEVELS) are taken'),
    ("mmk_samplify_cuts_i64", (None, 8, COEFS, COEFS, KNOTS, 2, P, P, 2, P, None, P, None), -1, 'samplify_cuts: bad arguments (n_samples = 8, count = 2)'),
    ("mmk_samplify_cuts_i64", (P + 2, 8, COEFS, COEFS, KNOTS, 2, P, P, 2, P, None, P, None), -1, 'samplify_cuts: bad arguments (n_samples = 8, count = 2)'),
    ("mmk_samplify_cuts_i64", (P, 8, COEFS, None, KNOTS, 2, P, P, 2, P, None, P, None), -1, 'samplify_cuts: bad arguments (n_samples = 8, count = 2)'),
    ("mmk_samplify_cuts_i64", (P, 8, SKEWED, COEFS, KNOTS, 2, P, P, 2, P, None, P, None), -1, 'samplify_cuts (env): the coefficients must be a float64 device pointer, 8-byte aligned'),
    ("mmk_samplify_cuts_i64", (P, 8, COEFS, SKEWED, KNOTS, 2, P, P, 2, P, None, P, None), -1, 'samplify_cuts (grad): the coefficients must be a float64 device pointer, 8-byte aligned'),
    ("mmk_samplify_cuts_i64", (P, 8, COEFS, COEFS, KNOTS, 2, None, P, 2, P, None, P, None), -1, 'samplify_cuts: coarse_cuts / coarse_peaks / sides / cuts must be int64 device pointers, lr_scores float32 or NULL'),
    ("mmk_samplify_cuts_i64", (P, 8, COEFS, COEFS, KNOTS, 2, P + 4, P, 2, P, None, P, None), -1, 'samplify_cuts: coarse_cuts / coarse_peaks / sides / cuts must be int64 device pointers, lr_scores float32 or NULL'),
    ("mmk_samplify_cuts_i64", (P, 8, COEFS, COEFS, KNOTS, 2, P, P, 2, P + 4, None, P, None), -1, 'samplify_cuts: coarse_cuts / coarse_peaks / sides / cuts must be int64 device pointers, lr_scores float32 or NULL'),
    ("mmk_samplify_cuts_i64", (P, 8, COEFS, COEFS, KNOTS, 2, P, P, 2, P, P + 2, P, None), -1, 'samplify_cuts: coarse_cuts / coarse_peaks / sides / cuts must be int64 device pointers, lr_scores float32 or NULL'),
    ("mmk_samplify_cuts_i64", (P, 8, COEFS, COEFS, KNOTS, 2, P, P, 2, P, None, P + 4, None), -1, 'samplify_cuts: coarse_cuts / coarse_peaks / sides / cuts must be int64 device pointers, lr_scores float32 or NULL'),
    # ---- hpss.hip
    ("mmk_hpss_f32", (None, 64, 8, 1, 8, 8, 3, 3, 1.0, 1.0, 1.0, P, None, None, None, 64, 8, None), -1, 'hpss: bad arguments (s (nil), batch 1, frames 8, bins 8)'),
    ("mmk_hpss_f32", (P, 64, 8, 1, 8, 8, 3, 3, 1.0, 1.0, 1.0, None, None, None, None, 64, 8, None), -1, 'hpss: no output requested'),
    ("mmk_hpss_f32", (P, 64, 8, 1, 8, 8, 0, 3, 1.0, 1.0, 1.0, P, None, None, None, 64, 8, None), -1, 'hpss: windows must be at least 1, got (0, 3)'),
    ("mmk_hpss_f32", (P, 64, 8, 1, 8, 8, 64, 3, 1.0, 1.0, 1.0, P, None, None, None, 64, 8, None), -3, 'hpss: windows (64, 3), the limit is 63'),
    ("mmk_hpss_f32", (P, 64, 8, 1, 8, 8, 31, 3, 1.0, 1.0, 1.0, P, None, None, None, 64, 8, None), -1, 'hpss: windows (31, 3) fold an axis of (8 frames, 8 bins) more than once: each axis needs at least win / 2'),
    ("mmk_hpss_f32", (P, 64, 8, 1, 8, 8, 3, 3, 1.0, 0.5, 1.0, P, None, None, None, 64, 8, None), -1, 'hpss: margins must be at least 1, got (0.5, 1)'),
    ("mmk_hpss_f32", (P, 64, 8, 1, 8, 8, 3, 3, 0.0, 1.0, 1.0, P, None, None, None, 64, 8, None), -1, 'hpss: power must be positive, got 0'),
    ("mmk_hpss_f32", (P, 64, 7, 1, 8, 8, 3, 3, 1.0, 1.0, 1.0, P, None, None, None, 64, 8, None), -1, 'hpss: strides (s 64 / 7, out 64 / 8) for 1 clips of (8, 8)'),
    ("mmk_hpss_f32", (P + 2, 64, 8, 1, 8, 8, 3, 3, 1.0, 1.0, 1.0, P, None, None, None, 64, 8, None), -1, 'hpss: s and the outputs must be 4-byte aligned'),
    ("mmk_hpss_f32", (P, 64, 8, 1, 8, 8, 3, 3, 1.0, 1.0, 1.0, P + 2, None, None, None, 64, 8, None), -1, 'hpss: s and the outputs must be 4-byte aligned'),
    ("mmk_hpss_f32", (P, 64, 8, 1, 8, 8, 3, 3, 1.0, 1.0, 1.0, None, P + 1, None, None, 64, 8, None), -1, 'hpss: s and the outputs must be 4-byte aligned'),
    ("mmk_hpss_f32", (P, 64, 8, 1, 8, 8, 3, 3, 1.0, 1.0, 1.0, None, None, P + 2, None, 64, 8, None), -1, 'hpss: s and the outputs must be 4-byte aligned'),
    ("mmk_hpss_f32", (P, 64, 8, 1, 8, 8, 3, 3, 1.0, 1.0, 1.0, None, None, None, P + 3, 64, 8, None), -1, 'hpss: s and the outputs must be 4-byte aligned'),
    # ---- novelty.hip
    ("mmk_novelty_f32", (P, 64, 8, None, 0, 8, 8, P, 2, P, None), -1, 'novelty: batch = 0 < 1'),
    ("mmk_novelty_f32", (P, 64, 8, None, 1, 1, 8, P, 2, P, None), -1, 'novelty: frames = 1 < 2 (a board needs two frames)'),
    ("mmk_novelty_f32", (P, 64, 8, None, 1, 8, 0, P, 2, P, None), -1, 'novelty: bins = 0 < 1'),
    ("mmk_novelty_f32", (P, 64, 8, None, 1, 8, 8, None, 2, P, None), -1, 'novelty: bad arguments (null pointer or negative stride 64 / 8)'),
    ("mmk_novelty_f32", (P, 64, -8, None, 1, 8, 8, P, 2, P, None), -1, 'novelty: bad arguments (null pointer or negative stride 64 / -8)'),
    ("mmk_novelty_f32", (P + 2, 64, 8, None, 1, 8, 8, P, 2, P, None), -1, 'novelty: x, inv_norm and raw must be 4-byte aligned'),
    ("mmk_novelty_f32", (P, 64, 8, P + 2, 1, 8, 8, P, 2, P, None), -1, 'novelty: x, inv_norm and raw must be 4-byte aligned'),
    ("mmk_novelty_f32", (P, 64, 8, None, 1, 8, 8, P, 2, P + 2, None), -1, 'novelty: x, inv_norm and raw must be 4-byte aligned'),
    ("mmk_novelty_finish_f32", (P, 0, 2, 8, P, P, P, BIG, None), -1, 'novelty_finish: batch = 0, frames = 8: both must be >= 1'),
    ("mmk_novelty_finish_f32", (P, 1, 0, 8, P, P, P, BIG, None), -1, 'novelty_finish: n_half = 0 < 1'),
    ("mmk_novelty_finish_f32", (P, 1, 9, 8, P, P, P, BIG, None), -3, 'novelty_finish: 9 half-widths, the limit is 8 (MMK_NOVELTY_MAX_KERNELS)'),
    ("mmk_novelty_finish_f32", (P, 1, 2, 8, P, P, None, BIG, None), -1, 'novelty_finish: bad arguments (null or misaligned pointer)'),
    ("mmk_novelty_finish_f32", (P + 2, 1, 2, 8, P, P, P, BIG, None), -1, 'novelty_finish: bad arguments (null or misaligned pointer)'),
    ("mmk_novelty_finish_f32", (P, 1, 2, 8, P, P + 2, P, BIG, None), -1, 'novelty_finish: bad arguments (null or misaligned pointer)'),
    ("mmk_novelty_finish_f32", (P, 1, 2, 8, P, P, P + 2, BIG, None), -1, 'novelty_finish: bad arguments (null or misaligned pointer)'),
    ("mmk_novelty_finish_f32", (P, 1, 2, 8, P, P, P, 1, None), -4, 'novelty_finish: the workspace has 1 floats, 2 are needed'),
    ("mmk_pick_peaks_f32", (P, 0, 2, 2, 0.02, P, P, BIG, None), -1, 'pick_peaks: n = 0 < 1'),
    ("mmk_pick_peaks_f32", (P, 8, -1, 2, 0.02, P, P, BIG, None), -1, 'pick_peaks: wait_before = -1, wait_after = 2: neither may be negative and one must be positive'),
    ("mmk_pick_peaks_f32", (P, 8, 1025, 2, 0.02, P, P, BIG, None), -3, 'pick_peaks: wait_before = 1025, wait_after = 2, the limit is 1024 (MMK_NOVELTY_MAX_WAIT)'),
    ("mmk_pick_peaks_f32", (P, 8, 2, 2, NAN, P, P, BIG, None), -1, 'pick_peaks: min_strength is NaN'),
    ("mmk_pick_peaks_f32", (P, 8, 2, 2, 0.02, None, P, BIG, None), -1, 'pick_peaks: bad arguments (null or misaligned pointer)'),
    ("mmk_pick_peaks_f32", (P, 8, 2, 2, 0.02, P, None, BIG, None), -1, 'pick_peaks: bad arguments (null or misaligned pointer)'),
    ("mmk_pick_peaks_f32", (P + 2, 8, 2, 2, 0.02, P, P, BIG, None), -1, 'pick_peaks: bad arguments (null or misaligned pointer)'),
    ("mmk_pick_peaks_f32", (P, 8, 2, 2, 0.02, P, P + 2, BIG, None), -1, 'pick_peaks: bad arguments (null or misaligned pointer)'),
    ("mmk_pick_peaks_f32", (P, 8, 2, 2, 0.02, P, P + 4, 8, None), -4, 'pick_peaks: the workspace has 8 bytes, 40 are needed'),
    ("mmk_pick_peaks_f32", (P, 8, 2, 2, 0.02, P, P, 0, None), -4, 'pick_peaks: the workspace has 0 bytes, 40 are needed'),
]


@pytest.mark.parametrize("row", range(len(ROWS)), ids=lambda i: f"{ROWS[i][0]}-{i}")
def test_the_entry_point_refuses_with_this_code_and_this_text(row):
    name, args, code, text = ROWS[row]
    assert code in (-1, -3, -4), "a row must be refused before any launch"
    assert call(name, args) == (code, text), (name, args)


def test_every_entry_point_that_checks_through_entry_util_has_rows():
    covered = {r[0] for r in ROWS}
    assert covered == {
        "mmk_lfilter1_f32", "mmk_row_normalize_f32", "mmk_interp1d_f32", "mmk_derivative_f32", "mmk_inv_row_norm_f32", "mmk_cosine_cost_f32",
        "mmk_dtw_subseq_f32", "mmk_nn_cosine_f32", "mmk_nn_cosine_self_f32", "mmk_cum_entropy_i64", "mmk_nn_components_i64",
        "mmk_edge_components_i64", "mmk_segment_mean_f32", "mmk_nn_topk_f32", "mmk_half_neg_sqnorm_f32", "mmk_kmeans_assign_f32",
        "mmk_kmeans_label_sums_f64", "mmk_kmeans_pp_step_f64", "mmk_nn_aggregate_f32", "mmk_pca_colstats_f64", "mmk_pca_cov_f64",
        "mmk_pca_eig_f64", "mmk_pca_project_f32", "mmk_nmf_start_f64", "mmk_nmf_w_half_f64", "mmk_nmf_h_half_f64", "mmk_nmf_solve_f64",
        "mmk_spline2_coef_f64", "mmk_spline2_eval_f32", "mmk_periods_count_i64", "mmk_periods_fill_i64", "mmk_samplify_scores_f32",
        "mmk_samplify_cuts_i64", "mmk_hpss_f32", "mmk_novelty_f32", "mmk_novelty_finish_f32", "mmk_pick_peaks_f32"}
