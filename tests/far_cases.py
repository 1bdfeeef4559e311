"""Strides beyond 4 GiB (include/mmk.h, conventions: strides): layouts, the table of stride parameters and the cases, shared by
tests/test_far_cases.py (no GPU) and tests/test_gpu_far_offsets.py.  Nothing here allocates: the module is arithmetic on word offsets.

The canvas.  One fp32 device buffer of CANVAS = LEAD + FIELD words (a word is 4 bytes) holds every strided operand of a case: a lead-in
of LEAD = 2^29 words (2 GiB) and behind it the field of FIELD = 2^31 + 2^24 words, about 10.1 GiB together.  The canvas is filled with
NaN (bit pattern NAN_BITS in every word; operands of 8-byte types view the same storage and see two such words).  A byte offset that a
kernel narrowed to a SIGNED 32 bits lands up to 2 GiB below the operand's base: inside the lead-in, where the scan finds a write and a
read returns fill.

A FarLayout places the rows (or clips) of every strided operand of a case in the field, the rows of an operand a far stride apart and
the operands side by side, each in a lane of 2^15 words and more.  Operands of one row count have one stride, so their rows i share
slot i; an operand with another row count has its own stride (its last row reaches the mark too) and its lane keeps it clear of the others.
  'far'  the last row begins MARK_FAR = 2^31 words or more from the operand's base: 2^33 bytes, an element offset of 2^31 or more for
         the 4-byte types;
  'mid'  the last row begins between 2^31 and 2^32 BYTES from the base (MARK_MID = 2^29 words): the mark a signed 32-bit byte offset
         wraps at, which 'far' may step over when an operand has two or three rows.  Every case has both.
An entry with a batch stride and a row stride has both layouts on either axis ('rows', 'batch'); the other axis keeps a near stride.
Far strides carry SKEW = 2^22 words on top of the mark, so that an offset narrowed to 32 bits does not land on row 0 again but on fill.

The near twin is the same case in a buffer of a few kilobytes: the same shapes, every base address equal to the far one modulo 256
bytes, every stride congruent modulo 64 elements.  The launchers choose vector or scalar paths from `ld % 4` and `ptr & 15`; two
layouts of one class take the same path and differ in nothing but the size of the offsets, so their outputs are equal bit for bit.
Two alignment classes: 0 - bases 16-byte (in fact 256-byte) aligned, strides multiples of 4 (of 64 plus the near part); 1 - bases one
element in (4 bytes for the 4-byte types, 8 for the 8-byte ones, which must stay 8-byte aligned) and odd strides.  FarCase.odd says
whether the entry runs class 1 or refuses it (the gemm family: A must be 16-byte aligned with lda % 4 == 0).

The table, FAR_PARAMS: every `int64_t` parameter of the five headers that is a stride or a leading dimension (header_stride_params),
as 'function.parameter', under exactly one of FAR (the id of its FarCase or plan test) and NOT_FAR (the reason).

LIMITS OF THE METHOD
  - 8-byte operands (int64 classes and indices, float64 coefficients): their last row begins 2^33 bytes from the base like everyone's,
    but that is an element offset of 2^30: an element offset of 2^31 of an 8-byte type needs a 16 GiB field.  A 32-bit ELEMENT offset of
    such an operand is not seen to wrap here.
  - the signed narrowing of an element offset (an `int` row index times an `int` stride) lands 8 GiB below the base, outside any
    lead-in that fits: such a defect would leave the canvas.  It is looked for by reading the kernels' address arithmetic, not by
    running them; the unsigned narrowing of an element offset does not wrap below 2^32 elements (16 GiB) at all and is invisible here.
    What the canvas sees: a byte offset narrowed to uint32 (wraps at 2^32 bytes) or to int32 (at 2^31 bytes), which is what a
    buffer-resource offset or an (int) cast of `row * stride * sizeof(float)` gives.
  - tests/test_gpu_far_offsets.py skips, with the figures in the message, when torch.cuda.mem_get_info reports less free memory than
    the canvas plus 1 GiB.
  - the far outputs are held to the family's own float64 restatement and bound wherever tests/f64_bounds.py or the family's *_refs
    module has one that takes the case's inputs (FarCase.bound: resample, lfilter1, row_normalize, cosine_cost, cum_entropy, novelty,
    pca_colstats, stft_mag, stft and stft_energy on the three kernel families, interp1d, derivative, hpss, melbank, the gemm family,
    attention, layer norm, kmeans_label_sums, nn_aggregate).  The rest are held to the near twin's bits alone:
      nn_cosine, nn_cosine_self, nn_topk, kmeans_assign, kmeans_pp_step, categorical_sample - their outputs are indices, labels or picks,
        and their refs modules state rules on margins between candidates, not bounds on values;
      pca_cov, pca_project - pca_refs' bounds take the restatement's own statistics, z and components (dict p of pca64), where the stream
        case passes torch's mean and scale and a QR basis;
      nmf start / solve / half steps - nmf_refs' sweep_bound and start_bound take the previous iterate and the device's own V;
      segment_mean - hcluster_refs builds reference and bound inside mean_case(k), for its own rows;
      spline2_coef, spline2_eval - samplify_refs.spline_ref bounds the evaluated curve of samples y; the two stream cases stop at the
        coefficients, or start from drawn ones;
      stft_mel - melspec_refs bounds the bank on given magnitudes (bank_bound); no function composes it with the transform's error;
      inv_row_norm, half_neg_sqnorm - nnn_refs and qcluster_refs fold their error into cost_bound / key_bound, which cosine_cost covers here;
      pack_weight - a permutation: bits.
  - the only NOT_FAR entries are mmk_wavenet_profile_steps' two strides; every other stride parameter has a case or the plan test.
"""
import bisect
import ctypes as C
import math
import re
from pathlib import Path

import numpy as np
import torch

from tests import f64_bounds as B
from tests import stream_cases as S

ROOT = Path(__file__).resolve().parent.parent
HEADERS = ("mmk.h", "mmk_kmeans.h", "mmk_nmf.h", "mmk_nn_filter.h", "mmk_samplify.h")

WORD = 4
LEAD = 2 ** 29
FIELD = 2 ** 31 + 2 ** 24
CANVAS = LEAD + FIELD
MARK_FAR = 2 ** 31              # words: 2^33 bytes, 2^31 elements of a 4-byte type
MARK_MID = 2 ** 29              # words: 2^31 bytes
SKEW = 2 ** 22                  # words on top of a mark
NAN_BITS = 0x7FC00000           # what tensor.fill_(nan) writes
SCAN_CHUNK = 2 ** 28
MARKS = {"far": MARK_FAR, "mid": MARK_MID}
assert FIELD - 2 ** 24 >= 2 ** 31 and MARK_MID + SKEW + 2 ** 24 < 2 ** 30


# ====================================================================================================================== the headers
def header_texts():
    return {h: (ROOT / "include" / h).read_text() for h in HEADERS}


_STRIDE_NAME = re.compile(r"(_stride|^ld[a-z]?|_ld|^[ac]_batch|_cs)$")


def header_stride_params(texts=None):
    """'function.parameter' for every int64_t (or int64_t array) parameter of the five headers named like a stride or leading dimension;
    prototypes are found the way stream_cases.header_stream_functions finds them"""
    found = []
    for text in (header_texts() if texts is None else texts).values():
        text = re.sub(r"//[^\n]*", " ", re.sub(r"/\*.*?\*/", " ", text, flags=re.S))
        for m in re.finditer(r"\b(mmk_[a-z0-9_]+)\s*\(([^;{}]*?)\)\s*;", text):
            for p in m.group(2).split(","):
                words = p.replace("*", " ").split()
                if "int64_t" in words and _STRIDE_NAME.search(words[-1]):
                    found.append(f"{m.group(1)}.{words[-1]}")
    return sorted(found)


# ====================================================================================================================== layouts
def roundup(v, m):
    return -(-int(v) // m) * m


def near_stride(k, cls):
    """the stride of the axis that stays near: more than a row, a multiple of 4 (class 0) or odd (class 1)"""
    return roundup(k, 4) + 4 if cls == 0 else (k + 2) | 1


class Placed:
    """one strided operand in a buffer: (B, R, K) elements of `ew` words each, strides s0 (batch) and s1 (rows) in elements, base `off`
    words from the buffer's start; far_axis: 0 (batch) or 1 (rows); levels: 1 (rows only: B == 1) or 2"""

    def __init__(self, name, ew, levels, B_, R, K, s0, s1, off, far_axis):
        self.name, self.ew, self.levels, self.B, self.R, self.K, self.s0, self.s1, self.off, self.far_axis = name, ew, levels, B_, R, K, s0, s1, off, far_axis

    @property
    def far_count(self):
        return self.B if self.far_axis == 0 else self.R

    @property
    def far_stride(self):
        return self.s0 if self.far_axis == 0 else self.s1

    @property
    def slot_words(self):
        """what one slot holds of this operand: the near axis' rows"""
        n, s = (self.R, self.s1) if self.far_axis == 0 else (self.B, self.s0)
        return ((n - 1) * s + self.K) * self.ew

    def intervals(self):
        """[start, end) in words of every row"""
        return [(self.off + (b * self.s0 + r * self.s1) * self.ew, self.off + (b * self.s0 + r * self.s1 + self.K) * self.ew)
                for b in range(self.B) for r in range(self.R)]

    def last_row_words(self):
        return (self.far_count - 1) * self.far_stride * self.ew


class FarLayout:
    def __init__(self, axis, mark, cls, far, twin, twin_words):
        self.axis, self.mark, self.cls, self.far, self.twin, self.twin_words = axis, mark, cls, far, twin, twin_words

    @property
    def id(self):
        return f"{self.axis}-{self.mark}-c{self.cls}"


def to_u32(b):
    return b % 2 ** 32


def to_i32(b):
    return (b + 2 ** 31) % 2 ** 32 - 2 ** 31


def wrapped_rows(p):
    """for every slot of a far operand and each narrowing the canvas can see: (narrowing, slot, wrapped word offset of the slot from the
    buffer's start, true one).  'elements->uint32' is listed to show that it is the identity inside this canvas (module docstring)."""
    out = []
    for i in range(p.far_count):
        e = i * p.far_stride
        b = e * p.ew * WORD
        for name, w in (("bytes->uint32", to_u32(b)), ("bytes->int32", to_i32(b)), ("elements->uint32", to_u32(e) * p.ew * WORD)):
            out.append((name, i, p.off + w // WORD, p.off + b // WORD))
    return out


def touched(placed):
    return sorted(iv for p in placed for iv in p.intervals())


def hits(ivs, lo, hi):
    """does [lo, hi) meet one of the sorted, disjoint intervals"""
    k = bisect.bisect_right(ivs, (lo, math.inf))
    return (k > 0 and ivs[k - 1][1] > lo) or (k < len(ivs) and ivs[k][0] < hi)


def problems(placed, words):
    """what is wrong with a placement in a buffer of `words` words: rows outside it or on one another, a narrowed offset that lands
    outside the buffer or on a row of the case"""
    ivs = touched(placed)
    bad = [f"row [{a}, {b}) outside the field" for a, b in ivs if a < LEAD or b > words]
    bad += [f"rows [{a}, {b}) and [{c}, {d}) overlap" for (a, b), (c, d) in zip(ivs, ivs[1:]) if c < b]
    for p in placed:
        for name, i, w, true in wrapped_rows(p):
            if w != true and (w < 0 or w + p.slot_words > words or hits(ivs, w, w + p.slot_words)):
                bad.append(f"{p.name}: slot {i} under {name} lands at word {w}: outside the canvas or on the case's own rows")
    return bad


def build_layout(specs, axis, mark, cls):
    """specs: [(name, ew, levels, B, R, K)].  -> FarLayout: the far placement in the canvas and its near twin"""
    for bump in range(32):
        # (operands with other row counts have other strides, rounded apart by up to 65 words a row: a lane of 2^15 words each keeps the
        #  rows of one from drifting onto the rows of the next; `bump` tries further apart)
        far, twin, cum, tcum, lane = [], [], 0, 64, 2 ** 15 + bump * 64 * 37
        for name, ew, levels, B_, R, K in specs:
            far_axis = 0 if (levels == 2 and B_ > 1 and axis == "batch") else 1
            n, ni = (B_, R) if far_axis == 0 else (R, B_)
            si = near_stride(K, cls)
            extent = (ni - 1) * si + K
            big = roundup(-(-(MARKS[mark] + SKEW) // ((max(n, 2) - 1) * ew)), 64) + cls
            small = roundup(extent + 1, 64) + 64 + cls
            strides = (lambda s: (s, si) if far_axis == 0 else (si, s))
            far.append(Placed(name, ew, levels, B_, R, K, *strides(big), LEAD + cum + cls * ew, far_axis))
            twin.append(Placed(name, ew, levels, B_, R, K, *strides(small), tcum + cls * ew, far_axis))
            cum += roundup(extent * ew, 64) + lane
            tcum += roundup(((n - 1) * small + extent) * ew, 64) + 64
        if not problems(far, CANVAS):
            return FarLayout(axis, mark, cls, far, twin, tcum + 64)
    raise AssertionError(("no placement found", [s[0] for s in specs], axis, mark, cls, problems(far, CANVAS)[:3]))


# ====================================================================================================================== the cases
P = S.P


class FarCase:
    """case: the stream Case whose build / outs / work / const / setup / ref are reused; ops: {operand: levels} - the strided operands
    (1: rows, 2: batch and rows), inputs and outputs alike; call(L, a, s): like Case.call, but a[operand] is a strided VIEW of the
    buffer (its data_ptr is the base, its stride() what the entry is given; 1 level: (R, K), 2 levels: (B, R, K)); params: the
    'function.parameter's the case drives; odd: 'runs' or 'refused' (class 1); stack: operands and outputs drawn twice and stacked
    along the batch (the stream cases with one clip); bound(i) -> {output: (float64 reference, the family's bound from tests/f64_bounds.py)};
    axes: the layouts' far axes where the entry's contract rules one out (default: 'rows', and 'batch' where an operand has clips)"""

    def __init__(self, case, ops, call, params, odd="runs", stack=(), bound=None, tag=None, axes=None, reshape=None):
        self.case, self.ops, self.call, self.odd, self.stack, self.bound, self.axes = case, ops, call, odd, tuple(stack), bound, axes
        self.reshape = dict(reshape or {})                   # outputs seen as (groups, rows of a group, columns)
        self.id = tag or case.id
        self.params = tuple(f"{case.entry}.{p}" if "." not in p else p for p in params)

    def build(self, seed):
        i = self.case.build(seed)
        if self.stack:
            j = self.case.build(seed + 1000)
            i = {k: torch.cat([v, j[k]]) if k in self.stack else v for k, v in i.items()}
        return i

    def outs(self, L, i):
        o = self.case.outs(L, self.case.build(0))
        o = {k: ((2 * shape[0],) + tuple(shape[1:]), dt) if k in self.stack else (tuple(shape), dt) for k, (shape, dt) in o.items()}
        return {k: (self.reshape.get(k, shape), dt) for k, (shape, dt) in o.items()}

    def specs(self, L):
        i = self.build(0)
        o = self.outs(L, i)
        specs = []
        for name, levels in self.ops.items():
            shape, dtype = (tuple(i[name].shape), i[name].dtype) if name in i else o[name]
            ew = torch.empty((), dtype=dtype).element_size() // WORD
            assert ew in (1, 2), (self.id, name, dtype)
            lead = 2 if levels == 2 else 1
            specs.append((name, ew, levels, shape[0] if levels == 2 else 1, shape[lead - 1], math.prod(shape[lead:]) if len(shape) > lead else 1))
        return specs

    def layouts(self, L):
        specs = self.specs(L)
        axes = self.axes or ["rows"] + (["batch"] if any(levels == 2 and B_ > 1 for _, _, levels, B_, _, _ in specs) else [])
        classes = (0, 1)
        return [build_layout(specs, axis, mark, cls) for axis in axes for mark in ("far", "mid") for cls in classes]


def _rows(*names):
    return {n: 1 for n in names}


def _two(*names):
    return {n: 2 for n in names}


def _case(cid):
    return S.BY_ID[cid]


# ---- the families' own float64 restatements and bounds (tests/f64_bounds.py and the *_refs modules), on a case's inputs `i`:
# -> {output: (float64 reference, bound)} in the output's shape, both as tensors
def _pair(want, bound):
    t = lambda a: a.double() if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=np.float64)))
    want, bound = t(want), t(bound)
    return want, bound.expand(want.shape) if bound.shape != want.shape else bound


def _np64(t):
    return t.double().numpy()


def _bound_resample(i):
    return dict(out=_pair(*B.resample_ref(i["x"].double(), i["table"].double(), 2, 3, 6)))


def _bound_lfilter1(i):
    from tests import filter_refs as FR
    x = _np64(i["x"])
    return dict(y=_pair(FR.lfilter1_ref(x, *FR.REMOVE_DC), FR.lfilter1_bound(x, *FR.REMOVE_DC)))


def _bound_row_normalize(i):
    from tests import filter_refs as FR
    want = FR.normalize_ref(_np64(i["x"]), 2)
    return dict(y=_pair(want, FR.normalize_bound(want, 2, i["x"].shape[-1])))


def _bound_cosine_cost(i):
    """the device's (batch, m, n_pad) layout: the transposed distances, the padding holds exactly 1"""
    from mimikit_amd import native
    from tests import nnn_refs as NR
    x, y = i["x"].numpy(), i["y"].numpy()
    n = x.shape[1]
    want = np.ones((x.shape[0], y.shape[0], native.nnn_n_pad(n)))
    bound = np.zeros_like(want)
    want[..., :n], bound[..., :n] = NR.cosine_distances(x, y).transpose(0, 2, 1), NR.cost_bound(x, y).transpose(0, 2, 1)
    return dict(cost=_pair(want, bound))


def _bound_derivative(i):
    from tests import envelope_refs as ER
    x = _np64(i["x"])
    return dict(y=_pair(ER.derivative_ref(x, 3), ER.derivative_bound(x, 3)))


def _bound_stft(coord, n_fft):
    def bound(i):
        S_, fw = B.stft_ref(i["x"].double(), n_fft, n_fft // 4, False)
        want = B.stft_want(S_, coord)
        return dict(out=(want, B.stft_err_bound(want, S_, fw, coord)[1]))
    return bound


def _bound_hpss(i):
    """clip by clip: the soft outputs inside hpss_bound, the two medians scipy's own bits (a bound of 0)"""
    from tests import hpss_refs as HR
    s = i["s"].numpy()
    harm, perc, hm, pm, _ = HR.hpss64(s, 31)
    zero = np.zeros(s.shape)
    return dict(harmonic=_pair(harm, HR.hpss_bound(harm, s, 1.0)), percussive=_pair(perc, HR.hpss_bound(perc, s, 1.0)),
                harm_median=_pair(hm, zero), perc_median=_pair(pm, zero))


def _bound_melbank(i):
    from tests import melspec_refs as MR
    dense = np.zeros((S.MEL_BANDS, i["s"].shape[1]), dtype=np.float32)
    for m, (lo, length, at) in enumerate(i["band"].tolist()):
        dense[m, lo:lo + length] = i["weights"][at:at + length].numpy()
    want = MR.mel64(i["s"].numpy(), dense)
    return dict(out=_pair(want, MR.bank_bound(want, dense)))


def _bound_pca_colstats(i):
    from tests import pca_refs as PR
    p = PR.pca64(i["x"].numpy(), S.PCA_K)
    mean_bound, scale_bound = PR.stats_bounds(p)
    return dict(mean=_pair(p["mean"], mean_bound), scale=_pair(p["scale"], scale_bound))


def _bound_kmeans_sums(i):
    """sums, squared distances and inertia inside the family's bounds; the counts are exact (a bound of 0)"""
    from tests import kmeans_refs as KR
    k = i["centres"].shape[0]
    xp, labels = KR.centred(i["x"].numpy(), i["offset"].numpy()), i["labels"].numpy()
    want, counts, asum = KR.label_sums64(xp, labels, k)
    d2 = KR.row_d2_64(xp, labels, i["centres"].numpy())
    total, (n, d) = float(d2.sum()), xp.shape
    return dict(sums=_pair(want, KR.sums_bound(counts, asum) + 1e-300), counts=_pair(counts, np.zeros(k)),
                row_d2=_pair(d2, KR.d2_bound(d2, d) + 1e-300), inertia=_pair(np.array([total]), np.array([KR.total_bound(total, n, d) + 1e-300])))


def _bound_stft_energy(n_fft):
    def bound(i):
        from tests import envelope_refs as ER
        return dict(out=_pair(*ER.energy_ref(i["x"].double(), n_fft, n_fft // 4, 0, 0)))
    return bound


def _bound_interp1d(i):
    from tests import envelope_refs as ER
    n_out = S.BY_ID["mmk_interp1d_f32"].outs(None, i)["y"][0][1]
    return dict(y=_pair(*ER.interp_ref(_np64(i["x"]), n_out, "linear", 1)))


def _bound_cum_entropy(i):
    """row by row: the per-step entropies inside entropy_bound, the totals inside total_bound"""
    from tests import neighbors_refs as NR
    e64 = np.stack([NR.cum_entropy64(row.numpy()) for row in i["items"]])
    return dict(e=_pair(e64, NR.entropy_bound(e64) + 1e-300), total=_pair(e64.sum(-1), np.array([NR.total_bound(e) for e in e64])))


def _bound_novelty(i):
    """clip by clip (the case is stacked): the raw scores of every half width inside segment_refs.bounds' raw bound"""
    from tests import segment_refs as SR
    per_clip = [SR.bounds(x.double().numpy(), S.NOVELTY_HALVES) for x in i["x"]]
    return dict(raw=_pair(np.stack([b[0] for b in per_clip]), np.stack([b[3] for b in per_clip])))


def _bound_nn_aggregate(i):
    """op 0 of include/mmk_nn_filter.h on the lists as given (not mutual), as the far call asks for it; the counts are exact"""
    from tests import nn_filter_refs as FR
    out, counts, bound = FR.nn_aggregate64(i["x"].numpy(), i["index"].numpy(), FR.OPS[0], False)
    return dict(out=_pair(out, bound), count=_pair(counts, np.zeros(counts.shape)))


def _resample():
    def call(L, a, s):
        x, out = a["x"], a["out"]
        return L.mmk_resample_f32(P(x), x.stride(0), x.shape[0], x.shape[1], P(a["table"]), 2, 3, 6, P(out), out.stride(0), s)
    return FarCase(_case("mmk_resample_f32"), _rows("x", "out"), call, ("x_row_stride", "out_row_stride"), bound=_bound_resample)


def _lfilter1():
    from tests import filter_refs as FR
    b0, b1, a1 = FR.REMOVE_DC

    def call(L, a, s):
        x, y = a["x"], a["y"]
        return L.mmk_lfilter1_f32(P(x), x.stride(0), x.shape[0], x.shape[1], b0, b1, a1, P(y), y.stride(0), P(a["ws"]), s)
    return FarCase(_case("mmk_lfilter1_f32"), _rows("x", "y"), call, ("x_row_stride", "y_row_stride"), bound=_bound_lfilter1)


def _row_normalize():
    def call(L, a, s):
        x, y = a["x"], a["y"]
        return L.mmk_row_normalize_f32(P(x), x.stride(0), x.shape[0], x.shape[1], 2, 1e-12, P(y), y.stride(0), P(a["ws"]), s)
    return FarCase(_case("mmk_row_normalize_f32"), _rows("x", "y"), call, ("x_row_stride", "y_row_stride"), bound=_bound_row_normalize)


def _inv_row_norm():
    def call(L, a, s):
        x = a["x"]
        return L.mmk_inv_row_norm_f32(P(x), x.stride(0), x.stride(1), x.shape[0], x.shape[1], x.shape[2], P(a["out"]), s)
    return FarCase(_case("mmk_inv_row_norm_f32"), _two("x"), call, ("x_batch_stride", "x_row_stride"))


def _cosine_cost():
    def call(L, a, s):
        x, y = a["x"], a["y"]
        return L.mmk_cosine_cost_f32(P(x), x.stride(0), x.stride(1), P(a["rx"]), x.shape[0], x.shape[1], P(y), y.stride(0), P(a["ry"]), y.shape[0],
                                     y.shape[1], P(a["cost"]), s)
    return FarCase(_case("mmk_cosine_cost_f32"), {"x": 2, "y": 1}, call, ("x_batch_stride", "x_row_stride", "y_row_stride"), bound=_bound_cosine_cost)


def _nn_cosine():
    def call(L, a, s):
        x, y = a["x"], a["y"]
        return L.mmk_nn_cosine_f32(P(x), x.stride(0), P(a["rx"]), x.shape[0], P(y), y.stride(0), P(a["ry"]), y.shape[0], x.shape[1], P(a["index"]),
                                   P(a["best"]), P(a["ws"]), a["ws"].numel(), s)
    return FarCase(_case("mmk_nn_cosine_f32"), _rows("x", "y"), call, ("x_row_stride", "y_row_stride"))


def _cum_entropy():
    def call(L, a, s):
        items, e = a["items"], a["e"]
        return L.mmk_cum_entropy_i64(P(items), items.stride(0), items.shape[0], items.shape[1], P(a["total"]), P(e), e.stride(0), s)
    return FarCase(_case("mmk_cum_entropy_i64"), _rows("items", "e"), call, ("row_stride", "e_row_stride"), bound=_bound_cum_entropy)


def _nn_cosine_self():
    def call(L, a, s):
        x = a["x"]
        return L.mmk_nn_cosine_self_f32(P(x), x.stride(0), P(a["rx"]), x.shape[0], x.shape[1], P(a["index"]), P(a["best"]), P(a["ws"]), a["ws"].numel(), s)
    return FarCase(_case("mmk_nn_cosine_self_f32"), _rows("x"), call, ("x_row_stride",))


def _segment_mean():
    def call(L, a, s):
        x, out = a["x"], a["out"]
        return L.mmk_segment_mean_f32(P(x), x.stride(0), x.shape[0], x.shape[1], P(a["order"]), P(a["offsets"]), out.shape[0], P(out), out.stride(0), s)
    return FarCase(_case("mmk_segment_mean_f32"), _rows("x", "out"), call, ("x_row_stride", "out_row_stride"))


def _nn_topk():
    def call(L, a, s):
        x, y, t = a["x"], a["y"], a["index"].shape[1]
        return L.mmk_nn_topk_f32(P(x), x.stride(0), P(a["ones"]), x.shape[0], P(y), y.stride(0), P(a["ones"]), P(a["cshift"]), -math.inf, math.inf,
                                 y.shape[0], x.shape[1], t, 0, P(a["index"]), P(a["key"]), P(a["ws"]), a["ws"].numel(), s)
    return FarCase(_case("mmk_nn_topk_f32"), _rows("x", "y"), call, ("x_row_stride", "y_row_stride"))


def _half_neg_sqnorm():
    def call(L, a, s):
        y = a["y"]
        return L.mmk_half_neg_sqnorm_f32(P(y), y.stride(0), y.shape[0], y.shape[1], P(a["out"]), s)
    return FarCase(_case("mmk_half_neg_sqnorm_f32"), _rows("y"), call, ("y_row_stride",))


def _novelty():
    halves = S.NOVELTY_HALVES

    def call(L, a, s):
        x = a["x"]
        h = (C.c_int32 * len(halves))(*halves)
        return L.mmk_novelty_f32(P(x), x.stride(0), x.stride(1), None, x.shape[0], x.shape[1], x.shape[2], h, len(halves), P(a["raw"]), s)
    return FarCase(_case("mmk_novelty_f32"), _two("x"), call, ("x_batch_stride", "x_row_stride"), stack=("x", "raw"), bound=_bound_novelty)


def _pca_colstats():
    def call(L, a, s):
        x = a["x"]
        return L.mmk_pca_colstats_f64(P(x), x.stride(0), x.shape[0], x.shape[1], P(a["mean"]), P(a["scale"]), P(a["ws"]), a["ws"].numel(), s)
    return FarCase(_case("mmk_pca_colstats_f64"), _rows("x"), call, ("x_row_stride",), bound=_bound_pca_colstats)


def _pca_cov():
    def call(L, a, s):
        x = a["x"]
        return L.mmk_pca_cov_f64(P(x), x.stride(0), x.shape[0], x.shape[1], P(a["mean"]), P(a["scale"]), P(a["c"]), P(a["ws"]), a["ws"].numel(), s)
    return FarCase(_case("mmk_pca_cov_f64"), _rows("x"), call, ("x_row_stride",))


def _pca_project():
    def call(L, a, s):
        y, out = a["y"], a["out"]
        return L.mmk_pca_project_f32(P(y), y.stride(0), y.shape[0], y.shape[1], P(a["mean"]), P(a["scale"]), P(a["components"]), out.shape[1], P(out),
                                     out.stride(0), s)
    return FarCase(_case("mmk_pca_project_f32"), _rows("y", "out"), call, ("y_row_stride", "out_row_stride"))


def _stft(stem, n_fft):
    hop, bins = n_fft // 4, n_fft // 2 + 1

    def call(L, a, s):
        x = a["x"]
        head = (P(x), x.stride(0), x.shape[0], x.shape[1], n_fft, hop, 0)
        if stem == "mmk_stft_mag_f32":
            return L.mmk_stft_mag_f32(*head, P(a["out"]), s)
        if stem == "mmk_stft_f32":
            return L.mmk_stft_f32(*head, 0, 0, P(a["out"]), s)
        if stem == "mmk_stft_energy_f32":
            return L.mmk_stft_energy_f32(*head, 0, P(a["out"]), s)
        host = S._band_host(S._bank()[0])
        return L.mmk_stft_mel_f32(*head, 0, bins, S.MEL_BANDS, host, P(a["band"]), P(a["weights"]), 5 * S.MEL_BANDS, None, 0, P(a["out"]), s)
    bound = {"mmk_stft_mag_f32": _bound_stft("mag", n_fft), "mmk_stft_f32": _bound_stft("car", n_fft),
             "mmk_stft_energy_f32": _bound_stft_energy(n_fft)}.get(stem)
    return FarCase(_case(f"{stem}[{n_fft}]"), _rows("x"), call, ("x_row_stride",), bound=bound)


def _interp1d():
    def call(L, a, s):
        x, y = a["x"], a["y"]
        return L.mmk_interp1d_f32(P(x), x.stride(0), x.shape[0], x.shape[1], P(y), y.stride(0), y.shape[1], 0, 1, s)
    return FarCase(_case("mmk_interp1d_f32"), _rows("x", "y"), call, ("x_row_stride", "y_row_stride"), bound=_bound_interp1d)


def _derivative():
    def call(L, a, s):
        x, y = a["x"], a["y"]
        return L.mmk_derivative_f32(P(x), x.stride(0), x.shape[0], x.shape[1], 3, P(y), y.stride(0), s)
    return FarCase(_case("mmk_derivative_f32"), _rows("x", "y"), call, ("x_row_stride", "y_row_stride"), bound=_bound_derivative)


def _hpss(clips):
    """the header ties out_batch_stride to (frames - 1) * out_row_stride + bins or more: with far rows a second clip would lie beyond the
    field, so the row strides are far with one clip and the batch strides with two"""
    names = ("harmonic", "percussive", "harm_median", "perc_median")

    def call(L, a, s):
        x, o = a["s"], a[names[0]]
        assert all(a[k].stride() == o.stride() for k in names)          # (one pair of output strides for the four)
        return L.mmk_hpss_f32(P(x), x.stride(0), x.stride(1), x.shape[0], x.shape[1], x.shape[2], 31, 31, 1.0, 1.0, 1.0, *[P(a[k]) for k in names],
                              o.stride(0), o.stride(1), s)
    if clips == 1:
        return FarCase(_case("mmk_hpss_f32"), _two("s", *names), call, ("s_row_stride", "out_row_stride"), bound=_bound_hpss)
    return FarCase(_case("mmk_hpss_f32"), _two("s", *names), call, ("s_batch_stride", "out_batch_stride"), stack=("s",) + names, tag="mmk_hpss_f32[2 clips]",
                   axes=["batch"], bound=_bound_hpss)


def _melbank():
    def call(L, a, s):
        x = a["s"]
        host = S._band_host(S._bank()[0])
        return L.mmk_melbank_f32(P(x), x.stride(0), x.shape[0], x.shape[1], x.shape[1], S.MEL_BANDS, host, P(a["band"]), P(a["weights"]), 5 * S.MEL_BANDS,
                                 None, 0, P(a["out"]), s)
    return FarCase(_case("mmk_melbank_f32"), _rows("s"), call, ("in_row_stride",), bound=_bound_melbank)


def _pack_weight():
    def call(L, a, s):
        w = a["w"]
        return L.mmk_pack_weight_f32(P(w), w.stride(0), w.shape[0], w.shape[1], P(a["packed"]), s)
    return FarCase(_case("mmk_pack_weight_f32"), _rows("w"), call, ("ldw",))


def _gemm_terms(x, w, bias, act):
    """-> (want64, bound) of act(x @ w^T + bias), tests/f64_bounds.py: gemm_bound"""
    x64, w64, b64 = x.double(), w.double(), None if bias is None else bias.double()
    pre = x64 @ w64.t() + (0 if b64 is None else b64)
    want = B.ACT_F[act](pre)
    return want, B.gemm_bound(x64, w64, b64, x.shape[-1], act, want)


def _linear():
    def call(L, a, s):
        x, y = a["x"], a["y"]
        return L.mmk_linear_f32(P(x), x.stride(0), x.shape[0], P(a["packed"]), P(a["bias"]), y.shape[1], x.shape[1], P(y), y.stride(0), 1, s)
    return FarCase(_case("mmk_linear_f32"), _rows("x", "y"), call, ("ldx", "ldy"), bound=lambda i: dict(y=_gemm_terms(i["x"], i["w"], i["bias"], 1)))


def _gemm():
    def call(L, a, s):
        x, c = a["a"], a["c"]
        return L.mmk_gemm_f32(P(x), x.stride(1), x.stride(0), P(a["packed"]), c.shape[2], x.shape[2], P(c), c.stride(1), c.stride(0), x.shape[1],
                              x.shape[0], s)
    return FarCase(_case("mmk_gemm_f32"), _two("a", "c"), call, ("lda", "a_batch", "ldc", "c_batch"), odd="refused",
                   bound=lambda i: dict(c=_gemm_terms(i["a"], i["w"], None, 0)))


def _gemm_bias_act():
    def call(L, a, s):
        x, c = a["a"], a["c"]
        return L.mmk_gemm_bias_act_f32(P(x), x.stride(0), x.shape[0], P(a["packed"]), P(a["bias"]), c.shape[1], x.shape[1], P(c), c.stride(0), 1, 0, 0, 0,
                                       0, P(a["partial"]), a["partial"].numel() // 4, S.GEMM_K_SPLIT, s)
    return FarCase(_case("mmk_gemm_bias_act_f32"), _rows("a", "c"), call, ("lda", "ldc"), odd="refused",
                   bound=lambda i: dict(c=_gemm_terms(i["a"], i["w"], i["bias"], 1)))


GEMM_GROUP = 10                 # the row map of mmk_gemm_bias_act_f32: 130 rows as 13 groups of 10, all of them kept


def _gemm_row_map():
    def call(L, a, s):
        x, c = a["a"], a["c"]
        assert c.shape[1] == GEMM_GROUP
        return L.mmk_gemm_bias_act_f32(P(x), x.stride(0), x.shape[0], P(a["packed"]), P(a["bias"]), c.shape[2], x.shape[1], P(c), 0, 1, GEMM_GROUP, GEMM_GROUP,
                                       c.stride(0), c.stride(1), P(a["partial"]), a["partial"].numel() // 4, S.GEMM_K_SPLIT, s)

    def bound(i):
        want, bnd = _gemm_terms(i["a"], i["w"], i["bias"], 1)
        return dict(c=(want.reshape(-1, GEMM_GROUP, want.shape[1]), bnd.reshape(-1, GEMM_GROUP, want.shape[1])))
    case = _case("mmk_gemm_bias_act_f32")
    m, n = case.build(0)["a"].shape[0], case.build(0)["w"].shape[0]
    assert m % GEMM_GROUP == 0
    return FarCase(case, {"a": 1, "c": 2}, call, ("group_stride", "row_stride"), odd="refused", bound=bound, tag="mmk_gemm_bias_act_f32[row map]",
                   reshape=dict(c=(m // GEMM_GROUP, GEMM_GROUP, n)))


def _skinny_linear():
    def call(L, a, s):
        x, c = a["a"], a["c"]
        return L.mmk_skinny_linear_f32(P(x), x.stride(0), x.shape[0], P(a["packed"]), P(a["bias"]), c.shape[1], x.shape[1], P(c), c.stride(0), 3, s)
    return FarCase(_case("mmk_skinny_linear_f32"), _rows("a", "c"), call, ("lda", "ldc"), odd="refused",
                   bound=lambda i: dict(c=_gemm_terms(i["a"], i["w"], i["bias"], 3)))


ATT_HEADS, ATT_HD = 2, 8


def _tr_attention():
    def call(L, a, s):
        q, k, v, o = a["q"], a["k"], a["v"], a["out"]
        assert k.stride() == v.stride()
        n_q, n_keys = q.shape[1], k.shape[1]
        return L.mmk_tr_attention_f32(P(q), q.stride(1), q.stride(0), P(k), P(v), k.stride(1), k.stride(0), P(o), o.stride(1), o.stride(0), n_q,
                                      n_keys - n_q, n_keys, ATT_HEADS, ATT_HD, 1.0 / math.sqrt(ATT_HD), q.shape[0], s)

    def bound(i):
        q, k, v = (i[n].double().reshape(i[n].shape[0], -1, ATT_HEADS, ATT_HD) for n in "qkv")
        scale, pos0 = 1.0 / math.sqrt(ATT_HD), k.shape[1] - q.shape[1]
        want, wts, x, vis = B.attention_ref(q, k, v, pos0, scale)
        return dict(out=(want.reshape(i["q"].shape), B.attention_bound(q, k, v, want, wts, x, vis, scale).reshape(i["q"].shape)))
    return FarCase(_case("mmk_tr_attention_f32"), _two("q", "k", "v", "out"), call, ("q_ld", "q_cs", "kv_ld", "kv_cs", "o_ld", "o_cs"), bound=bound)


def _tr_add_ln():
    def call(L, a, s):
        y, res, out = a["y"], a["res"], a["out"]
        return L.mmk_tr_add_ln_f32(P(y), y.stride(0), P(res), res.stride(0), P(a["w"]), P(a["b"]), P(out), out.stride(0), y.shape[0], y.shape[1], s)

    def bound(i):
        v, w64, b64 = i["y"].double() + i["res"].double(), i["w"].double(), i["b"].double()
        want, mean, d, var, rstd = B.ln_ref(v, w64, b64)
        return dict(out=(want, B.ln_bound(v, w64, True, want, mean, d, var, rstd)))
    return FarCase(_case("mmk_tr_add_ln_f32"), _rows("y", "res", "out"), call, ("y_ld", "res_ld", "out_ld"), bound=bound)


def _categorical_sample():
    def call(L, a, s):
        logits, out = a["logits"], a["out"]
        return L.mmk_categorical_sample_f32_i64(P(logits), logits.stride(0), logits.shape[0], logits.shape[1] - 1, 1, 0.9, P(a["temperature"]),
                                                P(a["uniforms"]), P(out), out.stride(0), s)
    return FarCase(_case("mmk_categorical_sample_f32_i64"), _rows("logits", "out"), call, ("ld", "out_stride"))


def _small_header_cases():
    """the STREAM_CASES of the four small headers' GPU tests (their modules import without a GPU)"""
    from tests import test_gpu_kmeans as TK, test_gpu_nmf as TN, test_gpu_nn_filter as TF, test_gpu_samplify as TS
    by = {c.id: c for c in TK.STREAM_CASES + TN.STREAM_CASES + TF.STREAM_CASES + TS.STREAM_CASES}

    def assign(L, a, s):
        x, c = a["x"], a["centres"]
        return L.mmk_kmeans_assign_f32(P(x), x.stride(0), P(a["offset"]), x.shape[0], x.shape[1], P(c), c.stride(0), P(a["shift"]), c.shape[0],
                                       P(a["labels"]), P(a["key"]), P(a["changed"]), s)

    def label_sums(L, a, s):
        x, c = a["x"], a["centres"]
        return L.mmk_kmeans_label_sums_f64(P(x), x.stride(0), P(a["offset"]), x.shape[0], x.shape[1], P(a["labels"]), c.shape[0], P(a["sums"]),
                                           P(a["counts"]), P(c), c.stride(0), P(a["row_d2"]), P(a["inertia"]), P(a["ws"]), a["ws"].numel(), s)

    def pp_step(L, a, s):
        x = a["x"]
        return L.mmk_kmeans_pp_step_f64(P(x), x.stride(0), P(a["offset"]), x.shape[0], x.shape[1], P(a["cand"]), a["cand"].numel(), P(a["closest"]),
                                        P(a["pot"]), P(a["chosen"]), P(a["ws"]), a["ws"].numel(), s)

    def nmf_fit(L, a, s):
        from tests import nmf_refs as NR
        f = NR.FIXTURES["tiny"]
        x, k, it = a["x"], a["w"].shape[1], C.c_int32(0)
        n, d = x.shape
        rc = L.mmk_nmf_start_f64(P(x), x.stride(0), n, d, k, P(a["w"]), P(a["ht"]), P(a["s"]), P(a["v"]), P(a["part"]), P(a["start"]), a["start"].numel(), s)
        return rc or L.mmk_nmf_solve_f64(P(x), x.stride(0), n, d, k, P(a["w"]), P(a["ht"]), 1, f["tol"], f["max_iter"], 0, 1, C.byref(it), P(a["solve"]),
                                         a["solve"].numel(), s)

    def nmf_half(which):
        from tests import nmf_refs as NR
        f = NR.FIXTURES["tiny"]
        n, d, k = f["n"], f["d"], f["k"]

        def build(seed):
            g = S.gen(seed + 40)
            return dict(x=torch.from_numpy(TN._tiny(seed)), w=S.uni(g, n, k, lo=0.0).double(), ht=S.uni(g, d, k, lo=0.0).double())

        def call(L, a, s):      # (the factor is updated in place: the dense input, which every run puts in place again, is copied out)
            x, (fixed, moved) = a["x"], (("ht", "w") if which == "w" else ("w", "ht"))
            rc = getattr(L, f"mmk_nmf_{which}_half_f64")(P(x), x.stride(0), n, d, k, P(a[fixed]), P(a[moved]), P(a["violation"]), P(a["ws"]), a["ws"].numel(), s)
            a["factor"].copy_(a[moved])
            return rc
        case = S.Case(f"mmk_nmf_{which}_half_f64", build, lambda L, i: dict(violation=((1,), torch.float64), factor=((n if which == "w" else d, k), torch.float64)),
                      call, work=lambda L, i: dict(ws=L.mmk_nmf_half_workspace_bytes(n, d, k)))
        return FarCase(case, _rows("x"), call, ("x_row_stride",))

    def aggregate(L, a, s):
        x, out = a["x"], a["out"]
        return L.mmk_nn_aggregate_f32(P(x), x.stride(0), x.shape[0], x.shape[1], P(a["index"]), a["index"].shape[1], 0, 0, P(out), out.stride(0),
                                      P(a["count"]), s)

    def coef(L, a, s):
        x, c = a["x"], a["coef"]
        return L.mmk_spline2_coef_f64(P(x), x.stride(0), x.shape[0], x.shape[1], P(c), c.stride(0), s)

    def evaluate(L, a, s):
        c, out = a["coef"], a["out"]
        return L.mmk_spline2_eval_f32(P(c), c.stride(0), c.shape[0], c.shape[1], P(out), out.stride(0), out.shape[1], s)

    return [FarCase(by["mmk_kmeans_assign_f32"], _rows("x", "centres"), assign, ("x_row_stride", "c_row_stride")),
            FarCase(by["mmk_kmeans_label_sums_f64"], _rows("x", "centres"), label_sums, ("x_row_stride", "c_row_stride"), bound=_bound_kmeans_sums),
            FarCase(by["mmk_kmeans_pp_step_f64"], _rows("x"), pp_step, ("x_row_stride",)),
            FarCase(by["mmk_nmf_solve_f64[fit]"], _rows("x"), nmf_fit, ("mmk_nmf_start_f64.x_row_stride", "mmk_nmf_solve_f64.x_row_stride")),
            nmf_half("w"), nmf_half("h"),
            FarCase(by["mmk_nn_aggregate_f32"], _rows("x", "out"), aggregate, ("x_row_stride", "out_row_stride"), bound=_bound_nn_aggregate),
            FarCase(by["mmk_spline2_coef_f64"], _rows("x", "coef"), coef, ("y_row_stride", "coef_row_stride")),
            FarCase(by["mmk_spline2_eval_f32"], _rows("coef", "out"), evaluate, ("coef_row_stride", "out_row_stride"))]


_STFT_STEMS = ("mmk_stft_mag_f32", "mmk_stft_f32", "mmk_stft_energy_f32", "mmk_stft_mel_f32")
FAR_CASES = [_resample(), _lfilter1(), _row_normalize(), _inv_row_norm(), _cosine_cost(), _nn_cosine(), _cum_entropy(), _nn_cosine_self(), _segment_mean(),
             _nn_topk(), _half_neg_sqnorm(), _novelty(), _pca_colstats(), _pca_cov(), _pca_project(),
             *[_stft(stem, n) for stem in _STFT_STEMS for n in S.SPECTRAL_N_FFT], _interp1d(), _derivative(), _hpss(1), _hpss(2), _melbank(), _pack_weight(),
             _linear(), _gemm(), _gemm_bias_act(), _gemm_row_map(), _skinny_linear(), _tr_attention(), _tr_add_ln(), _categorical_sample(), *_small_header_cases()]
FAR_BY_ID = {c.id: c for c in FAR_CASES}
assert len(FAR_BY_ID) == len(FAR_CASES)

# ---- the plans (tests/test_gpu_far_offsets.py: test_plan_with_far_strides): one smallest case per network and entry point of
# stream_cases.PLAN_CASES' kind, every one with two clips or more; the operands are the loop's tensor (`data`), the conditioning inputs
# and the step's output, {operand: levels} per network
PLAN_TEST = "test_plan_with_far_strides"
PLAN_CASES = [S.PlanCase("wavenet", "chain-cond"),                                        # in0 and the conditioning rows; warm-up, a short block
              S.PlanCase("wavenet", "launches", n=2 * S.GRAPH_STEPS + 3, graph=True),     # a block above the graph threshold
              S.PlanCase("wavenet", "chain", sampled=True),
              S.PlanCase("wavenet", "spipe-5"),                                           # the stage pipeline: its own logits copy-out
              S.PlanCase("srnn", "launches"), S.PlanCase("srnn", "bottom-four_clips-321"), S.PlanCase("srnn", "bottom-one_clip", sampled=True),
              S.PlanCase("s2s", "resident-128-2-3"), S.PlanCase("s2s", "classes"),
              S.PlanCase("tr", "one_layer_rf9"), S.PlanCase("tr", "one_layer_rf9", sampled=True), S.PlanCase("tr", "frames130_rf2")]
# (mmk_tr_generate refuses a class tensor whose time stride is not 1: the classes' clips are far apart, the frames' clips and positions)
PLAN_OPS = {"wavenet": dict(data=1, cond=1, logits=1), "srnn": dict(data=1, logits=1), "s2s": dict(data=2, step_y=2, logits=1),
            "tr": dict(data=1, step_y=1, logits=1), "tr frames": dict(data=2, step_y=1)}


def plan_ops(pc):
    return PLAN_OPS["tr frames" if pc.network == "tr" and S.plan_ref(pc).inputs().dim() == 3 else pc.network]


def plan_steps(pc):
    """the steps of a plan case's block, as test_gpu_streams.PlanRun counts them"""
    ref = S.plan_ref(pc)
    hop = 1 if pc.network == "tr" else (ref.hop or 1)
    resident = pc.network == "srnn" and pc.ref.startswith("resident")
    return pc.n or (ref.parts[0] if resident else 2 * hop if pc.network == "s2s" else S.SHORT_BLOCK)


# The logits' column count is the plan's (classes + a learned temperature, rounded by no one): known on the device only.  The no-GPU layout
# test places the rows with this stand-in; the GPU test builds its layouts with the plan's own count and checks that placement itself
# (problems(), and build_layout raises where it finds none)
LOGIT_COLS = 257


def plan_tensors(pc, logit_cols=LOGIT_COLS):
    """{operand: (shape, dtype)} of a plan case's strided operands: the loop's tensor, the conditioning inputs, the step's output and,
    for a network of classes, the rows that last_logits copies out"""
    ref = S.plan_ref(pc)
    if pc.network == "tr":
        prompt, conds, P, hop = ref.inputs(), (), ref.prompt, 1
    else:
        (prompt, conds), P, hop = ref.inputs(), ref.P, ref.hop or 1
    B, T = prompt.shape[0], P + plan_steps(pc)
    out = dict(data=((B, T) + tuple(prompt.shape[2:]), prompt.dtype))
    for j, c in enumerate(conds):
        out[f"cond{j}"] = (tuple(c.shape), c.dtype)
    if pc.network == "s2s":
        out["step_y"] = ((B, hop) + tuple(prompt.shape[2:]), prompt.dtype)
    elif pc.network == "tr":
        out["step_y"] = ((B,) + tuple(prompt.shape[2:]), prompt.dtype)          # the next class of a clip, or its next frame
    if prompt.dtype == torch.int64:
        out["logits"] = ((B * hop if pc.network == "s2s" else B, logit_cols), torch.float32)
    return out


def plan_layouts(pc, logit_cols=LOGIT_COLS):
    ops, specs = plan_ops(pc), []
    for name, (shape, dtype) in plan_tensors(pc, logit_cols).items():
        levels = ops["cond" if name.startswith("cond") else name]
        ew = torch.empty((), dtype=dtype).element_size() // WORD
        if levels == 2:
            specs.append((name, ew, 2, shape[0], shape[1], math.prod(shape[2:])))
        else:
            specs.append((name, ew, 1, 1, shape[0], math.prod(shape[1:])))
    axes = ["rows"] + (["batch"] if 2 in ops.values() else [])
    return [build_layout(specs, axis, mark, cls) for axis in axes for mark in ("far", "mid") for cls in (0, 1)]


# ---- the Seq2Seq plan (tests/test_gpu_far_offsets.py: test_s2s_frames_below_and_beyond_the_input_projection_limit): the config of net_refs for which the first encoder layer's
# input projection reads the caller's frames in place, and the three spans of csrc/s2s_plan.hip's switch to gather_frames_kernel
S2S_SPAN_LIMIT = 2 ** 31        # bytes (csrc/s2s_plan.hip: fm.floats * sizeof(float) >= 1 << 31 -> gather_frames_kernel)


def s2s_batch_stride(which, batch, hop, in_dim, frame_stride):
    """the clip stride (floats, a multiple of 4) that makes the frames' span - (batch - 1) clip strides, hop - 1 frame strides and one frame,
    as the plan computes it - the largest below 2^31 bytes ('below'), the smallest at or above it ('above'), or more than 2^32 bytes
    ('beyond')"""
    rest = (hop - 1) * frame_stride + in_dim
    limit = {"below": S2S_SPAN_LIMIT // WORD - 1, "above": S2S_SPAN_LIMIT // WORD + 3 * (batch - 1), "beyond": 2 ** 30 + SKEW}[which]
    return (limit - rest) // (batch - 1) // 4 * 4 if which == "below" else roundup(-(-(limit - rest) // (batch - 1)), 4)


def s2s_span_bytes(batch, hop, in_dim, batch_stride, frame_stride):
    return ((batch - 1) * batch_stride + (hop - 1) * frame_stride + in_dim) * WORD


_PROFILE = ("a measurement aid of bench.py that no test runs (stream_cases.NOT_RUN); it fills the same call record as mmk_wavenet_generate "
            "(csrc/wavenet_plan.hip: check_call, in0_rs, cond_rs), which the plan test drives")
NOT_FAR = {
    "mmk_wavenet_profile_steps.in0_row_stride": _PROFILE,
    "mmk_wavenet_profile_steps.cond_row_stride": _PROFILE,
}
PLAN_PARAMS = (
    [f"mmk_wavenet_{f}.{p}" for f in ("warmup", "generate") for p in ("in0_row_stride", "cond_row_stride")]
    + [f"mmk_srnn_{f}.idx_row_stride" for f in ("warmup", "generate", "warmup_multi", "generate_multi")]
    + [f"mmk_s2s_step.{p}" for p in ("x_batch_stride", "x_frame_stride", "y_batch_stride", "y_frame_stride")]
    + [f"mmk_s2s_generate.{p}" for p in ("batch_stride", "frame_stride")]
    + [f"mmk_s2s_step_classes.{p}" for p in ("x_batch_stride", "x_elem_stride", "y_batch_stride", "y_elem_stride")]
    + [f"mmk_s2s_generate_classes.{p}" for p in ("batch_stride", "elem_stride")]
    + [f"mmk_tr_step.{p}" for p in ("x_batch_stride", "x_time_stride", "y_batch_stride")]
    + [f"mmk_tr_generate.{p}" for p in ("batch_stride", "time_stride")]
    + [f"mmk_{f}.ld" for f in ("wavenet_last_logits", "wavenet_last_logits_of", "srnn_last_logits", "srnn_last_logits_of")]
    + ["mmk_s2s_last_logits.out_ld", "mmk_tr_last_logits.out_ld"])
FAR = {p: c.id for c in FAR_CASES for p in c.params}
FAR.update({p: PLAN_TEST for p in PLAN_PARAMS})
FAR_PARAMS = {**{p: ("FAR", c) for p, c in FAR.items()}, **{p: ("NOT_FAR", r) for p, r in NOT_FAR.items()}}
