"""Placed operands and the surround rule, shared by the family tests (tests/test_gpu_*.py) and tests/test_strided_inputs.py (no GPU).

A Strided is one (rows, k) or (batch, rows, k) operand as a misaligned, strided view inside a longer buffer of the test's own: row stride
k + PAD, batch stride rows * row stride + GAP, first element `offset` in, TAIL elements behind the last row - the layout every family file
used to build with a local Rows / Clips class.  Everything outside the view is the SURROUND.  An output or a workspace is surrounded by NaN
and held to f64_bounds.check_written, as before; an INPUT (Strided.of) is surrounded by one of

  ZERO   zeros: the baseline, and the one value that hides an over-read (neutral for a sum, a dot product, a norm, an |x| maximum, and what
         several kernels produce at an edge anyway);
  NAN    NAN_BITS in every word, as tensor.fill_(nan) writes it: any arithmetic use shows, a product with a zero weight included;
  HUGE   the largest finite value of the type with the sign alternating from element to element: it wins every >, <, min, max and median on
         either side - the comparisons that drop a NaN silently - and turns a sum into inf.

An integer input has no NaN: under NAN and HUGE (and DECOY, for a call with integer inputs only) its surround is DECOYS, valid values of the
case - an index below n, a label below k, a class below q_levels - that differ from the in-view element next to them, so that a kernel which
uses one gives a wrong answer and never an illegal address.  For offsets (MONOTONE) the decoys are the first value in front and the last
behind: valid and monotone.

THE RULE (surround_rule): a call helper that places its inputs with Strided.of is run once per surround, every other argument the same; every
result of the NAN and of the HUGE run is bit for bit the result of the ZERO run, and every placed input is untouched(), surround included.
The helper's caller sees the ZERO run's results, on which the family's float64 bound is checked as before.  The rule needs no reference and
no tolerance: the kernels are deterministic (the suite's "two calls, the same bits"), layout and alignment are the same in the three runs,
so a difference is a read outside the view.

SURROUND_PARAMS, at the end: every stride parameter of the five headers (far_cases.header_stride_params) under the GPU test that runs it
under the rule, or under the reason why none does.
"""
import functools

import numpy as np
import torch

PAD, GAP, TAIL = 7, 11, 5
ZERO, NAN, HUGE, DECOY = "zero", "nan", "huge", "decoy"
FLOAT_SURROUNDS = (ZERO, NAN, HUGE)
INT_SURROUNDS = (ZERO, DECOY)
NAN_BITS = 0x7FC00000           # what tensor.fill_(nan) writes
MONOTONE = "monotone"

_RUN = None                     # the surround_rule run in progress: [surround, [the inputs placed so far]]


def pattern(surround, numel, dtype, decoy=None):
    """the surround as a flat numpy array of `numel` elements: what a buffer holds before its view is copied in"""
    dtype = np.dtype(dtype)
    if surround == ZERO:
        return np.zeros(numel, dtype)
    if dtype.kind == "f":
        if surround == NAN:
            assert dtype == np.float32 or dtype == np.float64
            return np.full(numel, np.nan, dtype)
        assert surround == HUGE, surround
        big = np.full(numel, np.finfo(dtype).max, dtype)
        big[1::2] *= -1
        return big
    assert dtype.kind == "i" and decoy is not None and decoy != MONOTONE, (surround, dtype, decoy)
    lo, hi = decoy
    assert lo < hi
    return (lo + (np.arange(numel, dtype=np.int64) * 7 + 3) % (hi - lo)).astype(dtype)


class Strided:
    """shape (rows, k) or (batch, rows, k); strides in elements; `fill`: a number (outputs: NaN) or the flat numpy array the buffer starts from"""

    def __init__(self, shape, offset, device, fill, dtype=torch.float32, row_stride=None, batch_stride=None, tail=TAIL):
        self.shape, self.offset = tuple(int(s) for s in shape), int(offset)
        assert len(self.shape) in (2, 3) and offset >= 0
        self.rows, self.k = self.shape[-2:]
        self.stride = self.k + PAD if row_stride is None else int(row_stride)                              # the row stride
        assert self.stride >= self.k
        self.strides = (self.stride, 1)
        if len(self.shape) == 3:
            self.clip = self.rows * self.stride + GAP if batch_stride is None else int(batch_stride)      # the batch stride
            assert self.clip >= (self.rows - 1) * self.stride + self.k
            self.strides = (self.clip,) + self.strides
        self.numel = self.offset + self.shape[0] * self.strides[0] + tail
        if isinstance(fill, np.ndarray):
            assert fill.shape == (self.numel,)
            self.buf = torch.from_numpy(fill).to(device)
        else:
            self.buf = torch.full((self.numel,), fill, dtype=dtype, device=device)
        self.view = self.buf.as_strided(self.shape, self.strides, self.offset)
        self.before = None

    @classmethod
    def of(cls, x_np, offset, device, row_stride=None, batch_stride=None, tail=TAIL, decoy=None, surround=None):
        """an INPUT: `x_np` placed under the current run's surround (ZERO outside a surround_rule run); decoy: (lo, hi) or MONOTONE for an
        integer array.  The buffer is built on the host and copied once; untouched() compares with that copy."""
        x_np = np.asarray(x_np)
        surround = surround or (_RUN[0] if _RUN else ZERO)
        probe = cls(x_np.shape, offset, "cpu", 0, torch.from_numpy(x_np.ravel()[:1].copy()).dtype, row_stride, batch_stride, tail)
        integer = x_np.dtype.kind == "i"
        if integer and surround != ZERO:
            host = decoys(x_np, probe, decoy)
        else:
            host = pattern(surround, probe.numel, x_np.dtype)
            _view(host, probe)[...] = x_np
        s = cls(x_np.shape, offset, device, host, None, row_stride, batch_stride, tail)
        s.surround = DECOY if integer and surround != ZERO else surround
        s.before = s.buf.clone()
        if _RUN:
            _RUN[1].append(s)
        return s

    @property
    def ptr(self):
        return self.buf.data_ptr() + self.buf.element_size() * self.offset

    def mask(self):
        """True on the view's elements, on the host"""
        m = torch.zeros(self.buf.shape, dtype=torch.bool)
        m.as_strided(self.shape, self.strides, self.offset).fill_(True)
        return m

    def untouched(self):
        """the whole buffer, surround included, holds the bits it was placed with"""
        return self.before is not None and torch.equal(_ints(self.buf), _ints(self.before))


def _ints(t):
    return t.view({1: torch.int8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])


def _view(host, s):
    return np.lib.stride_tricks.as_strided(host[s.offset:], s.shape, tuple(st * host.itemsize for st in s.strides))


def decoys(x_np, s, decoy):
    """the host buffer of an integer input: valid values everywhere outside the view, none equal to the in-view element beside it"""
    inside = s.mask().numpy()
    if decoy == MONOTONE:
        flat = x_np.ravel()
        assert s.stride == s.k and len(s.shape) == 2 and (np.diff(flat) >= 0).all()
        host = np.concatenate([np.full(s.offset, flat[0]), flat, np.full(s.numel - s.offset - flat.size, flat[-1])]).astype(x_np.dtype)
        return host
    lo, hi = decoy
    host = pattern(DECOY, s.numel, x_np.dtype, decoy)
    _view(host, s)[...] = x_np
    near = np.zeros_like(inside)
    near[1:] |= inside[:-1]
    near[:-1] |= inside[1:]
    for at in np.nonzero(near & ~inside)[0]:
        beside = [host[j] for j in (at - 1, at + 1) if 0 <= j < s.numel and inside[j]]
        free = [v for v in range(lo, min(hi, lo + 3)) if v not in beside]
        if host[at] in beside and free:                                  # (a range of one value, or of two with both beside it, has none)
            host[at] = free[0]
    return host


# ====================================================================================================================== the rule
def bits_of(v):
    """a result of a call helper as something == compares bit for bit: tensors, arrays, placed outputs (their whole buffer), numbers, None,
    and tuples, lists and dicts of them"""
    if isinstance(v, Strided):
        return ("placed", bits_of(v.buf))
    if torch.is_tensor(v):
        v = v.detach().cpu().contiguous()
        return ("tensor", str(v.dtype), tuple(v.shape), _ints(v).numpy().tobytes())
    if isinstance(v, np.ndarray):
        return ("array", str(v.dtype), v.shape, np.ascontiguousarray(v).tobytes())
    if isinstance(v, (tuple, list)):
        return tuple(bits_of(e) for e in v)
    if isinstance(v, dict):
        return tuple((k, bits_of(e)) for k, e in sorted(v.items()))
    if isinstance(v, (float, np.floating)):
        return ("float", np.float64(v).tobytes())
    assert v is None or isinstance(v, (int, bool, str, np.integer)), type(v)
    return v if v is None or isinstance(v, str) else int(v)


def differing(a, b, path="result"):
    """where two bits_of values differ, for the message"""
    if type(a) is tuple and type(b) is tuple and len(a) == len(b) and a[:1] not in (("tensor",), ("array",), ("float",)):
        for i, (x, y) in enumerate(zip(a, b)):
            if x != y:
                return differing(x, y, f"{path}[{i}]")
    if type(a) is tuple and a[:1] in (("tensor",), ("array",)) and type(b) is tuple and a[:3] == b[:3]:
        x, y = np.frombuffer(a[3], np.uint8), np.frombuffer(b[3], np.uint8)
        item = max(1, x.size // max(1, int(np.prod(a[2]))))
        return f"{path} {a[1]}{a[2]}: {int((x != y).reshape(-1, item).any(-1).sum())} elements differ, first at flat index {int(np.nonzero(x != y)[0][0]) // item}"
    return f"{path}: {str(a)[:60]} against {str(b)[:60]}"


def surround_rule(*surrounds, may_place_nothing=False):
    """decorator of a call helper whose inputs are placed with Strided.of: THE RULE of the module docstring.  -> the ZERO run's results.
    may_place_nothing: a helper that has cases without any input (an empty list passed as a NULL pointer)"""
    assert surrounds and surrounds[0] == ZERO

    def wrap(call):
        @functools.wraps(call)
        def run(*args, **kwargs):
            global _RUN
            assert _RUN is None, "a call helper under the rule calls another one: place the inputs in one of them"
            base = want = None
            for surround in surrounds:
                _RUN = [surround, []]
                try:
                    got = call(*args, **kwargs)
                    placed = _RUN[1]
                finally:
                    _RUN = None
                assert placed or may_place_nothing, f"{call.__name__} places no input with Strided.of"
                for i, p in enumerate(placed):
                    assert p.untouched(), f"{call.__name__} under {surround}: input {i} {p.shape}, or its surround, was written"
                if surround == ZERO:
                    base, want = got, bits_of(got)
                else:
                    have = bits_of(got)
                    assert have == want, (f"{call.__name__} under {surround}: {differing(want, have)} - a read outside a view of "
                                          f"{[p.shape for p in placed]}")
            return base
        return run
    return wrap


# ====================================================================================================================== the table
# 'function.parameter' of every stride parameter of the five headers -> the GPU test ('file::test') that runs the operand under the rule,
# or the reason why none does.  tests/test_strided_inputs.py holds the table to the headers in both directions.
OUTPUT = "output stride"
PLAN = "plan entry, see below"
F64_KERNELS = "covered NaN-padded by test_gpu_kernels_f64"
F64_SPECTRAL = "covered NaN-padded by test_gpu_spectral_f64"

_NNN = "test_gpu_nnn.py::test_cost_kernel_within_the_bound_of_float64"
_SPLINE = "test_gpu_samplify.py::test_spline_entry_points_write_their_outputs_only"
UNDER_RULE = {
    "mmk_categorical_sample_f32_i64.ld": "test_gpu_pickers.py::test_sample_kernel_on_crafted_rows",
    "mmk_cosine_cost_f32.x_batch_stride": _NNN, "mmk_cosine_cost_f32.x_row_stride": _NNN, "mmk_cosine_cost_f32.y_row_stride": _NNN,
    "mmk_inv_row_norm_f32.x_batch_stride": _NNN, "mmk_inv_row_norm_f32.x_row_stride": _NNN,
    "mmk_cum_entropy_i64.row_stride": "test_gpu_neighbors.py::test_cum_entropy_against_the_bound",
    "mmk_derivative_f32.x_row_stride": "test_gpu_envelope.py::test_derivative_against_the_bound",
    "mmk_interp1d_f32.x_row_stride": "test_gpu_envelope.py::test_interp1d_against_the_bound",
    "mmk_stft_energy_f32.x_row_stride": "test_gpu_envelope.py::test_stft_energy_against_the_bound",
    "mmk_half_neg_sqnorm_f32.y_row_stride": "test_gpu_kmeans.py::test_assign_against_the_bound",
    "mmk_kmeans_assign_f32.x_row_stride": "test_gpu_kmeans.py::test_assign_against_the_bound",
    "mmk_kmeans_assign_f32.c_row_stride": "test_gpu_kmeans.py::test_assign_against_the_bound",
    "mmk_kmeans_label_sums_f64.x_row_stride": "test_gpu_kmeans.py::test_label_sums_against_the_bound",
    "mmk_kmeans_label_sums_f64.c_row_stride": "test_gpu_kmeans.py::test_label_sums_against_the_bound",
    "mmk_kmeans_pp_step_f64.x_row_stride": "test_gpu_kmeans.py::test_pp_step_against_the_bound",
    "mmk_hpss_f32.s_batch_stride": "test_gpu_hpss.py::test_tile_edges", "mmk_hpss_f32.s_row_stride": "test_gpu_hpss.py::test_tile_edges",
    "mmk_lfilter1_f32.x_row_stride": "test_gpu_filters.py::test_lfilter1_against_the_bound",
    "mmk_row_normalize_f32.x_row_stride": "test_gpu_filters.py::test_row_normalize_against_the_bound",
    "mmk_melbank_f32.in_row_stride": "test_gpu_melspec.py::test_bank_kernel_within_the_bound_of_float64",
    "mmk_stft_mel_f32.x_row_stride": "test_gpu_melspec.py::test_fused_path_against_float64_on_magspec",
    "mmk_nmf_start_f64.x_row_stride": "test_gpu_nmf.py::test_start_against_the_a_posteriori_bound",
    "mmk_nmf_w_half_f64.x_row_stride": "test_gpu_nmf.py::test_half_sweeps_against_the_bound",
    "mmk_nmf_h_half_f64.x_row_stride": "test_gpu_nmf.py::test_half_sweeps_against_the_bound",
    "mmk_nmf_solve_f64.x_row_stride": "test_gpu_nmf.py::test_the_flag_freezes_the_result_whenever_the_host_looks",
    "mmk_nn_aggregate_f32.x_row_stride": "test_gpu_nn_filter.py::test_aggregate_on_drawn_lists",
    "mmk_nn_cosine_f32.x_row_stride": "test_gpu_neighbors.py::test_argmax_against_the_bound",
    "mmk_nn_cosine_f32.y_row_stride": "test_gpu_neighbors.py::test_argmax_against_the_bound",
    "mmk_nn_cosine_self_f32.x_row_stride": "test_gpu_hcluster.py::test_self_argmax_against_the_bound",
    "mmk_nn_topk_f32.x_row_stride": "test_gpu_qcluster.py::test_topk_against_a_corpus",
    "mmk_nn_topk_f32.y_row_stride": "test_gpu_qcluster.py::test_topk_against_a_corpus",
    "mmk_novelty_f32.x_batch_stride": "test_gpu_segment.py::test_two_clips_with_a_gap",
    "mmk_novelty_f32.x_row_stride": "test_gpu_segment.py::test_scores_against_the_bound",
    "mmk_pack_weight_f32.ldw": "test_gpu_strided_inputs.py::test_pack_weight_rows_of_a_wider_matrix",
    "mmk_pca_colstats_f64.x_row_stride": "test_gpu_pca.py::test_colstats_against_the_bound",
    "mmk_pca_cov_f64.x_row_stride": "test_gpu_pca.py::test_covariance_against_the_bound",
    "mmk_pca_project_f32.y_row_stride": "test_gpu_pca.py::test_scores_against_the_bound",
    "mmk_segment_mean_f32.x_row_stride": "test_gpu_hcluster.py::test_segment_mean_against_the_bound",
    "mmk_spline2_coef_f64.y_row_stride": _SPLINE, "mmk_spline2_eval_f32.coef_row_stride": _SPLINE,
}
NOT_UNDER_RULE = {
    **{p: OUTPUT for p in (
        "mmk_categorical_sample_f32_i64.out_stride", "mmk_cum_entropy_i64.e_row_stride", "mmk_derivative_f32.y_row_stride",
        "mmk_gemm_bias_act_f32.ldc", "mmk_gemm_bias_act_f32.group_stride", "mmk_gemm_bias_act_f32.row_stride", "mmk_gemm_f32.ldc",
        "mmk_gemm_f32.c_batch", "mmk_hpss_f32.out_batch_stride", "mmk_hpss_f32.out_row_stride", "mmk_interp1d_f32.y_row_stride",
        "mmk_lfilter1_f32.y_row_stride", "mmk_linear_f32.ldy", "mmk_nn_aggregate_f32.out_row_stride", "mmk_pca_project_f32.out_row_stride",
        "mmk_resample_f32.out_row_stride", "mmk_row_normalize_f32.y_row_stride", "mmk_segment_mean_f32.out_row_stride",
        "mmk_skinny_linear_f32.ldc", "mmk_spline2_coef_f64.coef_row_stride", "mmk_spline2_eval_f32.out_row_stride", "mmk_tr_add_ln_f32.out_ld",
        "mmk_tr_attention_f32.o_ld", "mmk_tr_attention_f32.o_cs", "mmk_s2s_last_logits.out_ld", "mmk_tr_last_logits.out_ld",
        "mmk_srnn_last_logits.ld", "mmk_srnn_last_logits_of.ld", "mmk_wavenet_last_logits.ld", "mmk_wavenet_last_logits_of.ld",
        "mmk_s2s_step.y_batch_stride", "mmk_s2s_step.y_frame_stride", "mmk_s2s_step_classes.y_batch_stride", "mmk_s2s_step_classes.y_elem_stride",
        "mmk_tr_step.y_batch_stride")},
    **{p: F64_KERNELS for p in (
        "mmk_gemm_bias_act_f32.lda", "mmk_gemm_f32.lda", "mmk_gemm_f32.a_batch", "mmk_linear_f32.ldx", "mmk_skinny_linear_f32.lda",
        "mmk_tr_add_ln_f32.y_ld", "mmk_tr_add_ln_f32.res_ld", "mmk_tr_attention_f32.q_ld", "mmk_tr_attention_f32.q_cs",
        "mmk_tr_attention_f32.kv_ld", "mmk_tr_attention_f32.kv_cs")},
    **{p: F64_SPECTRAL for p in ("mmk_resample_f32.x_row_stride", "mmk_stft_f32.x_row_stride", "mmk_stft_mag_f32.x_row_stride")},
    # the plans read the caller's tensor in place and write the generated steps into the same rows: their rows are inputs and outputs
    # at once.  PLAN_TESTS below lists what runs them between decoys (finite ones only: no NaN goes into a plan).
    **{p: PLAN for p in (
        "mmk_s2s_generate.batch_stride", "mmk_s2s_generate.frame_stride", "mmk_s2s_generate_classes.batch_stride",
        "mmk_s2s_generate_classes.elem_stride", "mmk_s2s_step.x_batch_stride", "mmk_s2s_step.x_frame_stride",
        "mmk_s2s_step_classes.x_batch_stride", "mmk_s2s_step_classes.x_elem_stride", "mmk_srnn_generate.idx_row_stride",
        "mmk_srnn_generate_multi.idx_row_stride", "mmk_srnn_warmup.idx_row_stride", "mmk_srnn_warmup_multi.idx_row_stride",
        "mmk_tr_generate.batch_stride", "mmk_tr_generate.time_stride", "mmk_tr_step.x_batch_stride", "mmk_tr_step.x_time_stride",
        "mmk_wavenet_generate.cond_row_stride", "mmk_wavenet_generate.in0_row_stride", "mmk_wavenet_warmup.cond_row_stride",
        "mmk_wavenet_warmup.in0_row_stride", "mmk_wavenet_profile_steps.cond_row_stride", "mmk_wavenet_profile_steps.in0_row_stride")},
}
REASONS = (OUTPUT, PLAN, F64_KERNELS, F64_SPECTRAL)
# Entry points of the families' files that take contiguous operands only - no stride parameter, so no entry above.  Their float operands are
# the outputs of other entry points (a covariance, a cost or score buffer); the integer lists among them are placed between decoys by
# their call helpers all the same (components_call of test_gpu_qcluster.py and test_gpu_hcluster.py).
CONTIGUOUS_ONLY = ("mmk_fa_fit_f64", "mmk_fa_transform_matrix_f64", "mmk_pca_eig_f64", "mmk_nn_components_i64", "mmk_edge_components_i64",
                   "mmk_novelty_finish_f32")
# The plans under PLAN: the class prompt lies between decoy classes on every path listed; a conditioning input between +-1e3 decoys on
# the chain, lpipe and spipe paths only - tests/net_refs.py has no conditioned case of the launch, persist and bpipe paths.
PLAN_TESTS = ("test_gpu_strided_inputs.py::test_wavenet_prompt_and_conditioning_in_place_between_decoys",
              "test_gpu_strided_inputs.py::test_sample_rnn_prompt_in_place_between_decoys",
              "test_gpu_strided_inputs.py::test_transformer_prompt_in_place_between_decoys",
              "test_gpu_networks.py::test_seq2seq_frames_in_place_ignore_what_lies_behind_a_row")
assert not set(UNDER_RULE) & set(NOT_UNDER_RULE)
SURROUND_PARAMS = {**{p: ("RULE", t) for p, t in UNDER_RULE.items()}, **{p: ("REASON", r) for p, r in NOT_UNDER_RULE.items()}}
