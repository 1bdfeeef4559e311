/*
 * mmk.h — C ABI of the MI355X (gfx950) hot-path library `libmmk_hip.so`.
 *
 * Scope: the autoregressive generate path of ktonal/mimikit and its mu-law /
 * STFT feature functionals.  The reference reaches this path
 * through two *Python* protocols, not an FFI; each entry point below names the
 * reference function it stands in for (paths relative to the reference root).
 *
 * Conventions
 *   - every function returns MMK_OK (0) or a negative error code and never
 *     throws; `mmk_last_error()` returns a thread-local message for the last
 *     failure;
 *   - all data buffers are CALLER-OWNED DEVICE pointers (e.g. torch
 *     `tensor.data_ptr()`); sizes and strides are explicit, in ELEMENTS;
 *   - strides.  Row, clip, frame and group strides and leading dimensions are honoured over the full 64-bit range: the kernels
 *     compute their offsets in 64 bits, the logits copy-outs (`*_last_logits*`) included, so a view of a buffer of more than 4 GiB is
 *     read and written where it lies.  One kernel addresses the caller's rows with a 32-bit byte offset: the Seq2Seq input projection
 *     that reads continuous frames in place; it is taken only while the frames of a call span less than 2^31 bytes, and beyond that
 *     the frames are gathered first.  tests/far_cases.py lists every stride parameter with the test that drives it beyond 4 GiB (only
 *     mmk_wavenet_profile_steps has none, with its reason);
 *   - the library allocates no device memory: plans take a caller-provided
 *     workspace whose size is reported by `*_workspace_bytes`;
 *   - streams.  Every kernel, memset and copy of a call is enqueued on its `stream` argument (a `hipStream_t`, passed as void*; any
 *     stream, blocking or not) and on no other: nothing goes to the null stream, and a call returns without waiting for `stream`
 *     - with the exceptions listed here, each of which waits for `stream` (and for nothing else) and so cannot be captured into a
 *     graph.  tests/stream_cases.py lists every entry point under one of the two rules and tests/test_gpu_streams.py holds it to it
 *     behind a busy side stream.
 *       mmk_wavenet_commit, mmk_srnn_commit, mmk_s2s_commit, mmk_tr_commit: may wait - before the workspace is laid out anew
 *         (replays of a cached graph may still be queued) and after host-built tables were copied;
 *       mmk_srnn_reset: reads the plan's error word back first;
 *       mmk_wavenet_sync_status, mmk_srnn_sync_status, mmk_s2s_sync_status: wait, then read the plan's error word (on `stream`)
 *         and clear it where it is reported;
 *       mmk_wavenet_inject_sync_error, mmk_srnn_inject_sync_error, mmk_s2s_inject_sync_error: wait for their write of the word;
 *       mmk_wavenet_profile_steps: waits for its events;
 *       mmk_edge_components_i64: once per four rounds, to read its changed-flag;
 *       mmk_pca_eig_f64: every 8 iterations, to read its convergence flag;
 *       mmk_nmf_start_f64 and mmk_nmf_solve_f64 of mmk_nmf.h: the start inside mmk_pca_eig_f64 and once more for the smallest entry and
 *         the eigenvalues, the solver every 8 iterations (its `poll`) to read its convergence flag;
 *       mmk_fa_fit_f64 of mmk_factor_analysis.h: every 8 inner iterations, to read its state.
 *     Two more waits depend on what came before the call.  mmk_wavenet_warmup, mmk_wavenet_generate, mmk_srnn_warmup(_multi),
 *     mmk_srnn_generate(_multi) and mmk_tr_generate replay a cached graph of their step kernels from a block length on (16 steps; SampleRNN: two periods of
 *     frame_sizes[0]); the graph is keyed by the call's pointers, strides and phase, and a call whose key differs from the cached
 *     one waits for `stream` before it captures again (shorter blocks and repeated keys do not wait).  And the first spectral call
 *     of a process on a device (mmk_stft*_f32, mmk_istft_f32, mmk_gla_f32) builds the twiddle and window tables on its `stream` and
 *     waits for them once; later calls, on any stream, find them ready.
 *     Graph capture.  Every stateless entry point that is not listed above can be captured into a graph on its `stream` (it allocates
 *     nothing, queries nothing and copies nothing from the host) and replayed on other contents of the same buffers, with the workspace
 *     as the last replay left it; the first spectral call of a process comes before the capture.  The plans' calls are not captured
 *     from outside: they keep state on the host (the position, the graph cache and its key, the phase) and from that block length on
 *     begin a capture of their own.  tests/graph_cases.py lists every entry point of the headers under include/ under one of the two
 *     rules and tests/test_gpu_graphs.py replays the first kind.
 *     A plan is driven from ONE stream at a time: its workspace, queues and error word are ordered by that stream alone, and a
 *     caller who moves a plan to another stream synchronises the old one first.  The stateless functions keep nothing between
 *     calls but those tables: two of them may run on two streams at once, each with its own workspace;
 *   - no torch / C++ types cross the boundary;
 *   - diagnostics (in-kernel phase stamps, timing experiments that change results) are compiled only into the diagnostic
 *     build of the library (`python -m mimikit_amd.build --diag` -> libmmk_hip_diag.so, -DMMK_DIAG); the product library has
 *     no code path that produces wrong results on purpose.
 */
#ifndef MMK_H_
#define MMK_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MMK_ABI_VERSION 6   /* 2: exec_mode in the WaveNet / SampleRNN / Seq2Seq configs, mmk_*_sync_status for all three, mmk_*_inject_sync_error;
                              * 3: `tuning` text at the end of the three configs - the library reads no environment variable;
                              * 4: act_f / act_g in the WaveNet config, mlp_act in all three, mmk_srnn_resident_warmups;
                              * 5: SimpleTransformer plans (mmk_tr_config, mmk_tr_*);
                              * 6: building-block entry points mmk_gemm_f32, mmk_gemm_bias_act_f32, mmk_gemm_partial_floats,
                              *    mmk_skinny_linear_f32, mmk_tr_attention_f32, mmk_tr_add_ln_f32; an `act` outside 0..8 is MMK_ERR_INVALID */
/* activations (mimikit/modules/activations.py: ActivationEnum, the members the HIP path evaluates) */
#define MMK_ACT_IDENTITY 0
#define MMK_ACT_TANH 1
#define MMK_ACT_SIGMOID 2
#define MMK_ACT_MISH 3
#define MMK_ACT_ABS 4
#define MMK_ACT_RELU 5
#define MMK_ACT_SOFTPLUS 6
#define MMK_ACT_SIN 7
#define MMK_ACT_COS 8
#define MMK_TUNING_CHARS 256

#define MMK_OK 0
#define MMK_ERR_INVALID (-1)     /* bad argument / shape / unsupported option value */
#define MMK_ERR_HIP (-2)         /* a HIP runtime call failed */
#define MMK_ERR_UNSUPPORTED (-3) /* option combination outside this library's coverage */
#define MMK_ERR_WORKSPACE (-4)   /* workspace too small or misaligned */
#define MMK_ERR_STATE (-5)       /* call sequence violated (e.g. generate before commit) */
#define MMK_ERR_KEY (-6)         /* unknown / missing state_dict key */

#define MMK_MAX_LAYERS 128
#define MMK_MAX_COND 4
#define MMK_MAX_TIERS 8
#define MMK_MAX_MLP_HIDDEN 4
#define MMK_MAX_STREAMS 4                  /* inputs / targets of one network (len(IOSpec.inputs), len(IOSpec.targets)) */

typedef void* mmk_stream_t; /* hipStream_t */

int mmk_abi_version(void);
/* sizeof the config struct as this library was compiled: 0 mmk_wavenet_config, 1 mmk_srnn_config, 2 mmk_s2s_config, 3 mmk_tr_config; -1 for any
 * other number -
 * what a binding that mirrors the structs by hand (ctypes, cgo, JNI) compares its own layout with before the first call */
int64_t mmk_config_bytes(int which);
/* a digest of the sources this library was compiled from (mimikit_amd/build.py: sha256 over every translation unit and header,
 * 32 hex digits; "unknown" for a build outside that script): how a caller tells a stale prebuilt library from a current one */
const char* mmk_build_digest(void);
const char* mmk_last_error(void);
/* Diagnostic: weight re-packing kernels (`*_commit`, mmk_pack_weight_f32) launched since the library was loaded.
 * The host mirror re-commits a plan only when a parameter changed (in the reference `before_generate` never
 * touches the weights, mimikit/networks/wavenet_v2.py:368-445); tests assert that through this counter. */
int64_t mmk_pack_launch_count(void);
/* Content fingerprint of `n_words` 32-bit words on the device (position-mixed hash, summed as 64-bit integers: deterministic): the host
 * mirror takes it over the concatenated weights where a generation starts, to notice writes through `tensor.data` that no version
 * counter records.  `out`: one uint64 on the device (cleared by the call). */
int mmk_fingerprint_u32(const void* words, int64_t n_words, uint64_t* out, mmk_stream_t stream);
/* the same number for `n_buffers` device buffers taken as one concatenation (host arrays of pointers and word counts), without
 * concatenating them: one launch per 96 buffers */
int mmk_fingerprint_buffers_u32(const void* const* buffers, const int64_t* n_words, int32_t n_buffers, uint64_t* out, mmk_stream_t stream);

/* ------------------------------------------------------------------------
 * Feature functionals
 * ---------------------------------------------------------------------- */

/* MuLawCompress.torch_func (mimikit/features/functionals.py:330-338).
 * codes[i] = int64(trunc((sign(x)·log1p(mu·|x|·C)/log1p(mu·C) + 1)/2·mu + 0.5)), mu = q_levels-1.
 * `edges` holds the q_levels-1 ascending fp32 decision thresholds of that
 * formula (edges[c-1] = smallest x whose code is >= c), so in-range inputs are
 * quantised exactly as the reference does; inputs outside [edges[0], +1] fall
 * back to direct fp32 evaluation of the formula (no clamp, as the reference). */
int mmk_mulaw_compress_f32_i64(const float* x, int64_t* codes, int64_t n, int32_t q_levels,
                               float compression, const float* edges, mmk_stream_t stream);

/* MuLawExpand.torch_func (mimikit/features/functionals.py:361-369).
 * `table` holds the q_levels expanded values of codes 0..q_levels-1; codes
 * outside that range are evaluated directly in fp32. */
int mmk_mulaw_expand_i64_f32(const int64_t* codes, float* x, int64_t n, int32_t q_levels,
                             float compression, const float* table, mmk_stream_t stream);

/* Resample.torch_func (mimikit/features/functionals.py:292-310) = torchaudio.functional.resample(x, orig_sr, target_sr):
 * polyphase windowed-sinc FIR.  orig / nnew are the two rates divided by their gcd; `table` is the (nnew, 2*width + orig)
 * filter bank torchaudio builds (Hann-windowed sinc, lowpass_filter_width 6, rolloff 0.99), row j = output phase j.
 * x: (batch, n_in) rows x_row_stride apart; out: (batch, mmk_resample_n_out(n_in, orig, nnew)) rows out_row_stride apart.
 * Used between the networks of an EnsembleGenerator event (mimikit/models/ensemble_generator.py:113-144). */
int64_t mmk_resample_n_out(int64_t n_in, int32_t orig, int32_t nnew);
int mmk_resample_f32(const float* x, int64_t x_row_stride, int32_t batch, int64_t n_in, const float* table, int32_t orig,
                     int32_t nnew, int32_t width, float* out, int64_t out_row_stride, mmk_stream_t stream);

/* One first-order filter section per row, torchaudio.functional.lfilter(x, a = [1, a1], b = [b0, b1], clamp=False):
 *     y[n] = b0 x[n] + b1 x[n-1] - a1 y[n-1],    zero initial state, fp32
 * - Emphasis (b = [1, -e], a1 = 0), Deemphasis (b = [1 - e, 0], a1 = -e) and RemoveDC (b = [1, -1], a1 = -0.99) of
 * mimikit/features/functionals.py:211-288.  x, y: (batch, n) rows x_row_stride / y_row_stride elements apart (views of longer tensors),
 * 4-byte aligned and no more; y may not overlap x.  a1 == 0 is one streaming pass and needs no workspace; otherwise the row is cut into
 * chunks of MMK_LFILTER1_CHUNK samples (workgroups of MMK_LFILTER1_WG lanes that own MMK_LFILTER1_RUN consecutive samples each) and two
 * launches scan it, with one float per chunk in `workspace` (mmk_lfilter1_workspace_floats floats; may be NULL where n fits one chunk).
 * No atomics and one fixed order of every sum: the result is the same from run to run.  |a1| > 1 is MMK_ERR_UNSUPPORTED. */
#define MMK_LFILTER1_RUN 16
#define MMK_LFILTER1_WG 256
#define MMK_LFILTER1_CHUNK 4096   /* = MMK_LFILTER1_RUN * MMK_LFILTER1_WG */
size_t mmk_lfilter1_workspace_floats(int32_t batch, int64_t n);
int mmk_lfilter1_f32(const float* x, int64_t x_row_stride, int32_t batch, int64_t n, float b0, float b1, float a1, float* y,
                     int64_t y_row_stride, float* workspace, mmk_stream_t stream);
/* torch.nn.functional.normalize(x, p, dim=-1, eps) per row: y = x / max(||x||_p, eps); p: 0 = inf, 1, 2 (MMK_ERR_UNSUPPORTED otherwise).
 * Rows as above.  Two launches over chunks of MMK_LFILTER1_CHUNK samples: per-chunk partial norms into `workspace`
 * (mmk_row_normalize_workspace_floats floats, always needed), added up in one fixed order by the scale pass. */
size_t mmk_row_normalize_workspace_floats(int32_t batch, int64_t n);
int mmk_row_normalize_f32(const float* x, int64_t x_row_stride, int32_t batch, int64_t n, int32_t p, float eps, float* y,
                          int64_t y_row_stride, float* workspace, mmk_stream_t stream);

/* NearestNextNeighbor's alignment (mimikit/models/nnn.py:14-49): cosine distances of `batch` prompts of n frames against a corpus of m frames
 * over k bins, then the subsequence DTW (steps (1,1), (0,1), (1,0), unit weights) whose last row's FIRST minimum is the end column:
 *     D[0, j] = C[0, j],   D[i, 0] = D[i-1, 0] + C[i, 0],   D[i, j] = C[i, j] + min(D[i-1, j-1], D[i, j-1], D[i-1, j])
 * (NearestNextNeighbor.predict_start_frame = end column + 1).  n <= MMK_NNN_MAX_ROWS (one wave per clip; MMK_ERR_UNSUPPORTED beyond),
 * m < n is legal, n < 1, m < 1, k < 1 and batch < 1 are MMK_ERR_INVALID.  NaN in the inputs is not handled.
 *
 * mmk_inv_row_norm_f32: inv_norm[b * rows + r] = 1 / |x[b][r]|_2, and 0 for a row of norm 0 (sklearn's cosine distance leaves such a row as
 * zeros: distance 1 to everything).  Rows are x_row_stride floats apart, clips x_batch_stride; 4-byte alignment is enough.
 * mmk_cosine_cost_f32: cost[b][j][i] = clamp(1 - <|x_b,i|, |y_j|> rx[b * n + i] ry[j], 0, 2) - |.| is applied on load - as
 * (batch, m, n_pad) contiguous floats, 16-byte aligned, n_pad = n rounded up to MMK_NNN_ROW_PAD (the padding holds 1).  k need not be a multiple
 * of anything and tails are masked here, not padded by the caller.  fp32 MFMA with fp32 accumulation in one fixed order.
 * mmk_dtw_subseq_f32: over such a cost tensor; end_col[b] (int64), end_val[b] = D[n-1, end_col[b]] and, where last_row is not NULL,
 * last_row[b][j] = D[n-1, j] ((batch, m) contiguous).  Each D is one rounded add of an exact minimum: bit-identical to the sequential fp32
 * loop over the same costs.  Costs are fetched MMK_NNN_LOOKAHEAD anti-diagonals ahead of the chain. */
#define MMK_NNN_MAX_ROWS 64
#define MMK_NNN_ROW_PAD 16
#define MMK_NNN_LOOKAHEAD 16
int mmk_inv_row_norm_f32(const float* x, int64_t x_batch_stride, int64_t x_row_stride, int32_t batch, int64_t rows, int32_t k,
                         float* inv_norm, mmk_stream_t stream);
int mmk_cosine_cost_f32(const float* x, int64_t x_batch_stride, int64_t x_row_stride, const float* rx, int32_t batch, int32_t n,
                        const float* y, int64_t y_row_stride, const float* ry, int64_t m, int32_t k, float* cost, mmk_stream_t stream);
int mmk_dtw_subseq_f32(const float* cost, int32_t batch, int32_t n, int64_t m, int64_t* end_col, float* end_val, float* last_row,
                       mmk_stream_t stream);

/* Scoring generated clips (mimikit/extract/from_neighbors.py:13-19 nearest_neighbor, :44-55 cum_entropy; demos/checkpoint_k_bests.py:36-46).
 *
 * mmk_nn_cosine_f32: for `rows` query frames x (x_row_stride floats apart) and m corpus frames y (y_row_stride apart) over k bins, with
 * rx / ry their inverse norms from mmk_inv_row_norm_f32,
 *     c[r, j] = clamp(<x_r, y_j> rx[r] ry[j], -1, 1)       (no |.| on load, unlike mmk_cosine_cost_f32)
 * index[r] (int64) = the FIRST j that maximises c[r, :], cos_best[r] = that value.  A GEMM on v_mfma_f32_32x32x2_f32 whose epilogue is the row
 * arg-max: the matrix is never written.  The sum over k has one fixed order that does not depend on where a row or a column sits in a tile, so
 * two identical corpus frames have bit-identical cosines and ties go to the lower index.  rows, m and k need not be multiples of anything and
 * 4-byte alignment is enough: tails are masked here, the caller pads nothing.  The corpus is cut into spans of MMK_NN_SPAN frames; a workgroup
 * keeps its running (value, index) pairs in registers across its span, writes one pair per row and span to `workspace`
 * (mmk_nn_cosine_workspace_bytes(rows, m) = 8 bytes per row and span, never O(rows * m)), and a second small launch joins the spans by
 * "greater value, then lower index".  No atomics: repeated calls agree bit for bit.  rows < 1, m < 1, k < 1: MMK_ERR_INVALID; a workspace that
 * is too small: MMK_ERR_WORKSPACE; m >= 2^31 - MMK_NN_SPAN: MMK_ERR_UNSUPPORTED.  NaN in the inputs is not handled.
 *
 * mmk_cum_entropy_i64: `batch` rows of t int64 items, row_stride apart.  With p_i(s) = (occurrences of item i in row[0 .. s]) / (s + 1),
 *     e[s] = -sum_i p_i(s) log p_i(s)  =  log(s + 1) - S(s) / (s + 1),    S(s) = sum_{u <= s} (f(r_u + 1) - f(r_u)),  f(c) = c log c,
 * r_u = the number of earlier occurrences of row[u] (counted in the kernel; no items x t table).  total[b] = sum_s e[s]; where e is not NULL,
 * e[b][s] as well (rows e_row_stride apart).  fp64 throughout, the prefix sum in one fixed order, e clamped at 0, each result rounded to fp32
 * once.  t > MMK_CUM_ENTROPY_MAX_T: MMK_ERR_UNSUPPORTED (one workgroup ranks a row: t^2 / 2 comparisons); batch < 1, t < 1: MMK_ERR_INVALID. */
#define MMK_NN_SPAN 2048
#define MMK_CUM_ENTROPY_MAX_T 32768
size_t mmk_nn_cosine_workspace_bytes(int64_t rows, int64_t m);
int mmk_nn_cosine_f32(const float* x, int64_t x_row_stride, const float* rx, int64_t rows, const float* y, int64_t y_row_stride,
                      const float* ry, int64_t m, int32_t k, int64_t* index, float* cos_best, void* workspace, size_t workspace_bytes,
                      mmk_stream_t stream);
int mmk_cum_entropy_i64(const int64_t* items, int64_t row_stride, int32_t batch, int64_t t, float* total, float* e, int64_t e_row_stride,
                        mmk_stream_t stream);

/* Labelling corpus frames (mimikit/extract/clusters.py:157-205 HCluster): one level is mmk_inv_row_norm_f32, then the three below.
 *
 * mmk_nn_cosine_self_f32: mmk_nn_cosine_f32 with the corpus = the queries and frame r left out of row r: index[r] = the FIRST j != r that
 * maximises clamp(<x_r, x_j> rx[r] rx[j], -1, 1), cos_best[r] = that value.  The same kernel (a compile-time switch that tests j != r only
 * in the tiles the diagonal crosses), the same order of the sum, tie rule and span / merge workspace (mmk_nn_cosine_workspace_bytes(rows,
 * rows)), no atomics.  An all-zero x gives index 0 for every row but row 0, which gets 1.  rows < 2, k < 1: MMK_ERR_INVALID.
 *
 * mmk_nn_components_i64: labels[i] (int64) = the number of the weakly connected component of node i in the functional graph i -> nearest[i],
 * components numbered by rising smallest member; *n_components (one int64 on the device) = their count.  Right for any functional graph -
 * cycles of any length, self-loops, one chain of n nodes: ceil(log2 n) + 1 rounds of pointer doubling with a carried minimum find the
 * smallest node of every component's cycle, an integer atomicMin (order-free) the component's smallest member, and a prefix count over the
 * nodes that are their component's smallest member the number (a kernel of this call).  An entry of `nearest` outside [0, n) is the caller's
 * error: it is not reported (it is clamped, never used as an address).  Workspace: mmk_nn_components_workspace_bytes(n) = 20 bytes per node
 * and 4 per 256 nodes.  n < 1: MMK_ERR_INVALID; n >= 2^31: MMK_ERR_UNSUPPORTED.
 *
 * mmk_segment_mean_f32: out[s][0 .. k) = the mean of the rows x[order[u]], offsets[s] <= u < offsets[s + 1], for s < n_segments: `order`
 * holds n row numbers (int64), `offsets` n_segments + 1 rising positions in it.  Members are added in the order given in fp64, divided once
 * and rounded to fp32 once.  n_segments < 1 or > n (some segment would be empty), n < 1, k < 1: MMK_ERR_INVALID; an empty segment among
 * n_segments <= n is not looked for on the device (its row is NaN).
 *
 * All three: raw pointers and strides, 4-byte alignment of the float data (8 of the int64 data) is enough, tails are masked here, nothing but
 * the stated outputs and workspace is written, two calls give the same bits.  NaN in the inputs is not handled. */
int mmk_nn_cosine_self_f32(const float* x, int64_t x_row_stride, const float* rx, int64_t rows, int32_t k, int64_t* index, float* cos_best,
                           void* workspace, size_t workspace_bytes, mmk_stream_t stream);
size_t mmk_nn_components_workspace_bytes(int64_t n);
int mmk_nn_components_i64(const int64_t* nearest, int64_t n, int64_t* labels, int64_t* n_components, void* workspace, size_t workspace_bytes,
                          mmk_stream_t stream);
int mmk_segment_mean_f32(const float* x, int64_t x_row_stride, int64_t n, int32_t k, const int64_t* order, const int64_t* offsets,
                         int64_t n_segments, float* out, int64_t out_row_stride, mmk_stream_t stream);

/* The k nearest frames and the components of a graph (mimikit/extract/clusters.py:27-98 QCluster).
 *
 * mmk_nn_topk_f32: for `rows` query frames x and m corpus frames y over k bins, with a scale per query, a scale and a shift per corpus frame,
 *     key[r, j] = clamp((<x_r, y_j> * qscale[r]) * cscale[j] + cshift[j], key_min, key_max)        (three roundings after the sum; limits of
 *     -inf and +inf: no clamp)
 * index[r][0 .. t) (int64) = the t corpus frames of the largest keys, in falling key order, equal keys in rising index order; key[r][0 .. t)
 * those keys.  Cosine similarity: the two inverse norms of mmk_inv_row_norm_f32, a shift of 0 and the limits -1 and 1 - with t = 1 the index
 * and key are those of mmk_nn_cosine_f32 / mmk_nn_cosine_self_f32.  Euclidean distance: scales of 1, no limits and cshift =
 * mmk_half_neg_sqnorm_f32(y) = -|y_j|^2 / 2: the largest key is the smallest distance.  self_exclude != 0: the corpus IS the
 * queries (y == x, the same stride, m == rows, or MMK_ERR_INVALID) and frame r is left out of row r.  Where a row has fewer than t
 * candidates the slots behind them hold index -1 and key -inf.  The same tile walk, order of the sum over k and span / merge scheme as
 * mmk_nn_cosine_f32: a lane keeps its rows' t best in registers across a span, one list per row and span goes to `workspace`
 * (mmk_nn_topk_workspace_bytes(rows, m, t) = 8 t bytes per row and span, never O(rows * m)), a second launch joins the spans in rising span
 * order.  No atomics: repeated calls agree bit for bit.  t > MMK_NN_TOPK_MAX, m >= 2^31 - MMK_NN_SPAN: MMK_ERR_UNSUPPORTED; rows, m, k or
 * t < 1: MMK_ERR_INVALID; a workspace that is too small: MMK_ERR_WORKSPACE.  NaN and inf in the inputs are not handled.
 *
 * mmk_half_neg_sqnorm_f32: out[j] = -|y_j|^2 / 2, the squares added in fp64 in one fixed order and rounded to fp32 once.
 *
 * mmk_edge_components_i64: labels[i] (int64) = the number of the connected component of node i in the undirected graph of the n_edges edges
 * (src[e], dst[e]) over n nodes, components numbered by rising smallest member; *n_components (one int64 on the device) = their count.
 * Self-loops, repeated and reversed edges are allowed, n_edges may be 0 (src and dst may then be NULL), a node without an edge is a
 * component of its own; an edge with an endpoint outside [0, n) is the caller's error and is left out.  Min-hooking with an integer
 * atomicMin and pointer jumping until a round changes nothing; the fixed point is every node's smallest fellow member in whatever order the
 * atomics land, so two calls give the same labels.  THE CALL WAITS FOR THE STREAM once per four rounds to read its changed-flag: it cannot be
 * captured into a graph.  Workspace: mmk_edge_components_workspace_bytes(n) = 12 bytes per node, 4 per 256 nodes and 4.  n < 1,
 * n_edges < 0: MMK_ERR_INVALID; n >= 2^31: MMK_ERR_UNSUPPORTED.
 *
 * Raw pointers and strides, 4-byte alignment of the float data (8 of the int64 data) is enough, tails are masked here, nothing but the stated
 * outputs and workspace is written. */
#define MMK_NN_TOPK_MAX 16
size_t mmk_nn_topk_workspace_bytes(int64_t rows, int64_t m, int32_t t);
int mmk_nn_topk_f32(const float* x, int64_t x_row_stride, const float* qscale, int64_t rows, const float* y, int64_t y_row_stride,
                    const float* cscale, const float* cshift, float key_min, float key_max, int64_t m, int32_t k, int32_t t, int32_t self_exclude,
                    int64_t* index, float* key, void* workspace, size_t workspace_bytes, mmk_stream_t stream);
int mmk_half_neg_sqnorm_f32(const float* y, int64_t y_row_stride, int64_t rows, int32_t k, float* out, mmk_stream_t stream);
size_t mmk_edge_components_workspace_bytes(int64_t n);
int mmk_edge_components_i64(const int64_t* src, const int64_t* dst, int64_t n_edges, int64_t n, int64_t* labels, int64_t* n_components,
                            void* workspace, size_t workspace_bytes, mmk_stream_t stream);

/* Cutting corpus frames into segments (mimikit/extract/segment.py:21-174: discontinuity_scores, pick_globally_sorted_maxes).
 *
 * mmk_novelty_f32: for `batch` clips of `frames` frames over `bins` bins (clips x_batch_stride floats apart, rows x_row_stride) and n_half
 * half-widths h_q (a HOST array), with d(r, c) = 1 - <x_r, x_c> rx[r] rx[c] the cosine distance, d(r, r) = 0, d = 1 where a frame is zero,
 *     raw[b][q][i] = 1 / (4 h_q^2) sum_{a = -h_q .. h_q, a != 0} sum_{b = -h_q .. h_q, b != 0} -sign(a) sign(b) d(i + a, i - 1 + b)
 * where a term whose row or column lies outside [0, frames) counts 0: the normalised checkerboard of 2 h_q + 1 slid along the diagonal,
 * centred on (i, i - 1) as the reference's is.  raw: (batch, n_half, frames) contiguous.  inv_norm: (batch, frames) contiguous from
 * mmk_inv_row_norm_f32, or NULL: the kernel then computes the norms itself, by the same code.  One launch; a workgroup owns
 * MMK_NOVELTY_TILE output frames, forms the Gram tile of the frames their boards touch on the fp32 matrix pipe and sums the boards from LDS
 * in fp64 in one fixed order (rounded to fp32 once): neither the distances nor their band are written, and a half-width's bits do not
 * depend on the other half-widths of the call.  It differs from a numba run of the reference only where that run's out-of-bounds writes
 * land.  n_half > MMK_NOVELTY_MAX_KERNELS, a half-width > MMK_NOVELTY_MAX_HALF: MMK_ERR_UNSUPPORTED; frames < 2, bins,
 * batch, n_half or a half-width < 1: MMK_ERR_INVALID.
 *
 * mmk_novelty_finish_f32: scores[b][q][i] = raw[b][q][i] - min_i raw[b][q][:] and dg[b][i] = (sum_q scores[b][q][i]) / n_half, the sum in
 * rising q.  scores (batch, n_half, frames) and dg (batch, frames) contiguous, neither overlapping raw.  Workspace:
 * mmk_novelty_finish_workspace_floats(batch, n_half, frames) floats (one per 4096 frames of a row).
 *
 * mmk_pick_peaks_f32: picked[m] (one byte per index) = 1 where pick_globally_sorted_maxes(x, wait_before, wait_after, min_strength)
 * accepts index m, else 0.  With lo / hi the global minimum / maximum of x, a candidate is an index with x[m] > x[m-1] and x[m] >= x[m+1]
 * (the ends padded with themselves), (x[m] - min of x over scipy's window of wait_before + wait_after around m, lo outside the array)
 * / (hi - lo) >= min_strength (evaluated in fp64), and x[m] above the means of x[max(0, m - wait_before) : m] and of
 * x[m : min(n, m + wait_after)] (fp64 sums in rising index order).  Candidates are taken by falling x, equal values by rising index (the
 * reference's argsort is not stable there), and one is accepted unless an accepted one lies in [m - wait_before, m + wait_after).  A
 * constant x has no candidate.  Three launches, the last one workgroup; no host synchronisation.  Workspace:
 * mmk_pick_peaks_workspace_bytes(n) = 4 n + 8 bytes.  A wait > MMK_NOVELTY_MAX_WAIT: MMK_ERR_UNSUPPORTED; n < 1, a negative wait, both
 * waits 0 or a NaN min_strength: MMK_ERR_INVALID.
 *
 * All three: 4-byte alignment of the float data is enough, tails are masked here, nothing but the stated outputs and workspace is written,
 * no atomics: two calls give the same bits.  NaN in the inputs is not handled. */
#define MMK_NOVELTY_TILE 64
#define MMK_NOVELTY_MAX_KERNELS 8
#define MMK_NOVELTY_MAX_HALF 32
#define MMK_NOVELTY_MAX_WAIT 1024
int mmk_novelty_f32(const float* x, int64_t x_batch_stride, int64_t x_row_stride, const float* inv_norm, int32_t batch, int64_t frames,
                    int32_t bins, const int32_t* halves, int32_t n_half, float* raw, mmk_stream_t stream);
size_t mmk_novelty_finish_workspace_floats(int32_t batch, int32_t n_half, int64_t frames);
int mmk_novelty_finish_f32(const float* raw, int32_t batch, int32_t n_half, int64_t frames, float* scores, float* dg, float* workspace,
                           size_t workspace_floats, mmk_stream_t stream);
size_t mmk_pick_peaks_workspace_bytes(int64_t n);
int mmk_pick_peaks_f32(const float* x, int64_t n, int32_t wait_before, int32_t wait_after, double min_strength, uint8_t* picked,
                       void* workspace, size_t workspace_bytes, mmk_stream_t stream);

/* Principal components of corpus frames (mimikit/features/functionals.py:1114-1138 PCA: sklearn's StandardScaler, then sklearn's PCA).
 * x: n frames of d bins, fp32, rows x_row_stride apart; everything else is fp64 on the device and contiguous.
 *
 * mmk_pca_colstats_f64: scale[j] = the population (ddof 0) standard deviation of column j, or 1 where the column counts as constant by
 * sklearn's rule var <= n eps var + (n mu eps)^2 (eps = 2^-52); mean[j] = mu_j + m_j scale[j], where mu is the column mean and m the
 * column mean of (x - mu) / scale - the mean that sklearn's PCA subtracts after the scaler, folded in.  Three passes of per-chunk partial
 * sums added in rising chunk order.  Workspace: mmk_pca_colstats_workspace_bytes(n, d).
 *
 * mmk_pca_cov_f64: c (d, d) = Z^T Z / (n - 1) with Z = (x - mean) / scale, formed while the tiles are loaded and never written.
 * v_mfma_f64_16x16x4_f64 on 64 x 64 blocks of the lower block triangle, the rows split into runs over workgroups whose partial blocks
 * (workspace: mmk_pca_cov_workspace_bytes(n, d)) a second launch adds in rising run order; c[i][j] and c[j][i] are one value.  n < 2:
 * MMK_ERR_INVALID.
 *
 * mmk_pca_eig_f64: the n_components eigenpairs of the symmetric c with the largest eigenvalues, falling: components (n_components, d),
 * each of unit length with its entry of largest magnitude (the first of equals) positive - sklearn 1.5+'s svd_flip(u_based_decision=
 * False) - and variance (n_components) = the eigenvalues, negative ones as 0.  Block subspace iteration with a Rayleigh-Ritz step on
 * min(d, n_components + 16) columns from a fixed start block: Householder QR (orthonormal whatever the block's rank), C Q by
 * v_mfma_f64_16x16x4_f64, a cyclic Jacobi eigensolver of the small matrix in one workgroup.  It stops when
 * max_k |C q_k - theta_k q_k|_2 <= MMK_PCA_TOL |C|_inf over the first n_components columns; a device flag freezes the result at that
 * iteration, which *n_iter (HOST memory) receives.  THE CALL WAITS FOR THE STREAM every 8 iterations to read the flag: it cannot be
 * captured into a graph.  max_iter = 0: MMK_PCA_MAX_ITER; reaching the cap is MMK_ERR_CONVERGENCE and the message names the residual.
 * No eigendecomposition of size d is formed.  Workspace: mmk_pca_eig_workspace_bytes(d, n_components).
 *
 * mmk_pca_project_f32: out[i][k] (fp32, rows out_row_stride apart) = sum_j ((y[i][j] - mean[j]) / scale[j]) components[k][j], per entry
 * one fp64 fma chain over rising j, rounded to fp32 once.
 *
 * d > MMK_PCA_MAX_D, n_components > MMK_PCA_MAX_COMPONENTS: MMK_ERR_UNSUPPORTED.  fp32 data 4-byte, fp64 data and workspaces 8-byte
 * aligned; tails are masked here; nothing but the stated outputs and workspace is written; no atomics: two calls give the same bits.
 * NaN and inf in the inputs are not handled. */
#define MMK_ERR_CONVERGENCE (-7) /* an iteration reached its cap before its stop rule */
#define MMK_PCA_MAX_D 4096
#define MMK_PCA_MAX_COMPONENTS 64
#define MMK_PCA_MAX_ITER 4000
#define MMK_PCA_TOL 1e-12
size_t mmk_pca_colstats_workspace_bytes(int64_t n, int32_t d);
int mmk_pca_colstats_f64(const float* x, int64_t x_row_stride, int64_t n, int32_t d, double* mean, double* scale, void* workspace,
                         size_t workspace_bytes, mmk_stream_t stream);
size_t mmk_pca_cov_workspace_bytes(int64_t n, int32_t d);
int mmk_pca_cov_f64(const float* x, int64_t x_row_stride, int64_t n, int32_t d, const double* mean, const double* scale, double* c,
                    void* workspace, size_t workspace_bytes, mmk_stream_t stream);
size_t mmk_pca_eig_workspace_bytes(int32_t d, int32_t n_components);
int mmk_pca_eig_f64(const double* c, int32_t d, int32_t n_components, int32_t max_iter, double* components, double* variance,
                    int32_t* n_iter, void* workspace, size_t workspace_bytes, mmk_stream_t stream);
int mmk_pca_project_f32(const float* y, int64_t y_row_stride, int64_t m, int32_t d, const double* mean, const double* scale,
                        const double* components, int32_t n_components, float* out, int64_t out_row_stride, mmk_stream_t stream);

/* STFT.torch_func with coordinate="mag" == MagSpec.torch_func
 * (mimikit/features/functionals.py:507-524, :576-606): periodic-Hann framed
 * real FFT magnitudes.  x: (batch, n_samples) rows `x_row_stride` apart,
 * already length-fixed by the caller (STFT._fix_length, :468-486).
 * center != 0 pads n_fft/2 zeros on both sides (pad_mode="constant").
 * out: (batch, n_frames, n_fft/2+1) contiguous, n_frames as returned by
 * mmk_stft_n_frames.  n_fft must be a power of two in [64, 4096]. */
int64_t mmk_stft_n_frames(int64_t n_samples, int32_t n_fft, int32_t hop, int32_t center);
int mmk_stft_mag_f32(const float* x, int64_t x_row_stride, int32_t batch, int64_t n_samples,
                     int32_t n_fft, int32_t hop, int32_t center, float* out, mmk_stream_t stream);

/* STFT.torch_func with a complex coordinate (mimikit/features/functionals.py:506-523):
 * torch.stft(x, n_fft, hop, window=hann_window(n_fft), center, pad_mode, return_complex=True)
 * transposed to (batch, n_frames, n_fft/2+1), then
 *   coordinate 0 'car'   -> (..., 2) = (real, imag)
 *   coordinate 1 'pol'   -> (..., 2) = (abs, angle)
 *   coordinate 2 'angle' -> angle only, no trailing dimension.
 * reflect != 0 selects pad_mode="reflect" (needs n_samples > n_fft/2), else zeros.
 * n_fft: a power of two in [64, 4096] (MMK_ERR_UNSUPPORTED otherwise). */
#define MMK_STFT_CAR 0
#define MMK_STFT_POL 1
#define MMK_STFT_ANGLE 2
int mmk_stft_f32(const float* x, int64_t x_row_stride, int32_t batch, int64_t n_samples, int32_t n_fft,
                 int32_t hop, int32_t center, int32_t reflect, int32_t coordinate, float* out,
                 mmk_stream_t stream);

/* Envelop's frame energies (mimikit/features/functionals.py:816-818: MagSpec, then sum over the bins), without the spectrogram:
 *     out[b][f] = sum_k |STFT_b[f][k]|,   k = 0 .. n_fft/2
 * Frames, window (periodic Hann), padding (center, reflect as in mmk_stft_f32: reflect needs n_samples > n_fft/2) and the n_fft range
 * (a power of two in [64, 4096], MMK_ERR_UNSUPPORTED otherwise) are those of mmk_stft_f32; out: (batch, mmk_stft_n_frames()) contiguous.
 * An epilogue of the same transforms: a frame's magnitudes are added per lane in bin order, then over the wave (a butterfly) and, for
 * the sizes that take a workgroup per frame pair, over the waves in order.  One float per frame is written: no atomics, no scratch,
 * the same result from run to run. */
int mmk_stft_energy_f32(const float* x, int64_t x_row_stride, int32_t batch, int64_t n_samples, int32_t n_fft,
                        int32_t hop, int32_t center, int32_t reflect, float* out, mmk_stream_t stream);

/* Interpolate (mimikit/features/functionals.py:867-916): each row resampled from n knots at 0 .. n-1 to n_out points, one streaming pass.
 *   align 1: at np.linspace(0, n-1, n_out) - double(i) * step with step = (n-1) / (n_out-1) in float64 and the last position forced to n-1,
 *            as numpy does, so a position is the double scipy.interpolate.interp1d sees (Interpolate.np_func)
 *   align 0: at max(fma(float(n) / float(n_out), i + 0.5, -0.5), 0) in fp32, as the CPU kernel of torch.nn.functional.interpolate(mode="linear",
 *            align_corners=False) computes it (Interpolate.torch_func; one rounding: its vectorised build fuses the two operations); n_out == n copies
 *   mode  0: linear;  1: 'previous', y[floor(position)] (align 1 only).
 * x: (batch, n) rows x_row_stride apart, y: (batch, n_out) rows y_row_stride apart, 4-byte aligned, not overlapping.
 * n < 2, n_out < 1, another mode / align or 'previous' with align 0: MMK_ERR_INVALID. */
#define MMK_INTERP_LINEAR 0
#define MMK_INTERP_PREVIOUS 1
int mmk_interp1d_f32(const float* x, int64_t x_row_stride, int32_t batch, int64_t n, float* y, int64_t y_row_stride, int64_t n_out,
                     int32_t mode, int32_t align, mmk_stream_t stream);

/* Derivative (mimikit/features/functionals.py:960-974, derivative_torch) as one pass.  With xp the odd reflection of the row about its ends,
 * xp[-m] = x[0] + (x[0] - x[m]), xp[n-1+m] = x[n-1] + (x[n-1] - x[n-1-m]), and L = max_lag:
 *     y[i] = sum_{d=1..L} ((xp[i+d] - x[i]) + (x[i] - xp[i-d])) * (1/d) / 2 / L
 * added in lag order, each term rounded as the reference rounds it.  A workgroup stages MMK_DERIV_TILE samples and a halo of L on either
 * side in LDS.  Rows as above.  n <= max_lag or max_lag < 1: MMK_ERR_INVALID; max_lag > MMK_DERIV_MAX_LAG: MMK_ERR_UNSUPPORTED
 * (the reference's Samplifyer goes to 33). */
#define MMK_DERIV_MAX_LAG 64
#define MMK_DERIV_TILE 1024
int mmk_derivative_f32(const float* x, int64_t x_row_stride, int32_t batch, int64_t n, int32_t max_lag, float* y, int64_t y_row_stride,
                       mmk_stream_t stream);

/* HarmonicSource / PercussiveSource (mimikit/features/functionals.py:736-791): librosa.decompose.hpss(S, kernel_size, power, margin) of a
 * non-negative spectrogram as ONE launch.  s: (batch, frames, bins), time-major (the layout before the reference's transpose); rows
 * s_row_stride elements apart (>= bins), clips s_batch_stride apart, 4-byte aligned and no more.
 *   harm_median[t][b] = running median over win_harm frames of bin b, perc_median[t][b] = running median over win_perc bins of frame t:
 *     scipy.ndimage.median_filter(mode="reflect"): a window of s at i covers i - s/2 .. i - s/2 + s - 1, the result is its element of rank
 *     s/2 (the upper median of an even window), indices outside the axis fold by half-sample reflection (d c b a | a b c d | d c b a).
 *     Selections: bit-identical to scipy's.  A median never crosses a clip.
 *   mask_harm = softmask(harm, fl(perc * margin_harm)), mask_perc = softmask(perc, fl(harm * margin_perc)) with
 *     softmask(X, R): Z = max(X, R); bad = Z < FLT_MIN; m = (X / Z)^power, r = (R / Z)^power; m / (m + r), and where bad 0.5 if both margins
 *     are 1, else 0.  power == 1 takes no powf; power == +inf is the hard mask X > R.
 *   harmonic = s * mask_harm, percussive = s * mask_perc.
 * Any of the four outputs may be NULL (at least one is not); only the others are written, rows out_row_stride (>= bins) and clips
 * out_batch_stride apart; they may not overlap s or one another.  No workspace.  A workgroup owns MMK_HPSS_TILE_FRAMES x MMK_HPSS_TILE_BINS
 * outputs and stages them with a halo of win - 1 along each axis in LDS; one wave walks the tile's bins along time, one its frames along
 * frequency (the walk's step is the tile).
 * A window < 1, frames < win_harm / 2 or bins < win_perc / 2 (scipy folds such an axis more than once; that rule is not reproduced),
 * a margin < 1, power <= 0 or NaN, no output, frames / bins / batch < 1: MMK_ERR_INVALID.  A window > MMK_HPSS_MAX_KERNEL:
 * MMK_ERR_UNSUPPORTED.  Negative or NaN bins are not looked for (librosa raises on negative ones): their results are unspecified. */
#define MMK_HPSS_MAX_KERNEL 63
#define MMK_HPSS_TILE_FRAMES 64
#define MMK_HPSS_TILE_BINS 64
int mmk_hpss_f32(const float* s, int64_t s_batch_stride, int64_t s_row_stride, int32_t batch, int64_t frames, int32_t bins,
                 int32_t win_harm, int32_t win_perc, float power, float margin_harm, float margin_perc,
                 float* harmonic, float* percussive, float* harm_median, float* perc_median,
                 int64_t out_batch_stride, int64_t out_row_stride, mmk_stream_t stream);

/* MelSpec / MFCC (mimikit/features/functionals.py:650-707): librosa.feature.melspectrogram(S=...) and librosa.feature.mfcc(S=...) of
 * magnitude frames, the mel filter bank in banded form.  librosa's bank has at most two non-zero weights per bin and each band's
 * non-zeros are one run of bins, so band m is three int32 (first bin lo_m, length len_m >= 0, offset off_m into `weights`) and
 *     mel[m] = sum_{j < len_m} weights[off_m + j] * mag[lo_m + j]
 * added in ascending bin order as one fmaf chain from 0 in fp32; a band of length 0 gives 0.  With a DCT matrix,
 *     out[c] = sum_{m < n_mels} dct[m * n_mfcc + c] * mel[m],   c < n_mfcc
 * in ascending band order, the same way; the bands then stay in LDS.  Every entry below runs this one epilogue, so equal magnitudes
 * give equal bits whichever entry made them.
 *   band: (n_mels, 3) int32 on the device, band_host: the same values in host memory (read for the checks only, before the launch);
 *   weights: n_weights floats on the device; bank_n_bins: the number of bins the bank was built for;
 *   dct: NULL (then n_mfcc == 0), or the (n_mfcc, n_mels) matrix TRANSPOSED, (n_mels, n_mfcc) row-major on the device, 1 <= n_mfcc <= n_mels.
 * Errors: n_mels < 1, n_mfcc outside its range, bank_n_bins != the frames' bins, a band with lo < 0, len < 0, lo + len > n_bins or
 * off + len > n_weights: MMK_ERR_INVALID.
 *
 * mmk_melbank_f32: in (rows, n_bins) float32, rows in_row_stride (>= n_bins) apart -> out (rows, n_mels) contiguous, or (rows, n_mfcc) with a
 * DCT.  band == NULL (with band_host, weights NULL and n_weights 0) is the DCT alone on rows that already are mel bands: n_bins == n_mels,
 * dct not NULL.  A wave stages a row in LDS; n_bins + n_mels > MMK_MELBANK_MAX_ROW: MMK_ERR_UNSUPPORTED.
 *
 * mmk_stft_mel_f32: the arguments of mmk_stft_energy_f32 and a bank for n_fft/2 + 1 bins -> out (batch, mmk_stft_n_frames(), n_mels or n_mfcc)
 * contiguous, as ONE launch: an epilogue (output mode 6) of the STFT kernels that keeps a frame's magnitudes in the transform's LDS
 * buffer; the spectrogram is never written.  The magnitudes are those of mmk_stft_mag_f32, bit for bit, so with reflect == 0 the result
 * equals mmk_melbank_f32 of mmk_stft_mag_f32's output bit for bit.  n_mels > n_fft/2: MMK_ERR_UNSUPPORTED (the bands of a frame pair
 * share that buffer); the other limits and errors are those of mmk_stft_energy_f32. */
#define MMK_MELBANK_MAX_ROW 4096
int mmk_melbank_f32(const float* in, int64_t in_row_stride, int64_t rows, int32_t n_bins, int32_t bank_n_bins, int32_t n_mels,
                    const int32_t* band_host, const int32_t* band, const float* weights, int32_t n_weights, const float* dct,
                    int32_t n_mfcc, float* out, mmk_stream_t stream);
int mmk_stft_mel_f32(const float* x, int64_t x_row_stride, int32_t batch, int64_t n_samples, int32_t n_fft, int32_t hop, int32_t center,
                     int32_t reflect, int32_t bank_n_bins, int32_t n_mels, const int32_t* band_host, const int32_t* band,
                     const float* weights, int32_t n_weights, const float* dct, int32_t n_mfcc, float* out, mmk_stream_t stream);

/* ISTFT.torch_func (mimikit/features/functionals.py:553-564):
 * torch.istft(spec^T, n_fft, hop, window=hann_window(n_fft)) with torch's defaults (center=True,
 * length=None): inverse real FFT of every frame, periodic-Hann window, overlap-add, division by the
 * overlap-added squared window, n_fft/2 samples trimmed on both sides.
 * spec: (batch, n_frames, n_fft/2+1, 2) contiguous; coordinate 0: (real, imag), 1: (abs, angle)
 * [the reference's 'pol': abs * exp(1j * angle)].  out: (batch, hop * (n_frames - 1)).
 * work: mmk_istft_workspace_floats() floats of device scratch (0 for n_fft = 1024, where it may be NULL).
 * n_fft: a power of two in [64, 4096]; 1 <= hop < n_fft; n_frames >= 2.
 * out and work need no alignment beyond that of a float: the kernels that move 16 bytes at a time are taken only when both are
 * 16-byte aligned, the element-wise forms otherwise. */
int64_t mmk_istft_n_samples(int64_t n_frames, int32_t n_fft, int32_t hop);
size_t mmk_istft_workspace_floats(int32_t batch, int64_t n_frames, int32_t n_fft);
int mmk_istft_f32(const float* spec, int32_t coordinate, int32_t batch, int64_t n_frames, int32_t n_fft,
                  int32_t hop, float* work, float* out, mmk_stream_t stream);

/* GLA.torch_func (mimikit/features/functionals.py:634-642) = torchaudio.transforms.GriffinLim(
 * n_fft, hop_length, power=1.) as published in torchaudio 2.0.1 (functional.griffinlim; the
 * reference pins that version in pyproject.toml:63-68):
 *   angles <- init;  tprev <- 0;  m = momentum / (1 + momentum)
 *   n_iter times:  inverse = istft(mag * angles);  rebuilt = stft(inverse, center, reflect)
 *                  angles = rebuilt - m * tprev;  angles /= |angles| + 1e-16;  tprev = rebuilt
 *   out = istft(mag * angles)
 * mag: (batch, n_frames, n_fft/2+1) magnitudes (time x freq, as the functional receives them).
 * init: (batch, n_frames, n_fft/2+1, 2) initial complex "angles" (torchaudio draws torch.rand of a
 * complex dtype: both parts uniform in [0, 1)), or NULL for rand_init=False (all 1 + 0i).
 * out: (batch, hop * (n_frames - 1)), which must exceed n_fft/2 (reflect padding).
 * work: mmk_gla_workspace_floats() floats of device scratch, 8-byte aligned (MMK_ERR_WORKSPACE otherwise). */
size_t mmk_gla_workspace_floats(int32_t batch, int64_t n_frames, int32_t n_fft, int32_t hop);
int mmk_gla_f32(const float* mag, const float* init, int32_t batch, int64_t n_frames, int32_t n_fft,
                int32_t hop, int32_t n_iter, float momentum, float* work, float* out, mmk_stream_t stream);

/* ------------------------------------------------------------------------
 * Building blocks (exported for unit parity tests and for host-side reuse)
 * ---------------------------------------------------------------------- */

/* floats needed to hold an (N x K) weight in MFMA fragment order */
int64_t mmk_packed_weight_floats(int32_t n_rows, int32_t k_cols);
/* W: (N, K) row-major fp32 with leading dimension ldw -> packed order */
int mmk_pack_weight_f32(const float* w, int64_t ldw, int32_t n_rows, int32_t k_cols, float* packed,
                        mmk_stream_t stream);
/* Y[M,N] = act(X[M,K] @ W^T + bias); act: an MMK_ACT_* code, 0 none, 1 tanh, 2 sigmoid, 3 mish, 4 abs, 5 relu, 6 softplus
 * (beta 1, threshold 20), 7 sin, 8 cos - any other code is MMK_ERR_INVALID (nn.Linear / 1x1 nn.Conv1d as used by modules/io.py,
 * networks/mlp.py).  bias may be NULL. */
int mmk_linear_f32(const float* x, int64_t ldx, int32_t m_rows, const float* packed_w, const float* bias,
                   int32_t n_rows, int32_t k_cols, float* y, int64_t ldy, int32_t act, mmk_stream_t stream);

/* The kernels the plans are built from, each behind its own entry point so that it can be tested alone.  W is always a packed
 * matrix of mmk_pack_weight_f32(.., n_rows, k_cols, ..); A must be 16-byte aligned with lda % 4 == 0 (MMK_ERR_UNSUPPORTED otherwise).
 *
 * C[b][M, N] = A[b][M, K] @ W^T for b < batch; A and C advance a_batch / c_batch floats per b (a_batch % 4 == 0).  The 64-row block
 * of A is staged in LDS: K up to 624 (MMK_ERR_UNSUPPORTED beyond).  An ldc % 4 != 0 stores element by element. */
int mmk_gemm_f32(const float* a, int64_t lda, int64_t a_batch, const float* packed_w, int32_t n_rows, int32_t k_cols, float* c,
                 int64_t ldc, int64_t c_batch, int32_t m_rows, int32_t batch, mmk_stream_t stream);
/* floats of the `partial` buffer mmk_gemm_bias_act_f32 needs to split K k_split ways (0: the launch's own choice; more ways than
 * the K loop has 64-column stages: one per stage); 0 when that launch does not split */
int64_t mmk_gemm_partial_floats(int32_t m_rows, int32_t n_rows, int32_t k_cols, int32_t k_split);
/* C = act(A[M, K] @ W^T + bias), M >= 128 and K >= 16 (MMK_ERR_UNSUPPORTED otherwise - there is no other kernel behind it), bias may
 * be NULL.  group > 0 scatters the rows: row m = (g, i), g = m / group, i = m % group, goes to c + g group_stride + i row_stride and
 * rows with i >= kept are not written (ldc is then unused); group == 0: rows ldc apart.  partial: NULL (K is not split) or
 * partial_floats >= mmk_gemm_partial_floats(m_rows, n_rows, k_cols, k_split) floats (MMK_ERR_WORKSPACE otherwise); k_split as
 * there.  A split launch adds its partial sums in a fixed order: the result does not depend on the run. */
int mmk_gemm_bias_act_f32(const float* a, int64_t lda, int32_t m_rows, const float* packed_w, const float* bias, int32_t n_rows,
                          int32_t k_cols, float* c, int64_t ldc, int32_t act, int32_t group, int32_t kept, int64_t group_stride,
                          int64_t row_stride, float* partial, int64_t partial_floats, int32_t k_split, mmk_stream_t stream);
/* C = act(A[M, K] @ W^T + bias) for 1 <= M <= 64 and K a multiple of 128 up to 1024 (MMK_ERR_UNSUPPORTED otherwise); bias may be NULL */
int mmk_skinny_linear_f32(const float* a, int64_t lda, int32_t m_rows, const float* packed_w, const float* bias, int32_t n_rows,
                          int32_t k_cols, float* c, int64_t ldc, int32_t act, mmk_stream_t stream);
/* Causal multi-head attention (csrc/transformer.h: TrAttnArgs): query row i < n_q of clip b at q + b q_cs + i q_ld is window
 * position q_pos0 + i and sees keys 0 .. min(q_pos0 + i, n_keys - 1); key / value row j at k / v + b kv_cs + j kv_ld; head h uses the
 * columns [h head_dim, (h + 1) head_dim) of every row; out row i at out + b o_cs + i o_ld; softmax(scale q k^T) v.
 * head_dim: a multiple of 4 in [4, 128]; q_pos0 >= 0; n_keys >= 1 (MMK_ERR_INVALID otherwise). */
int mmk_tr_attention_f32(const float* q, int64_t q_ld, int64_t q_cs, const float* k, const float* v, int64_t kv_ld, int64_t kv_cs,
                         float* out, int64_t o_ld, int64_t o_cs, int32_t n_q, int32_t q_pos0, int32_t n_keys, int32_t n_heads,
                         int32_t head_dim, float scale, int32_t batch, mmk_stream_t stream);
/* out[r] = LayerNorm(y[r] + res[r]) * w + b over d columns, biased variance, eps 1e-5; res may be NULL (no residual) and out may be
 * res (the same rows).  1 <= d <= 1024 (MMK_ERR_INVALID otherwise). */
int mmk_tr_add_ln_f32(const float* y, int64_t y_ld, const float* res, int64_t res_ld, const float* w, const float* b, float* out,
                      int64_t out_ld, int32_t rows, int32_t d, mmk_stream_t stream);

/* MLP temperature column + CategoricalSampler
 * (mimikit/networks/mlp.py:58-63, mimikit/modules/targets.py:37-52).
 * logits: (rows, n_classes + has_temp_col) raw MLP outputs, `ld` apart.
 * temperature == NULL -> argmax (first maximum on ties); otherwise one
 * temperature per row and `uniforms` (one U[0,1) per row) drive inverse-CDF
 * sampling of softmax(logits / T).  out[r * out_stride] receives the class. */
int mmk_categorical_sample_f32_i64(const float* logits, int64_t ld, int32_t rows, int32_t n_classes,
                                   int32_t has_temp_col, float min_temp, const float* temperature,
                                   const float* uniforms, int64_t* out, int64_t out_stride,
                                   mmk_stream_t stream);

/* ------------------------------------------------------------------------
 * WaveNet (mimikit/networks/wavenet_v2.py)
 * ---------------------------------------------------------------------- */
typedef struct mmk_wavenet_config {
  int32_t n_layers;                        /* sum(blocks) */
  int32_t kernel_size[MMK_MAX_LAYERS];     /* get_kernels_and_dilation :295-327 */
  int32_t dilation[MMK_MAX_LAYERS];
  int32_t q_levels;                        /* class_size of input 0 (EmbeddingIO) ; 0 -> LinearIO input */
  int32_t in_dim;                          /* feature size of input 0 when q_levels == 0 */
  int32_t dim_dilated;                     /* dims_dilated[0] */
  int32_t residuals_dim;                   /* 0 = None */
  int32_t skips_dim;                       /* 0 = None */
  int32_t n_cond;                          /* len(dims_1x1) */
  int32_t cond_in_dim[MMK_MAX_COND];       /* feature size of input 1+j (LinearIO) */
  int32_t cond_dim[MMK_MAX_COND];          /* dims_1x1[j] */
  int32_t cond_q_levels[MMK_MAX_COND];     /* > 0: input 1+j is a stream of class indices through an EmbeddingIO (no bias) of that many
                                            * classes - cond[j] of the calls below is then int64 (batch, T); 0: fp32 features through a LinearIO */
  int32_t bias;                            /* Config.bias */
  int32_t gated;                           /* act_g is not None */
  int32_t act_f, act_g;                    /* Config.act_f / act_g as MMK_ACT_* codes (act_g ignored when gated == 0).  Anything but Tanh / Sigmoid runs
                                            * on the launch path (the persistent kernels and the prefill have the default gate built in) */
  int32_t head_kind;                       /* 0: MLPIO + categorical sampler, 1: linear + Abs (magspec), 2: linear */
  int32_t mlp_hidden;                      /* MLPIO.hidden_dim */
  int32_t mlp_n_hidden;                    /* MLPIO.n_hidden_layers */
  int32_t mlp_act;                         /* MLPIO.activation of every MLP head as an MMK_ACT_* code (modules/io.py:205: Mish); anything else: the launch path */
  int32_t out_dim;                         /* q_levels of the target, or n_bins */
  int32_t learn_temp;                      /* MLP.learn_temperature */
  float min_temp;
  int32_t max_batch;
  /* reverse_layer_order (:253): the layers run in reversed construction order, so the layer built without a residual
   * convolution (:216) is no longer the last one.  res_explicit != 0: layer_has_res[l] says whether layer l (in RUN
   * order) has its conv_res; 0: every layer but the last has one when residuals_dim == dim_dilated. */
  int32_t res_explicit;
  int32_t layer_has_res[MMK_MAX_LAYERS];
  int32_t layerwise_inputs;                /* Config.layerwise_inputs: the embedded input 0 is added to every layer's output (:285-286) */
  int32_t exec_mode;                       /* how the steps of a call are run: 0 = the library chooses (a persistent kernel where the
                                            * geometry and the device allow one), 1 = one fused kernel per layer half, hipGraph-replayed -
                                            * needs no co-residency of workgroups: what a caller asks for to redo a batch after
                                            * mmk_wavenet_sync_status reported a timed-out hand-off */
  int32_t with_affine_residuals;           /* Config.with_affine_residuals (:121-122, :148-149): every layer's input goes through
                                            * x_hat * a + b of a 1x1 convolution to 3 x its width (ParametrizedLinear) first; launch path,
                                            * without pad_side, layerwise_inputs, or conditioning inputs of an ungated network */
  /* more than one target (WaveNet.forward returns one output per output module, :293; the generate loop writes output k into input k,
   * loops/generate.py:213-218): n_targets in [0, MMK_MAX_STREAMS], 0 = 1.  Target 0 is the head described above and is written to in0;
   * target k >= 1 is an MLPIO + categorical sampler of x_out_dim[k] classes on the same hidden vector, written IN PLACE to cond[k - 1],
   * which must be a class stream (cond_q_levels[k - 1] > 0).  Entry 0 of the x_ arrays is unused.  Such networks run on the launch path. */
  int32_t n_targets;
  int32_t x_out_dim[MMK_MAX_STREAMS], x_mlp_hidden[MMK_MAX_STREAMS], x_mlp_n_hidden[MMK_MAX_STREAMS], x_learn_temp[MMK_MAX_STREAMS];
  float x_min_temp[MMK_MAX_STREAMS];
  char tuning[MMK_TUNING_CHARS];           /* execution switches of THIS plan as "NAME=VALUE;NAME=VALUE" (empty: the library's choices), e.g.
                                            * "MMK_WN_SPIPE=0;MMK_WN_CHAIN=1" - what the parity tests use to put one network on every kernel that can run it.  The
                                            * library reads no environment variable (the diagnostic build, -DMMK_DIAG, falls back to it) */
} mmk_wavenet_config;

typedef struct mmk_wavenet_plan mmk_wavenet_plan;

int mmk_wavenet_plan_create(const mmk_wavenet_config* cfg, mmk_wavenet_plan** out);
void mmk_wavenet_plan_destroy(mmk_wavenet_plan* plan);
/* bind one tensor of the network's state_dict by its reference key
 * (SURVEY.md section 8(a) row a4), e.g. "layers.3.conv_dil.0.0.weight". */
int mmk_wavenet_plan_bind(mmk_wavenet_plan* plan, const char* key, const float* dev_ptr, int64_t numel);
int64_t mmk_wavenet_receptive_field(const mmk_wavenet_plan* plan); /* WaveNet.rf :337-339 */
size_t mmk_wavenet_workspace_bytes(const mmk_wavenet_plan* plan);
/* packs all bound weights into `workspace` and clears the dilation queues */
int mmk_wavenet_commit(mmk_wavenet_plan* plan, void* workspace, size_t workspace_bytes, mmk_stream_t stream);
/* Teacher-forced pass over positions [t_begin, t_end) of the inputs: fills the
 * per-layer dilation queues exactly as a full-window WaveNet.forward
 * (:276-293) over those positions would see them.  in0: int64 class indices
 * (batch, T) when q_levels > 0, else fp32 (batch, T, in_dim).  cond[j]: fp32
 * (batch, T, cond_in_dim[j]), or int64 class indices (batch, T) when cond_q_levels[j] > 0.  Strides in elements. */
int mmk_wavenet_warmup(mmk_wavenet_plan* plan, int32_t batch, const void* in0, int64_t in0_row_stride,
                       const void* const* cond, const int64_t* cond_row_stride, int64_t t_begin,
                       int64_t t_end, mmk_stream_t stream);
/* n_steps of GenerateLoopV2's hot loop (mimikit/loops/generate.py:207-219)
 * fused with WaveNet.generate_step (:447-452): for t in [t0, t0+n_steps) the
 * class drawn from the network output is written IN PLACE to in0[:, t].
 * temperature: NULL (argmax) or `batch` floats; uniforms: (batch, n_steps) - with n_targets > 1 (n_targets, batch, n_steps), and the
 * class of target k >= 1 is written IN PLACE to cond[k - 1][:, t] (the const of that argument does not cover those streams). */
int mmk_wavenet_generate(mmk_wavenet_plan* plan, int32_t batch, void* in0, int64_t in0_row_stride,
                         const void* const* cond, const int64_t* cond_row_stride, int64_t t0,
                         int64_t n_steps, const float* temperature, const float* uniforms,
                         mmk_stream_t stream);
/* raw head outputs of the most recent step: (batch, out_dim + learn_temp) fp32 */
int mmk_wavenet_last_logits(mmk_wavenet_plan* plan, int32_t batch, float* out, int64_t ld, mmk_stream_t stream);
/* the same for target k: (batch, x_out_dim[k] + x_learn_temp[k]) */
int mmk_wavenet_last_logits_of(mmk_wavenet_plan* plan, int32_t target, int32_t batch, float* out, int64_t ld, mmk_stream_t stream);
/* Measurement aid for bench.py: runs n_steps like mmk_wavenet_generate (greedy) but eagerly, with HIP
 * start/stop events attached to every fused-linear launch on `stream`; waits for completion and returns
 * summed device time (ms) and launch counts per kernel class: [0] dilated+cond+gate layer kernel,
 * [1] residual+skip layer kernel, [2] input / conditioning / head linears. */
int mmk_wavenet_profile_steps(mmk_wavenet_plan* plan, int32_t batch, void* in0, int64_t in0_row_stride,
                              const void* const* cond, const int64_t* cond_row_stride, int64_t t0,
                              int64_t n_steps, double* ms_total, int64_t* launches, mmk_stream_t stream);

/* > 0 when the plan runs all steps of a call inside one persistent kernel (1 csrc/wavenet_persist.hip, 2 wavenet_chain.hip,
 * 4 wavenet_lpipe.hip, 5 wavenet_spipe.hip, 6 wavenet_bpipe.hip; 3 was the XCD-pipelined kernel, removed in round 5: no geometry where it ran and won), 0 when it enqueues one fused kernel per layer half (hipGraph-replayed) */
int mmk_wavenet_mode(const mmk_wavenet_plan* plan);
/* 1 when the plan's last mode-5 launch streamed the clips through the stages two at a time (csrc/wavenet_spipe_pair.inc: an even number of clips,
 * 54 to 128 of them; the plan switch MMK_WN_SPIPE_PAIR=0 / 1 refuses / asks for it from 24 clips on), 0 otherwise */
int mmk_wavenet_pair_visits(const mmk_wavenet_plan* plan);
/* waits for `stream`; MMK_ERR_STATE (and the word is cleared) if a hand-off inside the persistent kernel timed out since the last call */
int mmk_wavenet_sync_status(mmk_wavenet_plan* plan, mmk_stream_t stream);
/* Fault injection for the callers' tests: marks the plan as if a hand-off of its last call had timed out, so that the next
 * mmk_wavenet_sync_status fails exactly as it would after a real time-out (and the caller's redo path runs). */
int mmk_wavenet_inject_sync_error(mmk_wavenet_plan* plan, mmk_stream_t stream);

/* ------------------------------------------------------------------------
 * SampleRNN (mimikit/networks/sample_rnn_v2.py)
 * ---------------------------------------------------------------------- */
typedef struct mmk_srnn_config {
  int32_t n_tiers;                         /* len(frame_sizes) (last tier has no RNN) */
  int32_t frame_size[MMK_MAX_TIERS];
  int32_t hidden_dim;
  int32_t rnn_kind;                        /* 0 lstm, 1 gru, 2 rnn(tanh) */
  int32_t rnn_bias;
  int32_t h0_ones;                         /* h0_init == "ones" */
  int32_t q_levels;
  int32_t mlp_hidden, mlp_n_hidden, learn_temp;
  int32_t mlp_act;                         /* MLPIO.activation of every MLP head as an MMK_ACT_* code (Mish; anything else: the kernels in turns) */
  float min_temp;
  int32_t max_batch;
  int32_t n_rnn;                           /* Config.n_rnn: stacked recurrent layers per tier (:65, nn.LSTM / GRU num_layers); 0 = 1 */
  int32_t exec_mode;                       /* 0 = the library chooses (resident mode: the bottom tier's launch beside the tier kernels of a
                                            * second stream, where they are co-resident), 1 = the kernels in turns on one stream: what a
                                            * caller asks for to redo a batch after mmk_srnn_sync_status reported a timed-out wait */
  /* more than one input / target (from_config, sample_rnn_v2.py:141-145, :160-173, :181-182): every tier's input module is a
   * ZipReduceVariables (modules/io.py:289-313) over one framed linear per input, reduced with the weights of `inputs_mode`; the bottom
   * tier's hidden vector goes through one output module per target, and the loop writes output k into input k (loops/generate.py:213-218).
   * n_inputs / n_targets in [0, MMK_MAX_STREAMS], 0 = 1, n_targets <= n_inputs.  in_class[m]: classes of input m (0: q_levels).  Target 0 is
   * the head described above; target k >= 1 an MLPIO of x_q_levels[k] classes (entry 0 of the x_ arrays is unused).  Such networks run
   * with one launch per operation (mmk_srnn_warmup_multi / mmk_srnn_generate_multi). */
  int32_t n_inputs, n_targets;
  int32_t inputs_mode;                     /* ZipMode: 0 sum, 1 mean, 2 static_mix (softmax of the bound "tiers.i.input_module.weights") */
  int32_t in_class[MMK_MAX_STREAMS];
  int32_t x_q_levels[MMK_MAX_STREAMS], x_mlp_hidden[MMK_MAX_STREAMS], x_mlp_n_hidden[MMK_MAX_STREAMS], x_learn_temp[MMK_MAX_STREAMS];
  float x_min_temp[MMK_MAX_STREAMS];
  char tuning[MMK_TUNING_CHARS];           /* execution switches of THIS plan as "NAME=VALUE;NAME=VALUE" (empty: the library's choices), e.g.
                                            * "MMK_SRNN_RESIDENT=0" - what the parity tests use to put one network on every kernel that can run it.  The
                                            * library reads no environment variable (the diagnostic build, -DMMK_DIAG, falls back to it) */
} mmk_srnn_config;

typedef struct mmk_srnn_plan mmk_srnn_plan;

int mmk_srnn_plan_create(const mmk_srnn_config* cfg, mmk_srnn_plan** out);
void mmk_srnn_plan_destroy(mmk_srnn_plan* plan);
int mmk_srnn_plan_bind(mmk_srnn_plan* plan, const char* key, const float* dev_ptr, int64_t numel);
size_t mmk_srnn_workspace_bytes(const mmk_srnn_plan* plan);
int mmk_srnn_commit(mmk_srnn_plan* plan, void* workspace, size_t workspace_bytes, mmk_stream_t stream);
/* SampleRNN.reset_hidden (:266-268) */
int mmk_srnn_reset(mmk_srnn_plan* plan, mmk_stream_t stream);
/* SampleRNN.before_generate warm-up (:226-234): runs the tier schedule for
 * t in [rf, prompt_len - prompt_len % rf) on windows shifted by prompt_len % rf */
int mmk_srnn_warmup(mmk_srnn_plan* plan, int32_t batch, const int64_t* idx, int64_t idx_row_stride,
                    int64_t prompt_len, mmk_stream_t stream);
/* n_steps of the generate loop fused with SampleRNN.generate_step (:236-260) */
int mmk_srnn_generate(mmk_srnn_plan* plan, int32_t batch, int64_t* idx, int64_t idx_row_stride, int64_t t0,
                      int64_t n_steps, const float* temperature, const float* uniforms, mmk_stream_t stream);
int mmk_srnn_last_logits(mmk_srnn_plan* plan, int32_t batch, float* out, int64_t ld, mmk_stream_t stream);
/* the same calls for n_inputs class streams: idx[m] / idx_row_stride[m] for m < n_inputs; the class of target k is written IN PLACE to
 * idx[k][:, t]; uniforms: (n_targets, batch, n_steps).  With one input they are the calls above. */
int mmk_srnn_warmup_multi(mmk_srnn_plan* plan, int32_t batch, const int64_t* const* idx, const int64_t* idx_row_stride,
                          int64_t prompt_len, mmk_stream_t stream);
int mmk_srnn_generate_multi(mmk_srnn_plan* plan, int32_t batch, int64_t* const* idx, const int64_t* idx_row_stride, int64_t t0,
                            int64_t n_steps, const float* temperature, const float* uniforms, mmk_stream_t stream);
int mmk_srnn_last_logits_of(mmk_srnn_plan* plan, int32_t target, int32_t batch, float* out, int64_t ld, mmk_stream_t stream);
/* waits for the stream; fails (and clears the word) if a wait inside the tier / bottom kernels timed out since the last call -
 * the samples of that generation are invalid */
int mmk_srnn_sync_status(mmk_srnn_plan* plan, mmk_stream_t stream);
/* fault injection for the callers' tests: the next mmk_srnn_sync_status reports a timed-out wait (once) */
int mmk_srnn_inject_sync_error(mmk_srnn_plan* plan, mmk_stream_t stream);
/* diagnostic: generate blocks this plan has run in resident mode (the bottom tier as one launch beside the tier kernels of a
 * second stream) since it was created; tests assert that the mode they mean to cover is the one that ran */
int64_t mmk_srnn_resident_blocks(const mmk_srnn_plan* plan);
/* diagnostic: warm-ups (mmk_srnn_warmup: SampleRNN.before_generate, sample_rnn_v2.py:226-234) this plan has run as ONE teacher-forced resident launch - the
 * tiers with their matrices in registers, windows from the prompt, no bottom tier - instead of one launch per tier update */
int64_t mmk_srnn_resident_warmups(const mmk_srnn_plan* plan);
/* diagnostic: what the bottom tier and the head of the most recent steps outside resident mode were emitted as - 0 nothing yet,
 * 1 the fused kernel with one clip per workgroup, 2 the fused kernel with four clips per workgroup (MFMA), 3 one launch per op
 * (the draw is the stand-alone sampler); tests assert that the class picker they mean to cover is the one that ran */
int32_t mmk_srnn_bottom_kernel(const mmk_srnn_plan* plan);

/* ------------------------------------------------------------------------
 * Seq2SeqLSTMNetwork (mimikit/networks/s2s_lstm_v2.py)
 * ---------------------------------------------------------------------- */
typedef struct mmk_s2s_config {
  int32_t in_dim;                          /* n_bins of the magspec input */
  int32_t out_dim;                         /* n_bins of the target */
  int32_t model_dim;
  int32_t hop;
  int32_t enc_n_lstm, dec_n_lstm;          /* bi-LSTM layers per side (1 .. 8) */
  int32_t out_abs;                         /* output activation Abs */
  int32_t max_batch;
  int32_t enc_downsampling;                /* 0 edge_sum, 1 edge_mean, 2 sum, 3 mean  (s2s_lstm_v2.py:105-113) */
  int32_t dec_upsampling;                  /* 0 linear_resample, 1 repeat             (:158-163) */
  int32_t enc_apply_residuals;             /* x = x + y from the second encoder layer on (:101-104) */
  int32_t dec_apply_residuals;             /* x = x + y after every decoder layer       (:175-178) */
  /* discrete IO (IOSpec.mulaw_io with an embedding input, tests/test_seq2seq.py:149-154): */
  int32_t in_classes;                      /* > 0: inputs are class indices through nn.Embedding(in_classes, model_dim)
                                              under ZipReduceVariables (:205-210); in_dim must equal model_dim */
  int32_t head_kind;                       /* 0: Linear [+ Abs] to out_dim bins; 1: MLP (networks/mlp.py:42-63) over out_dim
                                              classes, then the argmax of CategoricalSampler (modules/targets.py:43-44) */
  int32_t mlp_hidden, mlp_n_hidden;        /* head_kind 1: width, number of extra hidden blocks (0 .. 4) */
  int32_t mlp_act;                         /* head_kind 1: MLPIO.activation as an MMK_ACT_* code (Mish) */
  int32_t learn_temp;                      /* head_kind 1: one more output, logits / max(sigmoid(it), min_temp) */
  float min_temp;
  int32_t exec_mode;                       /* 0 = the library chooses (one resident launch per bi-LSTM layer where its workgroups are
                                            * co-resident), 1 = one launch per frame: what a caller asks for to redo a call after
                                            * mmk_s2s_sync_status reported a timed-out wait */
  char tuning[MMK_TUNING_CHARS];           /* execution switches of THIS plan as "NAME=VALUE;NAME=VALUE" (empty: the library's choices), e.g.
                                            * "MMK_S2S_SEQ=0" - what the parity tests use to put one network on every kernel that can run it.  The
                                            * library reads no environment variable (the diagnostic build, -DMMK_DIAG, falls back to it) */
} mmk_s2s_config;

typedef struct mmk_s2s_plan mmk_s2s_plan;

int mmk_s2s_plan_create(const mmk_s2s_config* cfg, mmk_s2s_plan** out);
void mmk_s2s_plan_destroy(mmk_s2s_plan* plan);
int mmk_s2s_plan_bind(mmk_s2s_plan* plan, const char* key, const float* dev_ptr, int64_t numel);
size_t mmk_s2s_workspace_bytes(const mmk_s2s_plan* plan);
int mmk_s2s_commit(mmk_s2s_plan* plan, void* workspace, size_t workspace_bytes, mmk_stream_t stream);
/* Seq2SeqLSTMNetwork.generate_step == forward (:246-266): x (batch, hop, in_dim)
 * -> y (batch, hop, out_dim).  Row strides are per frame, batch strides per clip. */
int mmk_s2s_step(mmk_s2s_plan* plan, int32_t batch, const float* x, int64_t x_batch_stride,
                 int64_t x_frame_stride, float* y, int64_t y_batch_stride, int64_t y_frame_stride,
                 mmk_stream_t stream);
/* n_calls successive generate_steps on one (batch, T, n_bins) tensor, in place:
 * call i reads frames [t0 + i*hop - hop, t0 + i*hop) and writes up to hop
 * frames at t0 + i*hop (clipped at t_total), as loops/generate.py:207-219 does. */
int mmk_s2s_generate(mmk_s2s_plan* plan, int32_t batch, float* frames, int64_t batch_stride,
                     int64_t frame_stride, int64_t t0, int64_t n_steps, int64_t t_total, mmk_stream_t stream);

/* The same two calls for a plan with in_classes > 0 and head_kind 1: x / y / classes hold int64 class indices, one per
 * (clip, position); generate_step hands the sampler no temperature (s2s_lstm_v2.py:262-263), so every class is an argmax. */
int mmk_s2s_step_classes(mmk_s2s_plan* plan, int32_t batch, const int64_t* x, int64_t x_batch_stride,
                         int64_t x_elem_stride, int64_t* y, int64_t y_batch_stride, int64_t y_elem_stride,
                         mmk_stream_t stream);
int mmk_s2s_generate_classes(mmk_s2s_plan* plan, int32_t batch, int64_t* classes, int64_t batch_stride,
                             int64_t elem_stride, int64_t t0, int64_t n_steps, int64_t t_total, mmk_stream_t stream);
/* the MLP head's outputs (before the learned-temperature division) of the last step: (batch * hop, out_dim + learn_temp)
 * rows (clip-major) copied to `out` with leading dimension out_ld - what the parity tests compare with the oracle's */
int mmk_s2s_last_logits(mmk_s2s_plan* plan, int32_t batch, float* out, int64_t out_ld, mmk_stream_t stream);
/* waits for the stream; fails (and clears the word) if a wait inside the resident bi-LSTM kernel (csrc/lstm_seq.hip) timed out
 * since the last call - the outputs of the calls in between are invalid */
int mmk_s2s_sync_status(mmk_s2s_plan* plan, mmk_stream_t stream);
/* fault injection for the callers' tests: the next mmk_s2s_sync_status reports a timed-out wait (once) */
int mmk_s2s_inject_sync_error(mmk_s2s_plan* plan, mmk_stream_t stream);
/* diagnostic: bi-LSTM layers this plan has run as ONE resident launch since it was created */
int64_t mmk_s2s_resident_launches(const mmk_s2s_plan* plan);

/* ------------------------------------------------------------------------
 * SimpleTransformer (mimikit/networks/transformers.py:70-178)
 *
 * One step recomputes the whole rf-long window as the reference does: X0 = input(x[t-rf:t]) + pe[0:rf], then num_layers post-norm
 * nn.TransformerDecoderLayer blocks (causal self-attention, causal cross-attention with memory = X0, ReLU feed-forward, LayerNorm
 * eps 1e-5), the optional final LayerNorm and the head on the last position only.  There is no state between steps: the positional
 * encoding is tied to window positions, so every key changes at every step.
 * ---------------------------------------------------------------------- */
typedef struct mmk_tr_config {
  int32_t model_dim;                       /* D: multiple of 16, 16 .. 1024 */
  int32_t n_heads;                         /* head_dim = D / n_heads: multiple of 4, up to 128 */
  int32_t feedforward_dim;                 /* 1 .. 4096 */
  int32_t num_layers;                      /* 1 .. 16 */
  int32_t rf;                              /* window length, 1 .. 2048 (the reference's positional-encoding length) */
  int32_t final_norm;                      /* with_layer_norm: model.norm after the last layer */
  int32_t in_kind;                         /* 0: class indices through nn.Embedding(in_classes, D); 1: frames of in_dim bins through Linear(in_dim, D) */
  int32_t in_classes;
  int32_t in_dim;
  int32_t head_kind;                       /* 0: MLP (networks/mlp.py) + CategoricalSampler over out_dim classes; 1: Linear to out_dim bins [+ Abs] */
  int32_t out_dim;
  int32_t out_abs;                         /* head_kind 1: Abs after the Linear (IOSpec.magspec_io) */
  int32_t mlp_hidden, mlp_n_hidden;        /* head_kind 0: width, number of extra hidden blocks (0 .. 4) */
  int32_t mlp_act;                         /* head_kind 0: MMK_ACT_* code of MLPIO.activation */
  int32_t learn_temp;                      /* head_kind 0: one more output, logits / max(sigmoid(it), min_temp) */
  float min_temp;
  int32_t max_batch;                       /* 1 .. 512 clips */
  char tuning[MMK_TUNING_CHARS];           /* execution switches of THIS plan as "NAME=VALUE;..." (none are defined for this plan yet) */
} mmk_tr_config;

typedef struct mmk_tr_plan mmk_tr_plan;

/* -1 with the offending field named in mmk_last_error for geometry outside the table above, -3 for IO options outside the coverage */
int mmk_tr_plan_create(const mmk_tr_config* cfg, mmk_tr_plan** out);
void mmk_tr_plan_destroy(mmk_tr_plan* plan);
/* state_dict tensors by the reference's key names (model.layers.{l}.self_attn.in_proj_weight, ..., pe.pe as stored: (2048, 1, D)) */
int mmk_tr_plan_bind(mmk_tr_plan* plan, const char* key, const float* dev_ptr, int64_t numel);
size_t mmk_tr_workspace_bytes(const mmk_tr_plan* plan);
int mmk_tr_commit(mmk_tr_plan* plan, void* workspace, size_t workspace_bytes, mmk_stream_t stream);
/* SimpleTransformer.generate_step == eval forward (:159-178) on one window: x holds rf positions per clip (int64 classes, or fp32
 * frames of in_dim bins with unit stride along the bins), `time_stride` elements apart, `batch_stride` between clips.  y receives one
 * position per clip (a class, or out_dim bins), `y_batch_stride` apart.  temperature == NULL: argmax; else one temperature and one
 * uniform per clip (uniforms[clip]) drive the inverse-CDF draw of mmk_categorical_sample_f32_i64. */
int mmk_tr_step(mmk_tr_plan* plan, int32_t batch, const void* x, int64_t x_batch_stride, int64_t x_time_stride, void* y,
                int64_t y_batch_stride, const float* temperature, const float* uniforms, mmk_stream_t stream);
/* n_steps successive steps in place on the loop's (batch, T[, in_dim]) tensor: step t reads positions [t - rf, t) and writes position t,
 * t = t0 .. t0 + n_steps - 1 (t0 >= rf; class tensors need time_stride 1).  uniforms: (batch, n_steps) row-major, column = step. */
int mmk_tr_generate(mmk_tr_plan* plan, int32_t batch, void* data, int64_t batch_stride, int64_t time_stride, int64_t t0, int64_t n_steps,
                    const float* temperature, const float* uniforms, mmk_stream_t stream);
/* head_kind 0: the MLP's raw outputs of the last step, (batch, out_dim + learn_temp) rows copied to `out` with leading dimension out_ld */
int mmk_tr_last_logits(mmk_tr_plan* plan, int32_t batch, float* out, int64_t out_ld, mmk_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* MMK_H_ */
