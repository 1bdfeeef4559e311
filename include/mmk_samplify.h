/* libmmk_hip: the quadratic spline and the onset-cut kernels of Samplifyer (csrc/samplify.hip, csrc/spline2.h;
 * mimikit_amd/extract/samplify.py).
 *
 * A header of its own beside mmk.h, whose conventions hold here unchanged: raw device pointers and strides in ELEMENTS, every call
 * enqueues on `stream` and returns without waiting for it, 0 = MMK_OK or a negative MMK_ERR_* with the text in mmk_last_error().
 * MMK_ABI_VERSION does not change: these are additions, and the binding types them from a table of its own (native.SAMPLIFY_SYMBOLS).
 *
 * The spline is scipy.interpolate.interp1d(np.arange(n), y, kind="quadratic"): make_interp_spline(k = 2) with not-a-knot ends, knots
 * [0, 0, 0, 1.5, 2.5, ..., n - 2.5, n - 1, n - 1, n - 1], B-spline coefficients c (n float64 per row).  A value of it "at sample i of T" is
 *     fl32( s( linspace(0, n - 1, T)[i] ) ),    linspace as numpy makes it: i * ((n - 1) / (T - 1)) in float64, the last position forced to n - 1,
 * the basis from de Boor's recurrence in float64, three products and two sums, ONE rounding to float32 - computed by one __device__
 * function wherever it is needed, so that the eval kernel, the period kernels and the cut kernels see the same bits.  No kernel here
 * but mmk_spline2_eval_f32 writes a T-long float array.
 *
 * Common to the entry points:
 *   - float data needs 4-byte alignment, float64 / int64 data 8-byte; tails are masked in the kernels, the caller pads nothing; nothing
 *     but the stated outputs and the workspace is written;
 *   - no atomics, no workgroup waits for another, every list is ordered by prefix counts and every reduction has one order: two calls
 *     give the same bits.  NaN is not handled;
 *   - no entry point waits for its stream or allocates; each can be captured into a graph.
 */
#ifndef MMK_SAMPLIFY_H_
#define MMK_SAMPLIFY_H_

#include "mmk.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MMK_SPLINE2_TILE 256         /* knots one workgroup of the coefficient kernel owns */
#define MMK_SPLINE2_HALO 32          /* knots on either side that a coefficient is solved from: the influence of y[i +- h] on c[i] is 0.1716^h */
#define MMK_SPLINE2_EVAL_TILE 256    /* outputs one workgroup of the evaluation kernel writes per step */
#define MMK_PERIODS_TILE 1024        /* samples one workgroup of the period kernels owns */
#define MMK_SAMPLIFY_MAX_LEVELS 6    /* the reference's default has six */
#define MMK_SAMPLIFY_MAX_WINDOW 2000 /* the reference's half window of the left / right test */
#define MMK_SAMPLIFY_GROUP 256       /* lanes that share one cut: samples of a window or a refine range taken per step */

/* The coefficients of the spline through (j, y[j]), j = 0 .. n - 1, of every row: y (batch, n) float32, y_row_stride >= 0 floats apart;
 * coef (batch, n) float64, coef_row_stride >= n apart.  The collocation rows are made from the knot vector by the evaluation's own basis
 * function (tridiagonal; rows 0 and n - 1 are the identity); c[i] is solved from the rows i - MMK_SPLINE2_HALO .. i + MMK_SPLINE2_HALO
 * alone, by elimination from both ends of that window towards i: what lies beyond moves c[i] by less than 1e-23 of the largest |y|.
 * n < 3 (scipy refuses n = 2): MMK_ERR_INVALID.  batch > 65535: MMK_ERR_UNSUPPORTED. */
int mmk_spline2_coef_f64(const float* y, int64_t y_row_stride, int32_t batch, int64_t n, double* coef, int64_t coef_row_stride,
                         mmk_stream_t stream);

/* out[r, i] = the spline of row r at sample i of n_out (above); coef (batch, n) float64 coef_row_stride >= 0 apart, out (batch, n_out)
 * float32 out_row_stride >= n_out apart.  n_out = 1 gives position 0.  n < 3 or n_out < 1: MMK_ERR_INVALID. */
int mmk_spline2_eval_f32(const double* coef, int64_t coef_row_stride, int32_t batch, int64_t n, float* out, int64_t out_row_stride,
                         int64_t n_out, mmk_stream_t stream);

/* The reference's attack_decay (mimikit/extract/samplify.py:56-70) on g[i] = the spline `coef` (n knots) at sample i of n_samples, or, with
 * coef = NULL, on g = `row`, n_samples float32 as they are (exactly one of coef and row is given; n is not read with a row):
 *     attacks  a:  g[a - 1] < 0 and g[a] > 0                                  (1 <= a <= n_samples - 1)
 *     peaks    p:  g[p] > 0 and g[p + 1] < 0                                  (0 <= p <= n_samples - 2)
 *     dec(a)    :  the first peak p >= a if p <= b - 2, else n_samples - 1;   b = the next attack, n_samples - 1 after the last one
 * in two calls, because the lists are sized by their counts and not by a guess:
 *   mmk_periods_count_i64  counts[0] = the number of attacks, counts[1] = the number of peaks (device int64[2]); `work` keeps every tile's
 *                          offsets into the two lists (mmk_periods_workspace_bytes(n_samples) bytes, 8-byte aligned);
 *   mmk_periods_fill_i64   with the SAME coef, n, row, n_samples and work, and n_att / n_peak as read from counts: att (n_att), peaks (n_peak)
 *                          rising, dec (n_att).  An index past the stated counts is not written.  n_att = 0 writes nothing.
 * The spline is evaluated in both calls; its values are never written.  n < 3 or n_samples < 1: MMK_ERR_INVALID; a workspace too small: MMK_ERR_WORKSPACE. */
size_t mmk_periods_workspace_bytes(int64_t n_samples);
int mmk_periods_count_i64(const double* coef, int64_t n, const float* row, int64_t n_samples, int64_t* counts, void* work, size_t work_bytes,
                          mmk_stream_t stream);
int mmk_periods_fill_i64(const double* coef, int64_t n, const float* row, int64_t n_samples, const void* work, size_t work_bytes, int64_t n_att,
                         int64_t n_peak, int64_t* att, int64_t* dec, int64_t* peaks, mmk_stream_t stream);

/* Samplifyer.fit II: for every attack k < count, with ce = the envelope spline `env_coef` (n knots) at the n_samples positions,
 *     env_att[k] = ce[att[k]], env_dec[k] = ce[dec[k]], scores[k] = fl32(env_dec[k] - env_att[k]), keep[k] = scores[k] > sensitivity (0 / 1).
 * An index outside [0, n_samples) gives NaN and keep = 0.  count = 0 is legal and launches nothing. */
int mmk_samplify_scores_f32(const double* env_coef, int64_t n, int64_t n_samples, const int64_t* att, const int64_t* dec, int64_t count,
                            float sensitivity, float* scores, float* env_att, float* env_dec, uint8_t* keep, mmk_stream_t stream);

/* Samplifyer.fit III (left_right_scores, _refine, refine_cuts) for every kept attack k < count, one workgroup each.  env_coef / grad_coef /
 * n_knots are HOST arrays of `levels` entries (1 <= levels <= MMK_SAMPLIFY_MAX_LEVELS): the device pointers to the levels' coefficient rows
 * and their knot counts, level 0 the coarse one.  e_l, g_l = the float32 spline values of level l at the n_samples positions; y (n_samples) the signal.
 *   side    w = min(peak - cut, MMK_SAMPLIFY_MAX_WINDOW); left = max over [max(c - w, 0), c), right = max over [c, min(c + w, n_samples)) of
 *           fl32(e_0[i] - e_last[i]), an empty window is -inf; side = 0 if left >= right else 1.  (levels = 1: e_last = e_0.)
 *           lr_scores (count, 2) float32 or NULL receives (left, right).
 *   refine  side 0: the reference sets d = c; c = c - (d - c), which leaves c where it is with an empty range - a left-side cut is only
 *           snapped.  side 1: for l = 1 .. levels - 1 on [c, d), d = peak at first, while c != d:
 *               s = first argmin of 0.9 * double(e_l[i]) + 0.1 * (1.0 - double(g_l[i]))      (float64, every operation rounded, no fma)
 *               s = s - c;  s = s < d - 1 ? s : 0      (the RELATIVE s against the ABSOLUTE d - 1, as the reference does)
 *               m = first argmax of e_l[i], minus c;   c, d = c + s, max(c + m, c + s)
 *   snap    z[0] = true, z[i] = signbit(y[i]) != signbit(y[i - 1]) (librosa.zero_crossings with pad = True, WITHOUT its clipping of
 *           |y| <= 1e-10 to zero); before = c, after = c + 1 walk outwards until either is a crossing, before preferred; where `after`
 *           leaves the signal (the reference reads z[n_samples] there) the walk goes on to the left alone, and z[0] ends it.
 * sides and cuts: count int64.  A pair outside 0 <= cut <= peak <= n_samples - 1 gives side = cut = -1 (and NaN scores).  count = 0 is legal. */
int mmk_samplify_cuts_i64(const float* y, int64_t n_samples, const double* const* env_coef, const double* const* grad_coef,
                          const int64_t* n_knots, int32_t levels, const int64_t* coarse_cuts, const int64_t* coarse_peaks, int64_t count,
                          int64_t* sides, float* lr_scores, int64_t* cuts, mmk_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* MMK_SAMPLIFY_H_ */
