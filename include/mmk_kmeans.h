/* libmmk_hip: the k-means entry points (csrc/kmeans.hip; mimikit_amd/extract/clusters.py KMeans).
 *
 * A header of its own beside mmk.h, whose conventions hold here unchanged: raw device pointers and strides in ELEMENTS, every call
 * enqueues on `stream` and returns without waiting for it, 0 = MMK_OK or a negative MMK_ERR_* with the text in mmk_last_error().
 * MMK_ABI_VERSION does not change: these are additions, and the binding types them from a table of its own (native.KMEANS_SYMBOLS).
 * (The prototypes move into mmk.h, and their stream cases into the shared table of tests/stream_cases.py, in a later change.)
 *
 * Common to the three kernels:
 *   - x is n rows of d floats, x_row_stride >= 0 floats apart; float data needs 4-byte alignment only, float64 / int64 data 8-byte;
 *   - `offset` is d floats or NULL: every kernel works on x' = fl32(x - offset), subtracted while loading (NULL: x' = x); the centred
 *     corpus is never written.  `centres` are in the coordinates of x' (nothing is subtracted from them);
 *   - tails are masked in the kernel, the caller pads nothing; nothing but the stated outputs and the workspace is written;
 *   - no floating-point atomics, no workgroup waits for another; every sum has one order that depends on the sizes alone, so two
 *     calls give the same bits.  NaN and inf in the inputs are not handled.
 */
#ifndef MMK_KMEANS_H_
#define MMK_KMEANS_H_

#include "mmk.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MMK_KMEANS_MAX_K 256        /* centres of one assignment: the widest centre tile */
#define MMK_KMEANS_PP_MAX_TRIALS 8  /* candidate rows of one seeding step */
#define MMK_KMEANS_MAX_SLABS 1024   /* the fixed partition of the rows that the float64 sums are taken over */

/* The nearest centre of every row.
 *     key[r, j] = <x'_r, c_j> + shift[j],    shift = mmk_half_neg_sqnorm_f32 of the centres: the largest key is the smallest |x'_r - c_j|^2
 * The sum over d runs on v_mfma_f32_32x32x2_f32 in one order that does not depend on where a row or a centre sits in its tile (two
 * identical rows get the same bits, two identical centres tie); the shift is added with one more rounding.
 *   labels  n int32, IN/OUT: on return the FIRST j with the largest key
 *   key     n floats or NULL: that key
 *   changed one int64 or NULL: incremented (an integer atomic) once for every row whose new label differs from the value found in `labels`
 * 1 <= k <= MMK_KMEANS_MAX_K, beyond it MMK_ERR_UNSUPPORTED.  One launch, no workspace; nothing of size n x k exists anywhere. */
int mmk_kmeans_assign_f32(const float* x, int64_t x_row_stride, const float* offset, int64_t n, int32_t d, const float* centres,
                          int64_t c_row_stride, const float* shift, int32_t k, int32_t* labels, float* key, int64_t* changed,
                          mmk_stream_t stream);

/* The float64 sum and the count of every label's rows.
 *     sums[j][:] = the sum of x'_r over the rows with labels[r] == j  (k x d float64, contiguous),   counts[j] int64
 * A label outside [0, k) leaves its row out.  No sort, no gather: the rows are read once, in order, in at most MMK_KMEANS_MAX_SLABS
 * slabs of consecutive rows; a slab is added in rising row order, the slabs' partial sums in rising slab order.  The workspace holds
 * the partials; mmk_kmeans_label_sums_workspace_bytes(n, d, k) does not grow with n beyond that number of slabs (0: bad sizes).
 * Where `centres` is not NULL (k rows, c_row_stride apart) a second pass also writes
 *     row_d2[r] = |x'_r - c_labels[r]|^2  (n float64, or NULL)   and   *inertia = their sum  (float64, or NULL),
 * the squares of the float64 differences added in one fixed order (0 for a row whose label is outside [0, k)).
 * k >= 1 is not limited by MMK_KMEANS_MAX_K, but a wave keeps one float64 sum and one count per label in LDS: beyond 3750 labels
 * MMK_ERR_UNSUPPORTED.  MMK_ERR_WORKSPACE: the workspace is NULL, smaller than that or not 8-byte aligned. */
size_t mmk_kmeans_label_sums_workspace_bytes(int64_t n, int32_t d, int32_t k);
int mmk_kmeans_label_sums_f64(const float* x, int64_t x_row_stride, const float* offset, int64_t n, int32_t d, const int32_t* labels,
                              int32_t k, double* sums, int64_t* counts, const float* centres, int64_t c_row_stride, double* row_d2,
                              double* inertia, void* workspace, size_t workspace_bytes, mmk_stream_t stream);

/* One step of k-means++ seeding over t candidate rows cand[0 .. t) (int64 row numbers in [0, n), on the device):
 *     m_i[r] = min(closest[r], |x'_r - x'_cand[i]|^2),   pot_i = the sum of m_i over r;   the FIRST i with the smallest pot_i wins:
 *     closest <- m_i (n float64, IN/OUT),   *pot <- pot_i (float64),   *chosen <- cand[i] (int64)
 * The differences of two floats are exact in float64; their squares are added in one fixed order, the rows in the fixed slabs.  With
 * closest = +inf and t = 1 this is the initialisation from the first centre.  A candidate outside [0, n) is read as row n - 1 (and
 * reported as given).  1 <= t <= MMK_KMEANS_PP_MAX_TRIALS, beyond it MMK_ERR_UNSUPPORTED.  The workspace
 * (mmk_kmeans_pp_step_workspace_bytes(), a constant) holds the slabs' partial pots. */
size_t mmk_kmeans_pp_step_workspace_bytes(void);
int mmk_kmeans_pp_step_f64(const float* x, int64_t x_row_stride, const float* offset, int64_t n, int32_t d, const int64_t* cand, int32_t t,
                           double* closest, double* pot, int64_t* chosen, void* workspace, size_t workspace_bytes, mmk_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* MMK_KMEANS_H_ */
