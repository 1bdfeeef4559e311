/* libmmk_hip: the nearest-neighbour filter's entry point (csrc/nn_filter.hip; mimikit_amd/features/functionals.py NearestNeighborFilter).
 *
 * A header of its own beside mmk.h, whose conventions hold here unchanged: raw device pointers and strides in ELEMENTS, every call
 * enqueues on `stream` and returns without waiting for it, 0 = MMK_OK or a negative MMK_ERR_* with the text in mmk_last_error().
 * MMK_ABI_VERSION does not change: this is an addition, and the binding types it from a table of its own (native.NN_FILTER_SYMBOLS).
 *
 *   - x is n rows of d floats, x_row_stride >= 0 floats apart; out is n rows of d floats, out_row_stride >= d floats apart; float data
 *     needs 4-byte alignment only, int64 data 8-byte;
 *   - tails are masked in the kernel, the caller pads nothing; nothing but `out` and `count` is written;
 *   - one launch, no workspace, no atomics, no workgroup waits for another; a selection has no order of operations and the mean has one
 *     that depends on the list alone, so two calls give the same bits.  NaN in x is not handled; -0 and +0 are equal values, and which
 *     of the two a selection returns is not specified.
 */
#ifndef MMK_NN_FILTER_H_
#define MMK_NN_FILTER_H_

#include "mmk.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MMK_NN_AGG_MEDIAN 0 /* numpy.median: the middle value, or fl32(fl32(a + b) / 2) of the two middle values of an even count */
#define MMK_NN_AGG_MEAN 1   /* the float64 sum in rising slot order, divided in float64, rounded to float32 once (mmk_segment_mean_f32's rule) */
#define MMK_NN_AGG_MAX 2    /* numpy.max */
#define MMK_NN_AGG_MIN 3    /* numpy.min */

/* Every row replaced by an aggregate of its neighbours' rows (librosa.decompose.nn_filter behind a k-nearest search).
 *   index   (n, t) contiguous int64, as mmk_nn_topk_f32 writes it, 1 <= t <= MMK_NN_TOPK_MAX.  A slot is EMPTY if its value lies outside
 *           [0, n) or is its own row number (mmk_nn_topk_f32 writes -1 past the last candidate); no address is formed from an empty slot.
 *           The neighbours of row i are the non-empty j = index[i, p], one per slot: a row named by two slots counts twice.
 *   mutual  != 0: j counts only if some slot of row j holds i (the `sym=True` of librosa's recurrence matrix).
 *   op      MMK_NN_AGG_*:  out[i, b] = op over the neighbours j of x[j, b];  a row without a neighbour keeps its values, out[i] = x[i].
 *           The selections (median, max, min) return bits of x, or the one rounded sum and halving above; subnormals are not flushed.
 *   count   n int32 or NULL: the number of neighbours of every row.
 * `out` must not alias `x`: a row is read by the workgroups of its neighbours while its own workgroup writes it.
 * Any other op, or t > MMK_NN_TOPK_MAX: MMK_ERR_UNSUPPORTED.  Nothing of size n x t x d exists anywhere: a wave holds the at most 16
 * values of a bin in registers. */
int mmk_nn_aggregate_f32(const float* x, int64_t x_row_stride, int64_t n, int32_t d, const int64_t* index, int32_t t, int32_t mutual,
                         int32_t op, float* out, int64_t out_row_stride, int32_t* count, mmk_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* MMK_NN_FILTER_H_ */
