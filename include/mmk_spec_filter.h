/* libmmk_hip: the two harmonic spectrogram filters' entry points (csrc/spec_filter.hip; mimikit_amd/features/functionals.py AutoConvolve,
 * F0Filter).
 *
 * A header of its own beside mmk.h, whose conventions hold here unchanged: raw device pointers and strides in ELEMENTS, every byte offset
 * is formed in 64 bits, every call enqueues on `stream` and returns without waiting for it, 0 = MMK_OK or a negative MMK_ERR_* with the
 * text in mmk_last_error().  MMK_ABI_VERSION does not change: these are additions, and the binding types them from a table of its own
 * (native.SPEC_FILTER_SYMBOLS).
 *
 * Both take `batch` clips of `frames` frames of `bins` non-negative float32 magnitudes, bins contiguous: frame t of clip c begins at
 * s + c * s_batch_stride + t * s_row_stride, and the same frame of the result at out + c * out_batch_stride + t * out_row_stride.
 *   - float data needs 4-byte alignment only; tails are masked in the kernel, the caller pads nothing; nothing but the frames of `out`
 *     is written (the elements between two rows of out stay as they were);
 *   - one launch, no workspace, no atomics, no workgroup waits for another.  A frame's weights are computed and summed in float64 in an
 *     order that depends on `bins` alone and the result is rounded to float32 once: the same frame gives the same bits at any `frames`,
 *     any `batch` and any place in the batch (for mmk_auto_convolve_f32: the same frame with the same neighbours inside its clip);
 *   - `out` must not overlap `s`: a frame of s is read by the workgroups of its neighbours while its own is written;
 *   - NaN, negative or infinite bins are not looked for; their results are unspecified (nothing outside `out` is written for them).
 *
 * MMK_ERR_INVALID: a null pointer; batch, frames < 1; bins < 2; window < 2; n_overtone or n_undertone < 0; s_row_stride or s_batch_stride
 *   < 0 or out_row_stride or out_batch_stride < bins where there is more than one row or clip; a pointer that is not 4-byte aligned;
 *   out == s.
 * MMK_ERR_UNSUPPORTED: bins > MMK_SPEC_FILTER_MAX_BINS; window > MMK_AUTO_CONVOLVE_MAX_WINDOW; n_overtone > MMK_F0_FILTER_MAX_OVERTONE;
 *   n_undertone > MMK_F0_FILTER_MAX_UNDERTONE; more frames than one launch takes (2^31 - 1 workgroups of MMK_SPEC_FILTER_TILE_FRAMES).
 */
#ifndef MMK_SPEC_FILTER_H_
#define MMK_SPEC_FILTER_H_

#include "mmk.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MMK_SPEC_FILTER_MAX_BINS 4097       /* n_fft = 8192: a frame and its float64 weights lie in a workgroup's LDS (48 KiB) */
#define MMK_SPEC_FILTER_TILE_FRAMES 4       /* consecutive frames of one clip that a workgroup filters one after the other */
#define MMK_AUTO_CONVOLVE_MAX_WINDOW 64     /* every frame re-reads `window` rows from cache */
#define MMK_F0_FILTER_MAX_OVERTONE 16
#define MMK_F0_FILTER_MAX_UNDERTONE 16

/* The reference's AutoConvolve(window_size = window) (mimikit/features/functionals.py:1007-1036).  With k = window, for frame t and bin b:
 *   p    = the float64 product of s[u, b] over the frames u = t - k/2 ... t - k/2 + k - 1 of the SAME clip, in rising u; a frame outside
 *          [0, frames) counts as 1 (even k: the lopsided window this gives; k = 2 is frames t - 1, t)
 *   z    = log(1.0 + p)  - the rounded sum, not log1p
 *   out  = fl32( z / (sum_b z + 1e-8) * s[t, b] ) */
int mmk_auto_convolve_f32(const float* s, int64_t s_batch_stride, int64_t s_row_stride, int32_t batch, int32_t frames, int32_t bins,
                          int32_t window, float* out, int64_t out_batch_stride, int64_t out_row_stride, mmk_stream_t stream);

/* The reference's F0Filter (:1039-1080) on a uniform frequency grid, where harmonic h of bin b sits at bin position h * b.  For a frame z:
 *   sl[b]  = sum_{h = 1}^{n_overtone - 1} z[h b], a term counting only where h b <= bins - 1 (rising h; n_overtone <= 1: 0)
 *   sl2[b] = sum_{x = 2}^{n_undertone - 1} ( z[lo] + (z[min(lo + 1, bins - 1)] - z[lo]) * (r / x) ), lo = b div x, r = b mod x
 *            (rising x; n_undertone <= 2: 0); every operation in float64
 *   y      = sl - sl2;   soft != 0: y+ = y where y > 0, else 0;   soft == 0: y+ = 1 where y > 0, else 0
 *   normalize != 0: y+ /= (sum_b y+ + 1e-8)
 *   out[b] = fl32( z[b] * y+ )
 * Indices are formed in integers: no frequency grid exists on the device. */
int mmk_f0_filter_f32(const float* s, int64_t s_batch_stride, int64_t s_row_stride, int32_t batch, int32_t frames, int32_t bins,
                      int32_t n_overtone, int32_t n_undertone, int32_t soft, int32_t normalize, float* out, int64_t out_batch_stride,
                      int64_t out_row_stride, mmk_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* MMK_SPEC_FILTER_H_ */
