// AutoConvolve and F0Filter (mimikit/features/functionals.py:1007-1080; include/mmk_spec_filter.h): a per-frame float64 weight for every bin of
// a (T, F) magnitude spectrogram, normalised over the frame and multiplied onto the input.  One launch per call, no workspace, no atomics.
//
//   spec_filter_kernel<ROW>  one skeleton, two row filters.  A workgroup of 256 threads takes kSfFrames consecutive frames of one clip, one after
//     the other; thread i owns the bins i, i + 256, ... of every frame.  Per frame:
//       weights   ROW::weight(b) in float64 -> y[b] in LDS (the owner alone reads it back), and the thread's own running sum in rising b;
//       the sum   block_sum (wave_ops.h): the butterfly inside a wave, then the four waves in rising order.  The order depends on F alone, so a
//                 frame gives the same bits whatever T, the batch and its place in them are;
//       the write out[b] = fl32(ROW::apply(y[b], total) * z[b]), one rounding, 256 contiguous bytes per wave.
//   AutoConvolveRow  the product over the window's rows, read from global memory one float per lane (rows of 1025 floats are 4-byte aligned only):
//     the k rows of a frame are k coalesced reads, k - 1 of which the frame before it in the same workgroup (or the workgroup next door) has
//     just brought into cache; frames outside the clip are skipped, which is what a factor 1.0 does.  log(1.0 + p) in float64.
//   F0FilterRow  the frame is staged in LDS once (float32) and every harmonic is gathered from there.
//     overtones   z[h b] for h b <= F - 1: lane stride h.  ds_read_b32 has 32 banks and conflicts inside a half wave: gcd(h, 32)-way, so 2-way
//                 for h = 2, 6, 10, 14, 4-way for 4 and 12, 8-way for 8.  But harmonic h reads only the bins below F / h - the waves above
//                 skip the read - so the reads of a frame are F (1 + 1/2 + 1/3 + ...) and the conflict cycles on top of them F (1/2 + 1/4 +
//                 1/6 + 1/8 ...) / 32 per lane group: about a third of the gather's LDS cycles at n_overtone = 4, and the gather itself is a
//                 small part of the frame beside the float64 arithmetic (DESIGN.md 5.6.14 has the figures).  No padding or swizzle is applied.
//     undertones  lo = b div x through a multiplication (below), r = b mod x, and r / x from a table of the 120 quotients that exist for
//                 x <= 15, computed once per workgroup by the float64 division itself: the same bits as dividing in place.  Lanes b .. b + x - 1
//                 read the same two words: a broadcast, no conflict.
// No workgroup waits for another; out must not overlap s.  NaN, negative and infinite bins are not looked for.
#include "entry_util.h"
#include "wave_ops.h"

#include "../../include/mmk_spec_filter.h"

namespace mmk {

constexpr int kSfThreads = 256;
constexpr int kSfFrames = MMK_SPEC_FILTER_TILE_FRAMES;
constexpr int kSfMaxBins = MMK_SPEC_FILTER_MAX_BINS;
constexpr int kF0MaxX = MMK_F0_FILTER_MAX_UNDERTONE - 1;       // the largest undertone divisor
constexpr int kF0Fracs = kF0MaxX * (kF0MaxX + 1) / 2;         // r / x for 1 <= x <= kF0MaxX, 0 <= r < x, at x (x - 1) / 2 + r
// b div x as (b * ceil(2^18 / x)) >> 18: with e = ceil(2^18 / x) - 2^18 / x in [0, 1) the product is 2^18 (b / x + b e / 2^18), and
// b e / 2^18 < 2^12 / 2^18 < 1 / x cannot carry b / x = q + r / x, r <= x - 1, to q + 1.  Needs b <= 4096, x <= 16; b * ceil(2^18 / x) < 2^31
constexpr int kF0Shift = 18;
static_assert(kSfMaxBins - 1 <= 4096 && kF0MaxX <= 16, "the multiplication that stands for b div x is proven for b <= 4096 and x <= 16");
static_assert(kSfThreads >= kF0Fracs, "one thread per quotient of the table");

struct FrameArgs {
  const float* __restrict__ s;          // the clip's first frame
  int64_t s_row_stride;
  int32_t frames, bins;
};

struct AutoConvolveRow {
  int32_t window;
  const float* first;                   // the window's first row inside the clip
  const float* own;                     // frame t
  int64_t stride;
  int32_t rows;
  static size_t lds_bytes(int32_t) { return 0; }
  __device__ void prepare(char*, int32_t) {}
  __device__ void frame(const FrameArgs& a, int32_t t) {
    const int64_t lo = (int64_t)t - window / 2;
    const int64_t u0 = lo < 0 ? 0 : lo, u1 = lo + window > a.frames ? a.frames : lo + window;
    first = a.s + u0 * a.s_row_stride;
    own = a.s + (int64_t)t * a.s_row_stride;
    stride = a.s_row_stride;
    rows = (int32_t)(u1 - u0);
  }
  __device__ double weight(int32_t b) const {
    double p = 1.0;
    const float* q = first + b;
    for (int32_t u = 0; u < rows; ++u, q += stride) p *= (double)*q;
    return log(1.0 + p);
  }
  __device__ double value(int32_t b) const { return (double)own[b]; }
  __device__ double scale(double total) const { return total + 1e-8; }
  __device__ double apply(double y, double denom) const { return y / denom; }
};

struct F0FilterRow {
  int32_t n_overtone, n_undertone, soft, normalize;
  int32_t bins;
  const double* frac;
  float* z;
  static size_t lds_bytes(int32_t bins) { return kF0Fracs * sizeof(double) + (size_t)bins * sizeof(float); }
  __device__ void prepare(char* lds, int32_t bins_) {
    double* f = reinterpret_cast<double*>(lds);
    int x = 1;
    while (x < kF0MaxX && x * (x + 1) / 2 <= (int)threadIdx.x) ++x;
    if ((int)threadIdx.x < kF0Fracs) f[threadIdx.x] = (double)((int)threadIdx.x - x * (x - 1) / 2) / (double)x;
    frac = f;
    z = reinterpret_cast<float*>(f + kF0Fracs);
    bins = bins_;
  }
  __device__ void frame(const FrameArgs& a, int32_t t) {
    const float* row = a.s + (int64_t)t * a.s_row_stride;
    for (int32_t b = threadIdx.x; b < bins; b += kSfThreads) z[b] = row[b];      // (thread i rewrites the words it alone read in the write pass)
    __syncthreads();
  }
  __device__ double weight(int32_t b) const {
    double sl = 0.0, sl2 = 0.0;
    for (int32_t h = 1, p = b; h < n_overtone && p < bins; ++h, p += b) sl += (double)z[p];
    for (int32_t x = 2; x < n_undertone; ++x) {
      const int32_t lo = (int32_t)(((uint32_t)b * (uint32_t)(((1 << kF0Shift) + x - 1) / x)) >> kF0Shift), r = b - lo * x;
      const double a = (double)z[lo], c = (double)z[lo + 1 < bins ? lo + 1 : bins - 1];
      sl2 += a + (c - a) * frac[x * (x - 1) / 2 + r];
    }
    const double y = sl - sl2;
    if (soft) return y > 0.0 ? y : 0.0;
    return y > 0.0 ? 1.0 : 0.0;
  }
  __device__ double value(int32_t b) const { return (double)z[b]; }
  __device__ double scale(double total) const { return total + 1e-8; }
  __device__ double apply(double y, double denom) const { return normalize ? y / denom : y; }
};

template <class ROW>
__global__ __launch_bounds__(kSfThreads) void spec_filter_kernel(const float* __restrict__ s, int64_t s_batch_stride, int64_t s_row_stride, int32_t frames,
                                                                 int32_t bins, int32_t tiles, ROW row, float* __restrict__ out,
                                                                 int64_t out_batch_stride, int64_t out_row_stride) {
  extern __shared__ double sf_lds[];                  // y[bins], then what ROW keeps
  __shared__ double red[kSfThreads / 64];
  double* y = sf_lds;
  const int64_t clip = blockIdx.x / (uint32_t)tiles;
  const int32_t t0 = (int32_t)(blockIdx.x % (uint32_t)tiles) * kSfFrames;
  const int32_t t1 = frames - t0 > kSfFrames ? t0 + kSfFrames : frames;
  const FrameArgs a{s + clip * s_batch_stride, s_row_stride, frames, bins};
  float* oclip = out + clip * out_batch_stride;
  row.prepare(reinterpret_cast<char*>(sf_lds + bins), bins);
  for (int32_t t = t0; t < t1; ++t) {
    row.frame(a, t);
    double part = 0.0;
    for (int32_t b = threadIdx.x; b < bins; b += kSfThreads) {
      const double w = row.weight(b);
      y[b] = w;
      part += w;
    }
    const double denom = row.scale(block_sum(part, red));
    float* orow = oclip + (int64_t)t * out_row_stride;
    for (int32_t b = threadIdx.x; b < bins; b += kSfThreads) orow[b] = (float)(row.apply(y[b], denom) * row.value(b));
  }
}

// what the two entry points refuse alike
static int spec_filter_check(const char* who, const float* s, int64_t s_batch_stride, int64_t s_row_stride, int32_t batch, int32_t frames, int32_t bins,
                             const float* out, int64_t out_batch_stride, int64_t out_row_stride, int64_t* n_blocks, int32_t* tiles) {
  MMK_TRY(rows_check(who, s, s_row_stride, frames, bins, out, out_row_stride, bins, true));
  if (batch < 1 || bins < 2 || (batch > 1 && (s_batch_stride < 0 || out_batch_stride < bins)))
    return fail(MMK_ERR_INVALID, "%s: bad arguments (batch=%d, bins=%d: at least 1 clip of at least 2 bins; batch strides %lld / %lld)", who, batch, bins,
                (long long)s_batch_stride, (long long)out_batch_stride);
  if (s == out) return fail(MMK_ERR_INVALID, "%s: out must not overlap s", who);
  if (bins > kSfMaxBins)
    return fail(MMK_ERR_UNSUPPORTED, "%s: %d bins, more than the %d (MMK_SPEC_FILTER_MAX_BINS) a workgroup keeps in LDS", who, bins, kSfMaxBins);
  *tiles = (int32_t)(((int64_t)frames + kSfFrames - 1) / kSfFrames);
  *n_blocks = (int64_t)batch * *tiles;
  if (*n_blocks > 0x7fffffffLL)
    return fail(MMK_ERR_UNSUPPORTED, "%s: %d clips of %d frames are more than one launch takes", who, batch, frames);
  return MMK_OK;
}

template <class ROW>
static int spec_filter_launch(const float* s, int64_t s_batch_stride, int64_t s_row_stride, int32_t frames, int32_t bins, int64_t n_blocks, int32_t tiles,
                              ROW row, float* out, int64_t out_batch_stride, int64_t out_row_stride, hipStream_t st) {
  const size_t lds = (size_t)bins * sizeof(double) + ROW::lds_bytes(bins);
  return launch(spec_filter_kernel<ROW>, dim3((unsigned)n_blocks), dim3(kSfThreads), lds, st, s, s_batch_stride, s_row_stride, frames, bins, tiles, row, out,
                out_batch_stride, out_row_stride);
}

}  // namespace mmk

using namespace mmk;

extern "C" int mmk_auto_convolve_f32(const float* s, int64_t s_batch_stride, int64_t s_row_stride, int32_t batch, int32_t frames, int32_t bins,
                                     int32_t window, float* out, int64_t out_batch_stride, int64_t out_row_stride, mmk_stream_t stream) {
  int64_t n_blocks = 0;
  int32_t tiles = 0;
  MMK_TRY(spec_filter_check("auto_convolve", s, s_batch_stride, s_row_stride, batch, frames, bins, out, out_batch_stride, out_row_stride, &n_blocks, &tiles));
  if (window < 2) return fail(MMK_ERR_INVALID, "auto_convolve: window = %d, at least 2 (the reference's own slice is empty at 1)", window);
  if (window > MMK_AUTO_CONVOLVE_MAX_WINDOW)
    return fail(MMK_ERR_UNSUPPORTED, "auto_convolve: window = %d frames, more than %d (MMK_AUTO_CONVOLVE_MAX_WINDOW)", window, MMK_AUTO_CONVOLVE_MAX_WINDOW);
  AutoConvolveRow row{};
  row.window = window;
  return spec_filter_launch(s, s_batch_stride, s_row_stride, frames, bins, n_blocks, tiles, row, out, out_batch_stride, out_row_stride, (hipStream_t)stream);
}

extern "C" int mmk_f0_filter_f32(const float* s, int64_t s_batch_stride, int64_t s_row_stride, int32_t batch, int32_t frames, int32_t bins,
                                 int32_t n_overtone, int32_t n_undertone, int32_t soft, int32_t normalize, float* out, int64_t out_batch_stride,
                                 int64_t out_row_stride, mmk_stream_t stream) {
  int64_t n_blocks = 0;
  int32_t tiles = 0;
  MMK_TRY(spec_filter_check("f0_filter", s, s_batch_stride, s_row_stride, batch, frames, bins, out, out_batch_stride, out_row_stride, &n_blocks, &tiles));
  if (n_overtone < 0 || n_undertone < 0)
    return fail(MMK_ERR_INVALID, "f0_filter: n_overtone = %d, n_undertone = %d (neither may be negative)", n_overtone, n_undertone);
  if (n_overtone > MMK_F0_FILTER_MAX_OVERTONE || n_undertone > MMK_F0_FILTER_MAX_UNDERTONE)
    return fail(MMK_ERR_UNSUPPORTED, "f0_filter: n_overtone = %d, n_undertone = %d, more than %d (MMK_F0_FILTER_MAX_OVERTONE) or %d (MMK_F0_FILTER_MAX_UNDERTONE)",
                n_overtone, n_undertone, MMK_F0_FILTER_MAX_OVERTONE, MMK_F0_FILTER_MAX_UNDERTONE);
  F0FilterRow row{};
  row.n_overtone = n_overtone;
  row.n_undertone = n_undertone;
  row.soft = soft;
  row.normalize = normalize;
  return spec_filter_launch(s, s_batch_stride, s_row_stride, frames, bins, n_blocks, tiles, row, out, out_batch_stride, out_row_stride, (hipStream_t)stream);
}
