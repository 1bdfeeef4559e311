// HarmonicSource / PercussiveSource (mimikit/features/functionals.py:736-791): librosa.decompose.hpss as one launch - the running median of
// every bin along time, the running median of every frame along frequency (scipy.ndimage.median_filter, mode="reflect"), the two soft masks
// and their products with the spectrogram.  Spectrograms are (batch, frames, bins), time-major.
//
// A workgroup of two waves owns kTF x kTB outputs.  It stages two images of ORDERED KEYS in LDS (the float's bits, sign-folded so that
// unsigned order is float order: selections need no float compare and pass subnormals through untouched):
//   imgH  (1 + kTF + win_harm - 1) rows of kTB:      row 1 + j is frame t0 - win_harm/2 + j of the tile's bins (reflected at the clip's ends)
//   imgP  (1 + kTB + win_perc - 1) rows of kTF + 1:  row 1 + j is bin b0 - win_perc/2 + j of the tile's frames - the TRANSPOSE, so that both
//         walks step along rows with consecutive lanes on consecutive words (no bank conflict), and one routine serves both
// Wave 0 walks imgH (lane = bin), wave 1 walks imgP (lane = frame).  A walk keeps its window in registers, oldest first, with each element's
// count of STRICTLY smaller window elements.  A step shifts the window by one slot, takes the leaving element x_old and the entering x_new
// from LDS and corrects every count by (x_new < k) - (x_old < k): 2 compares per slot where a fresh rank count makes `win`; x_new's own
// count is one more compare per slot.  The element of rank r is then max{k : count(k) <= r} - ties need no order among themselves: every
// element above the rank-r value has more than r elements below it, and the rank-r value itself has at most r.  The median of output o is
// written over the slot of the element that left the window at that step (row o of the image), so the images need no second copy.
// Windows are run-time values: the register window has W = 16, 32 or 64 slots, the live ones at its end; slots before W - win hold the
// largest key and a count no rank reaches.
// The epilogue (lanes along bins, coalesced) reads both medians back from LDS, s from memory (the tile was just read: L2), and writes only
// the outputs asked for.
#include <math.h>

#include "entry_util.h"

namespace mmk {

constexpr int kHpssTF = MMK_HPSS_TILE_FRAMES, kHpssTB = MMK_HPSS_TILE_BINS;
constexpr int kHpssThreads = 128;
constexpr int kPitchH = kHpssTB, kPitchP = kHpssTF + 1;
constexpr uint32_t kKeyMax = 0xffffffffu, kCountOut = 1u << 20;
static_assert(kHpssTF == 64 && kHpssTB == 64, "one wave of 64 lanes walks the tile's 64 bins, the other its 64 frames");

__device__ __forceinline__ uint32_t hpss_key(float v) {
  const uint32_t b = __float_as_uint(v);
  return b ^ ((uint32_t)((int32_t)b >> 31) | 0x80000000u);
}
__device__ __forceinline__ float hpss_value(uint32_t k) { return __uint_as_float(k ^ ((k & 0x80000000u) ? 0x80000000u : 0xffffffffu)); }

// line[(1 + j) * pitch], j = 0 .. n_out + win - 2: the padded axis;  line[o * pitch], o = 0 .. n_out - 1, receives the medians
// FIT: win == W, every slot is live; otherwise win > W / 2 (or W == 16): slots from W / 2 - 1 on (W == 16: the last) are always live
template <int W, bool FIT>
__device__ __forceinline__ void median_walk(uint32_t* line, int pitch, int win, int n_out) {
  constexpr int kMaskable = FIT ? 0 : W == 16 ? W - 1 : W / 2 - 1;      // slots before this one may lie before W - win
  uint32_t k[W], c[W];
#pragma unroll
  for (int i = 0; i < W; ++i) {
    k[i] = kKeyMax;
    c[i] = kCountOut;
  }
  const int lo = W - win;                                    // first live slot
  const uint32_t rank = (uint32_t)(win >> 1);
  const int steps = n_out + win - 1;
  for (int j = 0; j < steps; ++j) {
    const uint32_t x_new = line[(1 + j) * pitch];
    const uint32_t x_old = j >= win ? line[(1 + j - win) * pitch] : kKeyMax;      // (nothing leaves while the window fills)
    uint32_t below = 0;
    int lo_j = lo;
    asm volatile("" : "+s"(lo_j));                           // keeps W lane masks of `i < lo` from being hoisted out of the walk (they spill)
#pragma unroll
    for (int i = 0; i < W - 1; ++i) {
      const uint32_t kk = k[i + 1];
      const uint32_t cc = c[i + 1] + (uint32_t)(x_new < kk) - (uint32_t)(x_old < kk);
      const bool out = i < kMaskable && i < lo_j;            // uniform
      k[i] = out ? kKeyMax : kk;
      c[i] = out ? kCountOut : cc;
      below += (uint32_t)(k[i] < x_new);
    }
    k[W - 1] = x_new;
    c[W - 1] = below;
    if (j >= win - 1) {
      uint32_t med = 0;
#pragma unroll
      for (int i = 0; i < W; ++i) {
        const uint32_t cand = c[i] <= rank ? k[i] : 0u;
        med = cand > med ? cand : med;
      }
      line[(j - win + 1) * pitch] = med;
    }
  }
}

// half-sample reflection of p about [0, n); one fold (win / 2 <= n), -1 where that leaves the axis (positions past a partial tile)
__device__ __forceinline__ int64_t hpss_reflect(int64_t p, int64_t n) {
  if (p < 0) p = -p - 1;
  else if (p >= n) p = 2 * n - 1 - p;
  return (p >= 0 && p < n) ? p : -1;
}

enum HpssMode : int { HPSS_LINEAR = 0, HPSS_POW = 1, HPSS_HARD = 2 };

// librosa.util.softmask in its order of operations
__device__ __forceinline__ float hpss_softmask(float X, float R, float power, int mode, float bad_value) {
  if (mode == HPSS_HARD) return X > R ? 1.f : 0.f;
  float Z = fmaxf(X, R);
  const bool bad = Z < __uint_as_float(0x00800000u);
  Z = bad ? 1.f : Z;
  float m = __fdiv_rn(X, Z), r = __fdiv_rn(R, Z);
  if (mode == HPSS_POW) {
    m = powf(m, power);
    r = powf(r, power);
  }
  m = __fdiv_rn(m, __fadd_rn(m, r));
  return bad ? bad_value : m;
}

struct HpssArgs {
  const float* s;
  int64_t s_batch_stride, s_row_stride, frames;
  int32_t bins, win_harm, win_perc, mode;
  float power, margin_harm, margin_perc, bad_value;
  float *harmonic, *percussive, *harm_median, *perc_median;
  int64_t out_batch_stride, out_row_stride, frame_tiles;
  int32_t bin_tiles;
};

template <int WH, bool FH, int WP, bool FP>
__global__ __launch_bounds__(kHpssThreads) void hpss_kernel(HpssArgs a) {
  extern __shared__ uint32_t hpss_lds[];
  uint32_t* imgH = hpss_lds;
  uint32_t* imgP = hpss_lds + (kHpssTF + a.win_harm) * kPitchH;
  const int tid = threadIdx.x;
  const int64_t tile = blockIdx.x;
  const int tb = (int)(tile % a.bin_tiles);
  const int64_t rest = tile / a.bin_tiles;
  const int64_t tf = rest % a.frame_tiles, clip = rest / a.frame_tiles;
  const int64_t t0 = tf * kHpssTF;
  const int b0 = tb * kHpssTB;
  const float* s = a.s + clip * a.s_batch_stride;
  const bool masks = a.harmonic || a.percussive;
  const bool need_h = masks || a.harm_median, need_p = masks || a.perc_median;

  // Staging, kStage loads in flight per lane before their LDS stores.  imgH: a lane keeps its bin and takes every other row (consecutive
  // lanes on consecutive bins: 256-byte rows);  imgP: a lane keeps its (reflected) bin of the padded axis and goes down the frames.
  constexpr int kStage = 8;
  const int lane = tid & 63, half = tid >> 6;
  if (need_h) {
    const int rows = kHpssTF + a.win_harm - 1, left = a.win_harm >> 1;
    const bool bin_ok = b0 + lane < a.bins;
    for (int j0 = half; j0 < rows; j0 += 2 * kStage) {
      uint32_t v[kStage];
#pragma unroll
      for (int u = 0; u < kStage; ++u) {
        const int j = j0 + 2 * u;
        const int64_t t = j < rows ? hpss_reflect(t0 - left + j, a.frames) : -1;
        v[u] = (t >= 0 && bin_ok) ? hpss_key(s[t * a.s_row_stride + b0 + lane]) : 0u;
      }
#pragma unroll
      for (int u = 0; u < kStage; ++u)
        if (j0 + 2 * u < rows) imgH[(1 + j0 + 2 * u) * kPitchH + lane] = v[u];
    }
  }
  if (need_p) {
    const int cols = kHpssTB + a.win_perc - 1, left = a.win_perc >> 1;      // at most 126: one lane per padded bin
    const int64_t b = tid < cols ? hpss_reflect((int64_t)b0 - left + tid, a.bins) : -1;
    for (int f0 = 0; f0 < kHpssTF; f0 += kStage) {
      uint32_t v[kStage];
#pragma unroll
      for (int u = 0; u < kStage; ++u) v[u] = (b >= 0 && t0 + f0 + u < a.frames) ? hpss_key(s[(t0 + f0 + u) * a.s_row_stride + b]) : 0u;
      if (tid < cols) {
#pragma unroll
        for (int u = 0; u < kStage; ++u) imgP[(1 + tid) * kPitchP + f0 + u] = v[u];
      }
    }
  }
  __syncthreads();
  const int64_t frames_here = a.frames - t0 < kHpssTF ? a.frames - t0 : kHpssTF;
  const int bins_here = a.bins - b0 < kHpssTB ? a.bins - b0 : kHpssTB;
  if (half == 0) {
    if (need_h) median_walk<WH, FH>(imgH + lane, kPitchH, a.win_harm, (int)frames_here);
  } else {
    if (need_p) median_walk<WP, FP>(imgP + lane, kPitchP, a.win_perc, bins_here);
  }
  __syncthreads();

  // Epilogue: a lane keeps its bin and takes every other frame, kOut of them at a time
  constexpr int kOut = 4;
  if (lane >= bins_here) return;
  const int64_t out0 = clip * a.out_batch_stride + b0 + lane;
  const float* sc = s + b0 + lane;
  for (int f0 = half; f0 < frames_here; f0 += 2 * kOut) {
    float v[kOut];
#pragma unroll
    for (int u = 0; u < kOut; ++u) v[u] = (masks && f0 + 2 * u < frames_here) ? sc[(t0 + f0 + 2 * u) * a.s_row_stride] : 0.f;
#pragma unroll
    for (int u = 0; u < kOut; ++u) {
      const int f = f0 + 2 * u;
      if (f >= frames_here) break;
      const float hm = need_h ? hpss_value(imgH[f * kPitchH + lane]) : 0.f;
      const float pm = need_p ? hpss_value(imgP[lane * kPitchP + f]) : 0.f;
      const int64_t o = out0 + (t0 + f) * a.out_row_stride;
      if (a.harm_median) a.harm_median[o] = hm;
      if (a.perc_median) a.perc_median[o] = pm;
      if (a.harmonic) a.harmonic[o] = __fmul_rn(v[u], hpss_softmask(hm, __fmul_rn(pm, a.margin_harm), a.power, a.mode, a.bad_value));
      if (a.percussive) a.percussive[o] = __fmul_rn(v[u], hpss_softmask(pm, __fmul_rn(hm, a.margin_perc), a.power, a.mode, a.bad_value));
    }
  }
}

// the register window of a walk: 16, 32 or 64 slots, or exactly 31 for the reference's default kernel_size (no idle slots to mask)
static inline int hpss_slots(int win) { return win == 31 ? 3 : win <= 16 ? 0 : win <= 32 ? 1 : 2; }

template <int WH, bool FH>
static int hpss_launch_p(int wp, dim3 grid, size_t lds, hipStream_t st, const HpssArgs& a) {
  switch (wp) {
    case 0: return launch(hpss_kernel<WH, FH, 16, false>, grid, dim3(kHpssThreads), lds, st, a);
    case 1: return launch(hpss_kernel<WH, FH, 32, false>, grid, dim3(kHpssThreads), lds, st, a);
    case 2: return launch(hpss_kernel<WH, FH, 64, false>, grid, dim3(kHpssThreads), lds, st, a);
    default: return launch(hpss_kernel<WH, FH, 31, true>, grid, dim3(kHpssThreads), lds, st, a);
  }
}

}  // namespace mmk

extern "C" int mmk_hpss_f32(const float* s, int64_t s_batch_stride, int64_t s_row_stride, int32_t batch, int64_t frames, int32_t bins,
                            int32_t win_harm, int32_t win_perc, float power, float margin_harm, float margin_perc, float* harmonic,
                            float* percussive, float* harm_median, float* perc_median, int64_t out_batch_stride, int64_t out_row_stride,
                            mmk_stream_t stream) {
  using namespace mmk;
  if (!s || batch < 1 || frames < 1 || bins < 1)
    return fail(MMK_ERR_INVALID, "hpss: bad arguments (s %p, batch %d, frames %lld, bins %d)", (const void*)s, batch, (long long)frames, bins);
  if (!harmonic && !percussive && !harm_median && !perc_median) return fail(MMK_ERR_INVALID, "hpss: no output requested");
  if (win_harm < 1 || win_perc < 1) return fail(MMK_ERR_INVALID, "hpss: windows must be at least 1, got (%d, %d)", win_harm, win_perc);
  if (win_harm > MMK_HPSS_MAX_KERNEL || win_perc > MMK_HPSS_MAX_KERNEL)
    return fail(MMK_ERR_UNSUPPORTED, "hpss: windows (%d, %d), the limit is %d", win_harm, win_perc, MMK_HPSS_MAX_KERNEL);
  if (frames < win_harm / 2 || bins < win_perc / 2)
    return fail(MMK_ERR_INVALID, "hpss: windows (%d, %d) fold an axis of (%lld frames, %d bins) more than once: each axis needs at least win / 2",
                win_harm, win_perc, (long long)frames, bins);
  if (!(margin_harm >= 1.f) || !(margin_perc >= 1.f))
    return fail(MMK_ERR_INVALID, "hpss: margins must be at least 1, got (%g, %g)", (double)margin_harm, (double)margin_perc);
  if (!(power > 0.f)) return fail(MMK_ERR_INVALID, "hpss: power must be positive, got %g", (double)power);
  if (s_row_stride < bins || out_row_stride < bins ||
      (batch > 1 && (s_batch_stride < 0 || out_batch_stride < (frames - 1) * out_row_stride + bins)))
    return fail(MMK_ERR_INVALID, "hpss: strides (s %lld / %lld, out %lld / %lld) for %d clips of (%lld, %d)", (long long)s_batch_stride,
                (long long)s_row_stride, (long long)out_batch_stride, (long long)out_row_stride, batch, (long long)frames, bins);
  if (misaligned(s, 4) || misaligned(harmonic, 4) || misaligned(percussive, 4) || misaligned(harm_median, 4) || misaligned(perc_median, 4))
    return fail(MMK_ERR_INVALID, "hpss: s and the outputs must be 4-byte aligned");
  HpssArgs a;
  a.s = s; a.s_batch_stride = s_batch_stride; a.s_row_stride = s_row_stride; a.frames = frames;
  a.bins = bins; a.win_harm = win_harm; a.win_perc = win_perc;
  a.mode = isinf(power) ? HPSS_HARD : power == 1.f ? HPSS_LINEAR : HPSS_POW;
  a.power = power; a.margin_harm = margin_harm; a.margin_perc = margin_perc;
  a.bad_value = (margin_harm == 1.f && margin_perc == 1.f) ? 0.5f : 0.f;      // split_zeros
  a.harmonic = harmonic; a.percussive = percussive; a.harm_median = harm_median; a.perc_median = perc_median;
  a.out_batch_stride = out_batch_stride; a.out_row_stride = out_row_stride;
  a.frame_tiles = (frames + kHpssTF - 1) / kHpssTF;
  a.bin_tiles = (bins + kHpssTB - 1) / kHpssTB;
  const int64_t tiles = a.frame_tiles * a.bin_tiles * batch;
  if (tiles > 0x7fffffffLL)
    return fail(MMK_ERR_UNSUPPORTED, "hpss: %lld tiles of %d x %d are more than one launch takes", (long long)tiles, kHpssTF, kHpssTB);
  const size_t lds = sizeof(uint32_t) * ((size_t)(kHpssTF + win_harm) * kPitchH + (size_t)(kHpssTB + win_perc) * kPitchP);
  const dim3 grid((unsigned)tiles);
  hipStream_t st = (hipStream_t)stream;
  switch (hpss_slots(win_harm)) {
    case 0: return hpss_launch_p<16, false>(hpss_slots(win_perc), grid, lds, st, a);
    case 1: return hpss_launch_p<32, false>(hpss_slots(win_perc), grid, lds, st, a);
    case 2: return hpss_launch_p<64, false>(hpss_slots(win_perc), grid, lds, st, a);
    default: return hpss_launch_p<31, true>(hpss_slots(win_perc), grid, lds, st, a);
  }
}
