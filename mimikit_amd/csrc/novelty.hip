// Recurrence-matrix segmentation (mimikit/extract/segment.py:21-174): checkerboard novelty scores along the diagonal of the frames'
// cosine self-distance matrix, and the picking of their peaks.
//
//   novelty_kernel<NB>    raw[b][q][i] = 1 / (4 h_q^2) sum_{a, b = -h_q .. h_q, a b != 0} -sign(a) sign(b) d(i + a, i - 1 + b) with
//                         d(r, c) = 1 - <x_r, x_c> rx[r] rx[c], d(r, r) = 0 and 0 where r or c lies outside [0, frames).  A workgroup of four
//                         waves owns a run of MMK_NOVELTY_TILE = 64 output frames and the R = 64 + 2 h_max + 1 frames their boards touch
//                         (local row p = frame i0 - 1 - h_max + p), h_max the largest half-width of the CALL; NB = ceil(R / 32) = 3, 4 or 5
//                         blocks of 32 rows.  The rows are staged by the pieces of frame_walk.h (clamped on both sides: a tile's first
//                         rows lie before frame 0), and the lower triangle of the NB x NB blocks of their Gram matrix is formed with its
//                         products, block w + 4 s on wave w: ONE order of the sum over the bins for every pair of frames, wherever it
//                         sits in a tile.
//                         The Gram tile becomes distances in the same LDS, by diagonal: D[r - c][r] for 0 <= r - c <= 2 h_max + 1 (the
//                         matrix is symmetric; a pitch of 32 NB + 1 keeps the lanes of the stores, which differ in c, and those of the
//                         reads, which differ in r, in different banks).  Then wave w owns one quadrant of the board (sign of a, sign of b)
//                         and lane t output frame i0 + t: it adds the quadrant's distances in fp64 shell by shell (|a| or |b| = s, s = 1 ..
//                         h_max) and keeps the sum at every requested half-width, so a half-width's bits do not depend on which others
//                         were asked for; the four quadrant sums meet in LDS and are joined in one fixed order, divided, rounded to fp32
//                         once.  Neither the band nor the matrix is written; x is read 1 + (2 h_max + 1) / 64 times.
//                         rx comes from the caller, or (NULL) a wave computes it per staged row with wave_inv_row_norm, inv_row_norm's code.
//   novelty_min_kernel / novelty_finish_kernel   scores = raw - min_i raw (per clip and half-width; the minimum over chunks of 4096 frames, then over
//                         the chunks), dg = (sum_q scores[q]) / n_half, added in rising q.
//   peaks_minmax_kernel / peaks_flag_kernel / peaks_suppress_kernel   pick_globally_sorted_maxes: the global range, then per index "a local maximum whose
//                         strength and two dominance tests pass" (state 2), then ONE workgroup decides the candidates in rounds: a candidate is
//                         rejected once an accepted higher-ranked one (greater x, then lower index) lies in [m - wb, m + wa), accepted once
//                         every higher-ranked candidate there is rejected.  The fixed point is the sequential walk's result, whatever the
//                         order in which the threads read each other's decisions.
// No atomics, no workgroup waits for another; every sum has one order, so two calls give the same bits.  NaN in the inputs is not handled.
#include "entry_util.h"
#include "frame_walk.h"
#include "wave_ops.h"

namespace mmk {

constexpr int kNvTile = MMK_NOVELTY_TILE;
constexpr int kNvThreads = 256;
constexpr int kNvMaxKernels = MMK_NOVELTY_MAX_KERNELS;
constexpr int kNvMaxHalf = MMK_NOVELTY_MAX_HALF;
constexpr int kNvMinChunk = 4096;   // frames of one partial minimum
static_assert(kNvTile == 64 && kNvThreads == 256, "one lane per output frame, one wave per quadrant of the board");
static_assert(kNvTile + 2 * kNvMaxHalf + 1 <= 5 * 32, "the rows of a tile fit five blocks of 32");

struct NvHalves {
  int32_t n, hmax;
  int32_t h[kNvMaxKernels];
};

constexpr int nv_max(int a, int b) { return a > b ? a : b; }
constexpr int nv_min(int a, int b) { return a < b ? a : b; }
// the largest half-width whose rows fit NB blocks, the diagonals it needs, and the floats of LDS the three uses share
constexpr int nv_half_cap(int nb) { return nv_min((nb * 32 - kNvTile - 1) / 2, kNvMaxHalf); }
constexpr int nv_deltas(int nb) { return 2 * nv_half_cap(nb) + 2; }
constexpr int nv_lds_floats(int nb) {
  return nv_max(nv_max(nv_deltas(nb) * (nb * 32 + 1), nb * 32 * kFwPitch), 2 * kNvMaxKernels * 4 * kNvTile);
}

template <int NB>
__global__ __launch_bounds__(kNvThreads) void novelty_kernel(const float* __restrict__ x, int64_t batch_stride, int64_t row_stride,
                                                             const float* __restrict__ inv_norm, int64_t T, int32_t K, const NvHalves hv,
                                                             float* __restrict__ raw) {
  constexpr int kRows = NB * 32;                     // staged rows
  constexpr int kRP = kRows + 1;                     // floats between the diagonals of D
  constexpr int kBlocks = NB * (NB + 1) / 2;         // the lower triangle, diagonal blocks included
  constexpr int kSlots = (kBlocks + 3) / 4;          // blocks of a wave
  constexpr int kLoads = kRows / 8;                  // dwords a thread loads per chunk
  __shared__ __attribute__((aligned(16))) float lds[nv_lds_floats(NB)];
  __shared__ float inv_s[kRows];
  float* stage = lds;                                // the K loop's operand rows, then
  float* D = lds;                                    // the distances by diagonal, then
  double* Q = reinterpret_cast<double*>(lds);        // the quadrant sums [half-width][quadrant][frame]

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int col = tid & 31, row0 = tid >> 5;         // loads: bin `col` of rows row0, row0 + 8, ...
  const int fr = lane & 31, fh = lane >> 5;          // MFMA fragments: row fr, bin half fh
  const int hmax = hv.hmax;
  const int R = kNvTile + 2 * hmax + 1;              // rows the tile's boards touch, <= kRows
  const int64_t i0 = (int64_t)blockIdx.x * kNvTile;
  const int64_t g0 = i0 - 1 - hmax;                  // the frame of local row 0
  const float* __restrict__ xb = x + (int64_t)blockIdx.y * batch_stride;

  if (inv_norm) {
    for (int p = tid; p < kRows; p += kNvThreads) {
      const int64_t g = g0 + p;
      const bool in = p < R && g >= 0 && g < T;
      inv_s[p] = inv_norm[(int64_t)blockIdx.y * T + (in ? g : 0)] * (in ? 1.f : 0.f);
    }
  } else {
    for (int p = wave; p < kRows; p += 4) {
      const int64_t g = g0 + p;
      float v = 0.f;
      if (p < R && g >= 0 && g < T) v = wave_inv_row_norm(xb + g * row_stride, K, lane);
      if (lane == 0) inv_s[p] = v;
    }
  }

  int br[kSlots], bc[kSlots];
  bool on[kSlots];
  fw_f32x16 acc[kSlots];
#pragma unroll
  for (int s = 0; s < kSlots; ++s) {
    const int idx = wave + 4 * s;
    on[s] = idx < kBlocks;
    int r = 0;
    while ((r + 1) * (r + 2) / 2 <= idx) ++r;
    br[s] = on[s] ? r : 0;
    bc[s] = on[s] ? idx - r * (r + 1) / 2 : 0;
#pragma unroll
    for (int q = 0; q < 16; ++q) acc[s][q] = 0.f;
  }

  float rg[kLoads];
  auto gload = [&](int k0) { fw_load<kLoads, 8, 0, true>(rg, xb, row_stride, g0, T, row0, col, k0, K); };
  gload(0);
  for (int k0 = 0; k0 < K; k0 += kFwKC) {
    const bool kin = k0 + col < K;
#pragma unroll
    for (int i = 0; i < kLoads; ++i) {
      const int p = i * 8 + row0;
      const int64_t g = g0 + p;
      stage[p * kFwPitch + col] = (kin && p < R && g >= 0 && g < T) ? rg[i] : 0.f;
    }
    __syncthreads();
    if (k0 + kFwKC < K) gload(k0 + kFwKC);
#pragma unroll
    for (int gb = 0; gb < kFwKC; gb += 8) {
#pragma unroll
      for (int s = 0; s < kSlots; ++s)
        if (on[s]) fw_mma(acc[s], fw_frag(stage, br[s] * 32 + fr, gb, fh), fw_frag(stage, bc[s] * 32 + fr, gb, fh));
    }
    __syncthreads();
  }

  // distances by diagonal: the A operand's row (block br) lies in the registers, the B operand's (block bc) on the lane
  const int dmax = 2 * hmax + 1;
#pragma unroll
  for (int s = 0; s < kSlots; ++s) {
    if (on[s]) {
      const int cl = bc[s] * 32 + fr;
      const int64_t gc = g0 + cl;
      const float rc = inv_s[cl];
#pragma unroll
      for (int q = 0; q < 16; ++q) {
        const int rl = fw_acc_row(br[s] * 32, q, fh);
        const int delta = rl - cl;
        if (delta >= 0 && delta <= dmax) {
          const int64_t gr = g0 + rl;
          const bool valid = delta != 0 && gc >= 0 && gr < T && rl < R;
          const float d = __fsub_rn(1.f, __fmul_rn(__fmul_rn(acc[s][q], inv_s[rl]), rc));
          D[delta * kRP + rl] = valid ? d : 0.f;
        }
      }
    }
  }
  __syncthreads();

  // wave = quadrant (sign of a, sign of b), lane = output frame; the board's centre is (i, i - 1)
  const int sa = (wave & 1) ? 1 : -1, sb = (wave & 2) ? 1 : -1;
  const int pr = lane + 1 + hmax, pc = lane + hmax;
  auto dist = [&](int r, int c) {
    const int hi = r > c ? r : c, lo = r > c ? c : r;
    return (double)D[(hi - lo) * kRP + hi];
  };
  double sum = 0.0;
  double snap[kNvMaxKernels];
#pragma unroll
  for (int q = 0; q < kNvMaxKernels; ++q) snap[q] = 0.0;
  for (int s = 1; s <= hmax; ++s) {
    const int r = pr + sa * s, c = pc + sb * s;
    for (int j = 1; j <= s; ++j) sum += dist(r, pc + sb * j);
    for (int j = 1; j < s; ++j) sum += dist(pr + sa * j, c);
#pragma unroll
    for (int q = 0; q < kNvMaxKernels; ++q)
      if (q < hv.n && hv.h[q] == s) snap[q] = sum;
  }
  __syncthreads();                                   // (every read of D lies before it)
#pragma unroll
  for (int q = 0; q < kNvMaxKernels; ++q)
    if (q < hv.n) Q[(q * 4 + wave) * kNvTile + lane] = snap[q];
  __syncthreads();
  if (tid < kNvTile && i0 + tid < T) {
    for (int q = 0; q < hv.n; ++q) {
      const double* Qq = Q + q * 4 * kNvTile + tid;
      const double h = (double)hv.h[q];
      const double v = ((Qq[1 * kNvTile] + Qq[2 * kNvTile]) - (Qq[3 * kNvTile] + Qq[0])) / (4.0 * h * h);
      raw[((int64_t)blockIdx.y * hv.n + q) * T + i0 + tid] = (float)v;
    }
  }
}

// ---- scores = raw - min, dg = mean over the half-widths ---------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void novelty_min_kernel(const float* __restrict__ raw, int64_t T, int32_t n_chunks, float* __restrict__ part) {
  __shared__ float red[4];
  const int64_t row = blockIdx.y;
  const int64_t beg = (int64_t)blockIdx.x * kNvMinChunk;
  const int64_t end = beg + kNvMinChunk < T ? beg + kNvMinChunk : T;
  float m = __int_as_float(0x7f800000);
  for (int64_t i = beg + threadIdx.x; i < end; i += 256) m = fminf(m, raw[row * T + i]);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) m = fminf(m, __shfl_xor(m, o));
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = m;
  __syncthreads();
  if (threadIdx.x == 0) part[row * n_chunks + blockIdx.x] = fminf(fminf(red[0], red[1]), fminf(red[2], red[3]));
}

__global__ __launch_bounds__(256) void novelty_finish_kernel(const float* __restrict__ raw, int64_t T, int32_t n_half, int32_t n_chunks,
                                                             const float* __restrict__ part, float* __restrict__ scores,
                                                             float* __restrict__ dg) {
  __shared__ float mins[kNvMaxKernels];
  const int64_t b = blockIdx.y;
  if (threadIdx.x < n_half) {
    const float* p = part + (b * n_half + threadIdx.x) * n_chunks;
    float m = p[0];
    for (int c = 1; c < n_chunks; ++c) m = fminf(m, p[c]);
    mins[threadIdx.x] = m;
  }
  __syncthreads();
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= T) return;
  float a = 0.f;
  for (int q = 0; q < n_half; ++q) {
    const int64_t at = (b * n_half + q) * T + i;
    const float s = __fsub_rn(raw[at], mins[q]);
    scores[at] = s;
    a = q == 0 ? s : __fadd_rn(a, s);
  }
  dg[b * T + i] = a / (float)n_half;
}

// ---- peak picking -------------------------------------------------------------------------------------------------------------------------
constexpr int kPkThreads = 1024;

__global__ __launch_bounds__(kPkThreads) void peaks_minmax_kernel(const float* __restrict__ x, int64_t n, float* __restrict__ mm) {
  __shared__ float lo_s[kPkThreads / 64], hi_s[kPkThreads / 64];
  float lo = __int_as_float(0x7f800000), hi = __int_as_float(0xff800000);
  for (int64_t i = threadIdx.x; i < n; i += kPkThreads) {
    const float v = x[i];
    lo = fminf(lo, v);
    hi = fmaxf(hi, v);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    lo = fminf(lo, __shfl_xor(lo, o));
    hi = fmaxf(hi, __shfl_xor(hi, o));
  }
  if ((threadIdx.x & 63) == 0) {
    lo_s[threadIdx.x >> 6] = lo;
    hi_s[threadIdx.x >> 6] = hi;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < kPkThreads / 64; ++w) {
      lo = fminf(lo, lo_s[w]);
      hi = fmaxf(hi, hi_s[w]);
    }
    mm[0] = lo;
    mm[1] = hi;
  }
}

// state: 0 no candidate (or a rejected one), 1 accepted, 2 undecided
__global__ __launch_bounds__(256) void peaks_flag_kernel(const float* __restrict__ x, int64_t n, int32_t wb, int32_t wa, double min_strength,
                                                         const float* __restrict__ mm, int32_t* __restrict__ state) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const float gmin = mm[0], gmax = mm[1];
  const float xi = x[i];
  int st = 0;
  // librosa.util.localmax: greater than the left neighbour, not less than the right one, the ends padded with themselves
  if (xi > x[i > 0 ? i - 1 : 0] && xi >= x[i + 1 < n ? i + 1 : n - 1] && gmax > gmin) {
    // scipy's minimum_filter1d(size = wb + wa, mode = "constant", cval = the global minimum): the window [i - size / 2, i + size - size / 2 - 1]
    const int size = wb + wa;
    float mn = __int_as_float(0x7f800000);
    for (int64_t j = i - size / 2; j < i - size / 2 + size; ++j) mn = fminf(mn, (j < 0 || j >= n) ? gmin : x[j]);
    const double strength = ((double)xi - (double)mn) / ((double)gmax - (double)gmin);
    if (strength >= min_strength) {
      const int64_t lo = i - wb > 0 ? i - wb : 0, hi = i + wa < n ? i + wa : n;
      double sl = 0.0, sr = 0.0;
      for (int64_t j = lo; j < i; ++j) sl += (double)x[j];
      for (int64_t j = i; j < hi; ++j) sr += (double)x[j];
      if (i > lo && hi > i && (double)xi > sl / (double)(i - lo) && (double)xi > sr / (double)(hi - i)) st = 2;
    }
  }
  state[i] = st;
}

__global__ __launch_bounds__(kPkThreads) void peaks_suppress_kernel(const float* __restrict__ x, int64_t n, int32_t wb, int32_t wa,
                                                                    int32_t* state_, uint8_t* __restrict__ picked) {
  volatile int32_t* state = state_;
  for (;;) {
    int pending = 0;
    for (int64_t i = threadIdx.x; i < n; i += kPkThreads) {
      if (state[i] != 2) continue;
      const float xi = x[i];
      const int64_t lo = i - wb > 0 ? i - wb : 0, hi = i + wa < n ? i + wa : n;
      bool accepted = false, undecided = false;
      for (int64_t j = lo; j < hi; ++j) {
        const int s = state[j];
        if (s == 0 || j == i) continue;
        const float xj = x[j];
        if (xj > xi || (xj == xi && j < i)) {          // ranked above i
          accepted = accepted || s == 1;
          undecided = undecided || s == 2;
        }
      }
      if (accepted) state[i] = 0;
      else if (undecided) pending = 1;
      else state[i] = 1;
    }
    if (!__syncthreads_or(pending)) break;
  }
  for (int64_t i = threadIdx.x; i < n; i += kPkThreads) picked[i] = state[i] == 1 ? 1 : 0;
}

template <int NB>
static int novelty_launch(const float* x, int64_t bs, int64_t rs, const float* inv_norm, int32_t batch, int64_t frames, int32_t bins,
                          const NvHalves& hv, float* raw, hipStream_t st) {
  const int64_t tiles = (frames + kNvTile - 1) / kNvTile;
  return launch(novelty_kernel<NB>, dim3((unsigned)tiles, (unsigned)batch), dim3(kNvThreads), 0, st, x, bs, rs, inv_norm, frames, bins, hv, raw);
}

}  // namespace mmk

extern "C" int mmk_novelty_f32(const float* x, int64_t x_batch_stride, int64_t x_row_stride, const float* inv_norm, int32_t batch, int64_t frames,
                               int32_t bins, const int32_t* halves, int32_t n_half, float* raw, mmk_stream_t stream) {
  using namespace mmk;
  if (batch < 1) return fail(MMK_ERR_INVALID, "novelty: batch = %d < 1", batch);
  if (frames < 2) return fail(MMK_ERR_INVALID, "novelty: frames = %lld < 2 (a board needs two frames)", (long long)frames);
  if (bins < 1) return fail(MMK_ERR_INVALID, "novelty: bins = %d < 1", bins);
  if (!x || !halves || !raw || x_batch_stride < 0 || x_row_stride < 0)
    return fail(MMK_ERR_INVALID, "novelty: bad arguments (null pointer or negative stride %lld / %lld)", (long long)x_batch_stride,
                (long long)x_row_stride);
  if (misaligned(x, 4) || misaligned(inv_norm, 4) || misaligned(raw, 4)) return fail(MMK_ERR_INVALID, "novelty: x, inv_norm and raw must be 4-byte aligned");
  if (n_half < 1) return fail(MMK_ERR_INVALID, "novelty: n_half = %d < 1 (half-widths)", n_half);
  if (n_half > kNvMaxKernels)
    return fail(MMK_ERR_UNSUPPORTED, "novelty: %d half-widths, more than the %d (MMK_NOVELTY_MAX_KERNELS) one launch sums", n_half, kNvMaxKernels);
  NvHalves hv;
  hv.n = n_half;
  hv.hmax = 0;
  for (int q = 0; q < kNvMaxKernels; ++q) hv.h[q] = 0;
  for (int q = 0; q < n_half; ++q) {
    if (halves[q] < 1) return fail(MMK_ERR_INVALID, "novelty: half-width %d = %d < 1", q, halves[q]);
    if (halves[q] > kNvMaxHalf)
      return fail(MMK_ERR_UNSUPPORTED, "novelty: half-width %d = %d, the limit is %d (MMK_NOVELTY_MAX_HALF)", q, halves[q], kNvMaxHalf);
    hv.h[q] = halves[q];
    hv.hmax = halves[q] > hv.hmax ? halves[q] : hv.hmax;
  }
  if (batch > 65535 || (frames + kNvTile - 1) / kNvTile > 0x7fffffffLL)
    return fail(MMK_ERR_UNSUPPORTED, "novelty: %d clips of %lld frames are more than one launch takes", batch, (long long)frames);
  const int rows = kNvTile + 2 * hv.hmax + 1;
  hipStream_t st = (hipStream_t)stream;
  if (rows <= 96) return novelty_launch<3>(x, x_batch_stride, x_row_stride, inv_norm, batch, frames, bins, hv, raw, st);
  if (rows <= 128) return novelty_launch<4>(x, x_batch_stride, x_row_stride, inv_norm, batch, frames, bins, hv, raw, st);
  return novelty_launch<5>(x, x_batch_stride, x_row_stride, inv_norm, batch, frames, bins, hv, raw, st);
}

extern "C" size_t mmk_novelty_finish_workspace_floats(int32_t batch, int32_t n_half, int64_t frames) {
  if (batch < 1 || n_half < 1 || frames < 1) return 0;
  return (size_t)batch * (size_t)n_half * (size_t)((frames + mmk::kNvMinChunk - 1) / mmk::kNvMinChunk);
}

extern "C" int mmk_novelty_finish_f32(const float* raw, int32_t batch, int32_t n_half, int64_t frames, float* scores, float* dg, float* workspace,
                                      size_t workspace_floats, mmk_stream_t stream) {
  using namespace mmk;
  if (batch < 1 || frames < 1) return fail(MMK_ERR_INVALID, "novelty_finish: batch = %d, frames = %lld: both must be >= 1", batch, (long long)frames);
  if (n_half < 1) return fail(MMK_ERR_INVALID, "novelty_finish: n_half = %d < 1", n_half);
  if (n_half > kNvMaxKernels)
    return fail(MMK_ERR_UNSUPPORTED, "novelty_finish: %d half-widths, the limit is %d (MMK_NOVELTY_MAX_KERNELS)", n_half, kNvMaxKernels);
  if (!raw || !scores || !dg || !workspace || misaligned(raw, 4) || misaligned(scores, 4) || misaligned(dg, 4) || misaligned(workspace, 4))
    return fail(MMK_ERR_INVALID, "novelty_finish: bad arguments (null or misaligned pointer)");
  if (workspace_floats < mmk_novelty_finish_workspace_floats(batch, n_half, frames))
    return fail(MMK_ERR_WORKSPACE, "novelty_finish: the workspace has %zu floats, %zu are needed", workspace_floats,
                mmk_novelty_finish_workspace_floats(batch, n_half, frames));
  const int64_t n_chunks = (frames + kNvMinChunk - 1) / kNvMinChunk;
  if ((int64_t)batch * n_half > 65535 || n_chunks > 0x7fffffffLL || (frames + 255) / 256 > 0x7fffffffLL)
    return fail(MMK_ERR_UNSUPPORTED, "novelty_finish: %d clips of %lld frames are more than one launch takes", batch, (long long)frames);
  hipStream_t st = (hipStream_t)stream;
  MMK_TRY(launch(novelty_min_kernel, dim3((unsigned)n_chunks, (unsigned)(batch * n_half)), dim3(256), 0, st, raw, frames, (int32_t)n_chunks, workspace));
  return launch(novelty_finish_kernel, dim3((unsigned)((frames + 255) / 256), (unsigned)batch), dim3(256), 0, st, raw, frames, n_half,
                (int32_t)n_chunks, workspace, scores, dg);
}

extern "C" size_t mmk_pick_peaks_workspace_bytes(int64_t n) { return n < 1 ? 0 : ((size_t)n + 2) * 4; }

extern "C" int mmk_pick_peaks_f32(const float* x, int64_t n, int32_t wait_before, int32_t wait_after, double min_strength, uint8_t* picked,
                                  void* workspace, size_t workspace_bytes, mmk_stream_t stream) {
  using namespace mmk;
  if (n < 1) return fail(MMK_ERR_INVALID, "pick_peaks: n = %lld < 1", (long long)n);
  if (wait_before < 0 || wait_after < 0 || wait_before + wait_after < 1)
    return fail(MMK_ERR_INVALID, "pick_peaks: wait_before = %d, wait_after = %d: neither may be negative and one must be positive", wait_before,
                wait_after);
  if (wait_before > MMK_NOVELTY_MAX_WAIT || wait_after > MMK_NOVELTY_MAX_WAIT)
    return fail(MMK_ERR_UNSUPPORTED, "pick_peaks: wait_before = %d, wait_after = %d, the limit is %d (MMK_NOVELTY_MAX_WAIT)", wait_before, wait_after,
                MMK_NOVELTY_MAX_WAIT);
  if (!(min_strength == min_strength)) return fail(MMK_ERR_INVALID, "pick_peaks: min_strength is NaN");
  if (!x || !picked || !workspace || misaligned(x, 4) || misaligned(workspace, 4))
    return fail(MMK_ERR_INVALID, "pick_peaks: bad arguments (null or misaligned pointer)");
  MMK_TRY(workspace_check("pick_peaks", workspace, 4, workspace_bytes, mmk_pick_peaks_workspace_bytes(n)));
  if ((n + 255) / 256 > 0x7fffffffLL) return fail(MMK_ERR_UNSUPPORTED, "pick_peaks: n = %lld is more than one launch takes", (long long)n);
  hipStream_t st = (hipStream_t)stream;
  float* mm = static_cast<float*>(workspace);
  int32_t* state = reinterpret_cast<int32_t*>(mm + 2);
  MMK_TRY(launch(peaks_minmax_kernel, dim3(1), dim3(kPkThreads), 0, st, x, n, mm));
  MMK_TRY(launch(peaks_flag_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, x, n, wait_before, wait_after, min_strength, mm, state));
  return launch(peaks_suppress_kernel, dim3(1), dim3(kPkThreads), 0, st, x, n, wait_before, wait_after, state, picked);
}
