// Signal conditioning around the mu-law codec: the first-order filter section behind Emphasis / Deemphasis / RemoveDC
//     y[n] = b0 x[n] + b1 x[n-1] + p y[n-1],   p = -a1,   zero initial state,
// and the row normalisation behind Normalize.  Both are HBM-bound passes over (batch, n) rows that are strided views of longer
// tensors, of any 4-byte alignment.
//
// A workgroup of kLfWg lanes takes one chunk of kLfChunk samples of one row; lane t owns the kLfRun consecutive samples
// [t kLfRun, (t + 1) kLfRun) of it and keeps them in registers.  A run whose 16 samples all lie in the row moves as 16-byte accesses
// from the first 16-byte boundary on, the samples before it and after the last whole quad one by one (rows of the same call start
// at any element of a longer tensor, and x and y need not share an alignment); a run that the row's end cuts moves sample by
// sample, what lies beyond the end counts as zero and is never stored.
//
// The recurrence (p != 0) is a scan.  With local[i] the run's own recurrence from a zero state, sample i of a run is
//     y = local[i] + p^(i+1) carry,          carry = y just before the run,
// and carries compose: over a stretch of L samples that ends in `end` under a zero carry-in, carry_out = end + p^L carry_in.  Every
// stretch of one level has the same length (runs of 16, waves of 1024, chunks of 4096), so the power that joins two neighbours is
// one constant per level - the (value, power) pairs of a general scan carry the same power in every lane, and only the value travels:
//   lanes of a wave   Hillis-Steele over __shfl_up, step d joins with p^(16 d);
//   waves             through LDS, joined in order with p^1024;
//   chunks            two launches.  The first writes every chunk's end under a zero carry-in to the workspace; the second forms its
//                     chunk's carry-in from the ends of the chunks before it in the row (each wave on its own: 64 ends per round of the
//                     same shuffle scan, joined with p^4096; the rounds are aligned to END at the chunk, so a short first round is
//                     padded with zeros in front and every round joins with p^(4096 64)), recomputes the chunk and stores it.
// The two launches are the only ordering between workgroups: nothing waits for another workgroup, and there are no atomics - every
// sum has one fixed order, so a result does not depend on the run.  Powers of p come from repeated squaring (and p^(i+1), i < 16, from
// a product chain), never from powf.
#include "entry_util.h"
#include "wave_ops.h"

namespace mmk {

constexpr int kLfRun = MMK_LFILTER1_RUN;
constexpr int kLfWg = MMK_LFILTER1_WG;
constexpr int kLfChunk = MMK_LFILTER1_CHUNK;
static_assert(kLfRun == 16 && kLfWg == 256 && kLfChunk == kLfRun * kLfWg, "the level powers below are written for 16 x 64 x 4");

typedef float lf_f32x4 __attribute__((ext_vector_type(4)));

// samples in front of the first 16-byte boundary at or after p (p is 4-byte aligned)
__device__ __forceinline__ int lf_head(const float* p) { return (int)((4 - ((reinterpret_cast<uintptr_t>(p) >> 2) & 3)) & 3); }

template <int H>
__device__ __forceinline__ void lf_load_full(const float* __restrict__ p, float (&v)[kLfRun]) {
  constexpr int kQuads = H ? 3 : 4;
#pragma unroll
  for (int i = 0; i < H; ++i) v[i] = p[i];
#pragma unroll
  for (int k = 0; k < kQuads; ++k) {
    const lf_f32x4 q = *reinterpret_cast<const lf_f32x4*>(p + H + 4 * k);
#pragma unroll
    for (int e = 0; e < 4; ++e) v[H + 4 * k + e] = q[e];
  }
#pragma unroll
  for (int i = H + 4 * kQuads; i < kLfRun; ++i) v[i] = p[i];
}

template <int H>
__device__ __forceinline__ void lf_store_full(float* __restrict__ p, const float (&v)[kLfRun]) {
  constexpr int kQuads = H ? 3 : 4;
#pragma unroll
  for (int i = 0; i < H; ++i) p[i] = v[i];
#pragma unroll
  for (int k = 0; k < kQuads; ++k)
    *reinterpret_cast<lf_f32x4*>(p + H + 4 * k) = lf_f32x4{v[H + 4 * k], v[H + 4 * k + 1], v[H + 4 * k + 2], v[H + 4 * k + 3]};
#pragma unroll
  for (int i = H + 4 * kQuads; i < kLfRun; ++i) p[i] = v[i];
}

// the run at p, of which `cnt` samples (<= 0: none) lie in the row; head = lf_head(p)
__device__ __forceinline__ void lf_load_run(const float* __restrict__ p, int head, int64_t cnt, float (&v)[kLfRun]) {
  if (cnt >= kLfRun) {
    switch (head) {
      case 0: lf_load_full<0>(p, v); break;
      case 1: lf_load_full<1>(p, v); break;
      case 2: lf_load_full<2>(p, v); break;
      default: lf_load_full<3>(p, v); break;
    }
  } else {
#pragma unroll
    for (int i = 0; i < kLfRun; ++i) v[i] = i < cnt ? p[i] : 0.f;
  }
}

__device__ __forceinline__ void lf_store_run(float* __restrict__ p, int head, int64_t cnt, const float (&v)[kLfRun]) {
  if (cnt >= kLfRun) {
    switch (head) {
      case 0: lf_store_full<0>(p, v); break;
      case 1: lf_store_full<1>(p, v); break;
      case 2: lf_store_full<2>(p, v); break;
      default: lf_store_full<3>(p, v); break;
    }
  } else {
#pragma unroll
    for (int i = 0; i < kLfRun; ++i)
      if (i < cnt) p[i] = v[i];
  }
}

// inclusive scan over the lanes of a wave of  E[l] = e[l] + q E[l - 1],  given pw[b] = q^(2^b)
__device__ __forceinline__ float lf_wave_scan(float e, const float (&pw)[6], int lane) {
#pragma unroll
  for (int b = 0; b < 6; ++b) {
    const float o = __shfl_up(e, 1u << b);
    if (lane >= (1 << b)) e = fmaf(pw[b], o, e);
  }
  return e;
}

struct LfRunState {
  const float* xr;      // the row
  int64_t s;            // first sample of this lane's run
  int64_t cnt;          // n - s
  float v[kLfRun];
  float xprev;          // x[s - 1], 0 in front of the row
};

__device__ __forceinline__ void lf_fetch(LfRunState& r, const float* __restrict__ x, int64_t x_row_stride, int64_t n, int64_t row, int64_t chunk) {
  r.xr = x + row * x_row_stride;
  r.s = chunk * kLfChunk + (int64_t)threadIdx.x * kLfRun;
  r.cnt = n - r.s;
  lf_load_run(r.xr + r.s, lf_head(r.xr), r.cnt, r.v);       // (s is a multiple of 4: the run's head is the row's)
  r.xprev = (r.s > 0 && r.cnt >= 0) ? r.xr[r.s - 1] : 0.f;
}

// a1 == 0: y[n] = b0 x[n] + b1 x[n-1], one pass
__global__ __launch_bounds__(kLfWg) void lfilter1_fir_kernel(const float* __restrict__ x, int64_t x_row_stride, int64_t n, int64_t n_chunks,
                                                            float b0, float b1, float* __restrict__ y, int64_t y_row_stride) {
  const int64_t row = blockIdx.x / n_chunks, chunk = blockIdx.x % n_chunks;
  LfRunState r;
  lf_fetch(r, x, x_row_stride, n, row, chunk);
  float out[kLfRun];
  float xp = r.xprev;
#pragma unroll
  for (int i = 0; i < kLfRun; ++i) {
    out[i] = fmaf(b1, xp, b0 * r.v[i]);
    xp = r.v[i];
  }
  float* yr = y + row * y_row_stride;
  lf_store_run(yr + r.s, lf_head(yr), r.cnt, out);
}

// kStore = false: ends[row][chunk] = the chunk's last y under a zero carry-in (launched without each row's last chunk);
// kStore = true: the carry-in from ends[row][0 .. chunk), and the chunk's samples
template <bool kStore>
__global__ __launch_bounds__(kLfWg) void lfilter1_scan_kernel(const float* __restrict__ x, int64_t x_row_stride, int64_t n, int64_t n_chunks,
                                                             int64_t grid_chunks, float b0, float b1, float p, float* __restrict__ y,
                                                             int64_t y_row_stride, float* __restrict__ ends) {
  __shared__ float s_wave_end[kLfWg / 64];
  const int64_t row = blockIdx.x / grid_chunks, chunk = blockIdx.x % grid_chunks;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  LfRunState r;
  lf_fetch(r, x, x_row_stride, n, row, chunk);

  // p^16 2^b (b < 6: the lanes' scan), then p^1024 (waves), p^4096 2^b (chunks)
  const float p2 = p * p, p4 = p2 * p2, p8 = p4 * p4;
  float pw_lane[6];
  pw_lane[0] = p8 * p8;
#pragma unroll
  for (int b = 1; b < 6; ++b) pw_lane[b] = pw_lane[b - 1] * pw_lane[b - 1];
  const float p1024 = pw_lane[5] * pw_lane[5];

  float local[kLfRun];
  float acc = 0.f, xp = r.xprev;
#pragma unroll
  for (int i = 0; i < kLfRun; ++i) {
    acc = fmaf(p, acc, fmaf(b1, xp, b0 * r.v[i]));
    local[i] = acc;
    xp = r.v[i];
  }
  const float incl = lf_wave_scan(acc, pw_lane, lane);      // the end of this lane's run under a zero carry into the WAVE
  if (lane == 63) s_wave_end[wave] = incl;
  __syncthreads();

  if (!kStore) {
    if (threadIdx.x == 0) {
      float e = 0.f;
#pragma unroll
      for (int w = 0; w < kLfWg / 64; ++w) e = fmaf(p1024, e, s_wave_end[w]);
      ends[row * n_chunks + chunk] = e;
    }
    return;
  }

  float carry = 0.f;                                        // y just before the chunk
  if (chunk > 0) {
    float pw_chunk[6];
    const float p2048 = p1024 * p1024;
    pw_chunk[0] = p2048 * p2048;
#pragma unroll
    for (int b = 1; b < 6; ++b) pw_chunk[b] = pw_chunk[b - 1] * pw_chunk[b - 1];
    const float p_round = pw_chunk[5] * pw_chunk[5];        // p^(4096 64)
    const float* e_row = ends + row * n_chunks;
    for (int64_t first = chunk - (chunk + 63) / 64 * 64; first < chunk; first += 64) {
      const int64_t k = first + lane;
      const float e = lf_wave_scan(k >= 0 ? e_row[k] : 0.f, pw_chunk, lane);
      carry = fmaf(p_round, carry, __shfl(e, 63));
    }
  }
  for (int w = 0; w < wave; ++w) carry = fmaf(p1024, carry, s_wave_end[w]);      // ... before the wave
  float p_lane = 1.f;                                       // p^(16 lane)
#pragma unroll
  for (int b = 0; b < 6; ++b)
    if ((lane >> b) & 1) p_lane *= pw_lane[b];
  const float excl = __shfl_up(incl, 1);
  carry = fmaf(p_lane, carry, lane ? excl : 0.f);           // ... before the run

  float pi = p;
#pragma unroll
  for (int i = 0; i < kLfRun; ++i) {
    local[i] = fmaf(pi, carry, local[i]);
    pi *= p;
  }
  float* yr = y + row * y_row_stride;
  lf_store_run(yr + r.s, lf_head(yr), r.cnt, local);
}

// ---- Normalize: y = x / max(||x||_p, eps) per row, p in {inf, 1, 2} ------------------------------------------------------------
// Two launches over the same chunks.  The first leaves one partial per chunk in the workspace (max |x|, sum |x| or sum x^2: the lane's run
// in order, a butterfly over the wave, the four waves in order); the second has every wave add up its row's partials in one fixed order
// (lane l takes partials l, l + 64, ... in turn, then the same butterfly) and divides its chunk - a true division, as torch's.
template <int P>
__device__ __forceinline__ float nrm_join(float a, float b) { return P == 0 ? fmaxf(a, b) : a + b; }

template <int P>
__device__ __forceinline__ float nrm_wave(float a) { return P == 0 ? wave_max(a) : wave_sum(a); }

template <int P>
__global__ __launch_bounds__(kLfWg) void row_norm_partial_kernel(const float* __restrict__ x, int64_t x_row_stride, int64_t n, int64_t n_chunks,
                                                                float* __restrict__ partial) {
  __shared__ float s_wave[kLfWg / 64];
  const int64_t row = blockIdx.x / n_chunks, chunk = blockIdx.x % n_chunks;
  const float* xr = x + row * x_row_stride;
  const int64_t s = chunk * kLfChunk + (int64_t)threadIdx.x * kLfRun;
  float v[kLfRun];
  lf_load_run(xr + s, lf_head(xr), n - s, v);
  float a = 0.f;
#pragma unroll
  for (int i = 0; i < kLfRun; ++i) a = P == 0 ? fmaxf(a, fabsf(v[i])) : (P == 1 ? a + fabsf(v[i]) : fmaf(v[i], v[i], a));
  a = nrm_wave<P>(a);
  if ((threadIdx.x & 63) == 0) s_wave[threadIdx.x >> 6] = a;
  __syncthreads();
  if (threadIdx.x == 0) {
    float t = s_wave[0];
#pragma unroll
    for (int w = 1; w < kLfWg / 64; ++w) t = nrm_join<P>(t, s_wave[w]);
    partial[row * n_chunks + chunk] = t;
  }
}

template <int P>
__global__ __launch_bounds__(kLfWg) void row_norm_scale_kernel(const float* __restrict__ x, int64_t x_row_stride, int64_t n, int64_t n_chunks,
                                                              float eps, const float* __restrict__ partial, float* __restrict__ y,
                                                              int64_t y_row_stride) {
  const int64_t row = blockIdx.x / n_chunks, chunk = blockIdx.x % n_chunks;
  const int lane = threadIdx.x & 63;
  const float* xr = x + row * x_row_stride;
  const int64_t s = chunk * kLfChunk + (int64_t)threadIdx.x * kLfRun;
  float v[kLfRun];
  lf_load_run(xr + s, lf_head(xr), n - s, v);
  float a = 0.f;
  for (int64_t k = lane; k < n_chunks; k += 64) a = nrm_join<P>(a, partial[row * n_chunks + k]);
  a = nrm_wave<P>(a);
  const float denom = fmaxf(P == 2 ? sqrtf(a) : a, eps);
#pragma unroll
  for (int i = 0; i < kLfRun; ++i) v[i] = v[i] / denom;
  float* yr = y + row * y_row_stride;
  lf_store_run(yr + s, lf_head(yr), n - s, v);
}

static int chunks_check(const char* what, const void* x, int64_t x_row_stride, int32_t batch, int64_t n, const void* y, int64_t y_row_stride,
                        int64_t* n_chunks) {
  MMK_TRY(rows_check(what, x, x_row_stride, batch, n, y, y_row_stride, n, true));
  *n_chunks = (n + kLfChunk - 1) / kLfChunk;
  if (*n_chunks * batch > 0x7fffffffLL)
    return fail(MMK_ERR_UNSUPPORTED, "%s: %lld chunks of %d samples are more than one launch takes", what, (long long)(*n_chunks * batch), kLfChunk);
  return MMK_OK;
}

}  // namespace mmk

extern "C" size_t mmk_lfilter1_workspace_floats(int32_t batch, int64_t n) {
  if (batch <= 0 || n <= 0) return 0;
  return (size_t)batch * (size_t)((n + MMK_LFILTER1_CHUNK - 1) / MMK_LFILTER1_CHUNK);
}

extern "C" int mmk_lfilter1_f32(const float* x, int64_t x_row_stride, int32_t batch, int64_t n, float b0, float b1, float a1, float* y,
                                int64_t y_row_stride, float* workspace, mmk_stream_t stream) {
  using namespace mmk;
  int64_t n_chunks = 0;
  MMK_TRY(chunks_check("lfilter1", x, x_row_stride, batch, n, y, y_row_stride, &n_chunks));
  if (!(fabsf(a1) <= 1.f))
    return fail(MMK_ERR_UNSUPPORTED, "lfilter1: |a1| = %g > 1 (the chunk powers a1^4096 .. of an unstable section overflow)", (double)fabsf(a1));
  const unsigned grid = (unsigned)(n_chunks * batch);
  if (a1 == 0.f)
    return launch(lfilter1_fir_kernel, dim3(grid), dim3(kLfWg), 0, (hipStream_t)stream, x, x_row_stride, n, n_chunks, b0, b1, y, y_row_stride);
  if (n_chunks > 1) {
    if (!workspace) return fail(MMK_ERR_WORKSPACE, "lfilter1: a row of %lld samples needs mmk_lfilter1_workspace_floats() floats", (long long)n);
    MMK_TRY(launch(lfilter1_scan_kernel<false>, dim3((unsigned)((n_chunks - 1) * batch)), dim3(kLfWg), 0, (hipStream_t)stream, x, x_row_stride, n,
                   n_chunks, n_chunks - 1, b0, b1, -a1, (float*)nullptr, (int64_t)0, workspace));
  }
  return launch(lfilter1_scan_kernel<true>, dim3(grid), dim3(kLfWg), 0, (hipStream_t)stream, x, x_row_stride, n, n_chunks, n_chunks, b0, b1, -a1,
                y, y_row_stride, workspace);
}

extern "C" size_t mmk_row_normalize_workspace_floats(int32_t batch, int64_t n) { return mmk_lfilter1_workspace_floats(batch, n); }

extern "C" int mmk_row_normalize_f32(const float* x, int64_t x_row_stride, int32_t batch, int64_t n, int32_t p, float eps, float* y,
                                     int64_t y_row_stride, float* workspace, mmk_stream_t stream) {
  using namespace mmk;
  int64_t n_chunks = 0;
  MMK_TRY(chunks_check("row_normalize", x, x_row_stride, batch, n, y, y_row_stride, &n_chunks));
  if (p < 0 || p > 2) return fail(MMK_ERR_UNSUPPORTED, "row_normalize: p must be 0 (inf), 1 or 2, got %d", p);
  if (!workspace) return fail(MMK_ERR_WORKSPACE, "row_normalize: needs mmk_row_normalize_workspace_floats() floats");
  const dim3 grid((unsigned)(n_chunks * batch)), wg(kLfWg);
  hipStream_t st = (hipStream_t)stream;
#define MMK_NRM_LAUNCH(P)                                                                                                \
  MMK_TRY(launch(row_norm_partial_kernel<P>, grid, wg, 0, st, x, x_row_stride, n, n_chunks, workspace));                 \
  return launch(row_norm_scale_kernel<P>, grid, wg, 0, st, x, x_row_stride, n, n_chunks, eps, workspace, y, y_row_stride)
  if (p == 0) { MMK_NRM_LAUNCH(0); }
  else if (p == 1) { MMK_NRM_LAUNCH(1); }
  else { MMK_NRM_LAUNCH(2); }
#undef MMK_NRM_LAUNCH
}
