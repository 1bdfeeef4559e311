// The k nearest frames of every frame (mimikit/extract/clusters.py:27-98 QCluster; any k-nearest-neighbour graph): a GEMM whose epilogue keeps
// the T best corpus frames of every query row and which never writes the matrix.
//
//   nn_topk_kernel<TC, kSelf>   key[r, j] = clamp((<x_r, y_j> * qscale[r]) * cscale[j] + cshift[j], key_min, key_max), three separate roundings
//                         after the sum (no contraction); the limits are the caller's, -inf and +inf for none: the euclidean key has no
//                         range, a cosine is clamped to [-1, 1] as nn_cosine_kernel clamps it - where k = 1 every cosine is +-1 give or
//                         take an ulp, and only the clamp makes those a tie that the lower index wins.
//                         The tile walk is nn_cosine_kernel's (neighbors.hip), statement for statement: 128 query
//                         rows by one span of MMK_NN_SPAN corpus frames in tiles of 128, 2 x 2 products of v_mfma_f32_32x32x2_f32 per wave,
//                         operands through LDS in chunks of 32 bins with the SAME permutation of the bins - two identical corpus frames have
//                         bit-identical keys, and the sums are those of nn_cosine_kernel bit for bit.  The kernel is a separate one, not a
//                         shared header: the two existing instances stay exactly as they were compiled.
//                         A lane keeps, for each of its two query rows, a list of TC (key, index) pairs in registers, sorted by falling key,
//                         across the whole span.  A lane meets its frames in rising index order, so "strictly greater than the list's last
//                         key" is the whole guard: one compare per candidate once the list has filled with good keys, and an insertion (the
//                         new pair replaces the last and rises by compare-and-swap, all register numbers fixed at compile time) only behind
//                         that branch.  Equal keys keep the earlier, lower index in front.  Empty slots hold (-inf, int max).
//                         At the end of the span the four lists of a query row are merged by "greater key, then lower index": the other
//                         half-wave's list arrives by shuffles and is pushed into the lane's own, then the two waves that share the rows leave
//                         their lists in LDS (the operands' LDS, free by then) and one thread per row walks the two with two cursors.  The
//                         first T pairs go to the workspace, span-major: key[span][row][T] floats, then index[span][row][T] int32.
//                         TC is the list's capacity, the smallest of 1, 4, 8, 16 that holds T.
//   nn_topk_merge_kernel<TC>    one thread per query row pushes the spans' lists into one list in rising span order (strictly greater wins:
//                         the lower index stays in front; a span's list is left at its first pair that does not enter) and writes
//                         index (rows, T) int64 and key (rows, T) fp32; empty slots leave as (-1, -inf).
//   half_neg_sqnorm_kernel      cshift of the euclidean metric: -|y_j|^2 / 2, a wave per row, the squares added in fp64 in one fixed order
//                         and rounded to fp32 once.  With scales 1 the largest key <x, y> - |y|^2 / 2 is the smallest |x - y|^2.
// No atomics, no workgroup waits for another; two calls give the same bits.  NaN and inf in the inputs are not handled (a key of -inf never
// enters a list).
#include "mmk_common.h"

namespace mmk {

typedef float tk_f32x4 __attribute__((ext_vector_type(4)));
typedef float tk_f32x16 __attribute__((ext_vector_type(16)));

constexpr int kTkSpan = MMK_NN_SPAN;
constexpr int kTkThreads = 256;
constexpr int kTkRows = 128;      // query rows of a workgroup, 64 per wave pair
constexpr int kTkCols = 128;      // corpus frames of a tile, 64 per wave pair
constexpr int kTkKC = 32;         // bins per LDS chunk
constexpr int kTkPitch = 36;      // floats between LDS rows (neighbors.hip: kNnPitch)
constexpr int kTkGroup = 16;      // query blocks that are in flight together
constexpr int kTkLoads = (kTkRows + kTkCols) / 8;
constexpr int kTkEmpty = 0x7fffffff;
static_assert(kTkSpan % kTkCols == 0, "a span is a whole number of tiles");
static_assert(MMK_NN_TOPK_MAX == 16, "the list capacities below end at 16");
static_assert(2 * MMK_NN_TOPK_MAX * kTkRows <= kTkCols * kTkPitch, "the two waves' lists of a span fit the LDS of one operand");

__device__ __forceinline__ bool tk_better(float v, int j, float bv, int bj) { return v > bv || (v == bv && j < bj); }

// (c, j) takes the last place of the sorted list and rises.  kTies: equal keys are ordered by index as well (a merge of lists whose indices
// interleave); without it an equal key stays behind (the candidates arrive in rising index order).  The caller has tested the guard.
template <int TC, bool kTies>
__device__ __forceinline__ void tk_push(float (&key)[TC], int (&idx)[TC], float c, int j) {
  key[TC - 1] = c;
  idx[TC - 1] = j;
#pragma unroll
  for (int p = TC - 1; p > 0; --p) {
    const bool up = kTies ? tk_better(key[p], idx[p], key[p - 1], idx[p - 1]) : key[p] > key[p - 1];
    const float k_hi = up ? key[p] : key[p - 1], k_lo = up ? key[p - 1] : key[p];
    const int j_hi = up ? idx[p] : idx[p - 1], j_lo = up ? idx[p - 1] : idx[p];
    key[p - 1] = k_hi;
    key[p] = k_lo;
    idx[p - 1] = j_hi;
    idx[p] = j_lo;
  }
}

template <int TC, bool kSelf>
__global__ __launch_bounds__(kTkThreads, 2) void nn_topk_kernel(const float* __restrict__ x, int64_t x_row_stride, const float* __restrict__ qscale,
                                                              int64_t rows, const float* __restrict__ y, int64_t y_row_stride,
                                                              const float* __restrict__ cscale, const float* __restrict__ cshift, float key_min,
                                                              float key_max, int64_t M, int32_t K, int32_t T, int32_t n_blocks, int32_t n_spans,
                                                              float* __restrict__ ws_key, int32_t* __restrict__ ws_idx) {
  __shared__ __attribute__((aligned(16))) float ys[kTkCols * kTkPitch];
  __shared__ __attribute__((aligned(16))) float xs[kTkRows * kTkPitch];
  __shared__ float css[2][kTkCols];
  __shared__ float shs[2][kTkCols];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int col = tid & 31, row0 = tid >> 5;       // loads: bin `col` of rows row0, row0 + 8, ...
  const int fr = lane & 31, fh = lane >> 5;         // MFMA fragments: row / column fr, bin half fh
  const int wm = wave & 1, wn = wave >> 1;          // this wave's corpus half and query half of the tile

  // workgroup -> (query block, span): groups of kTkGroup query blocks by all spans, the query block fastest
  const int per_group = kTkGroup * n_spans;
  const int group = blockIdx.x / per_group, within = blockIdx.x % per_group;
  const int gsize = min(kTkGroup, n_blocks - group * kTkGroup);
  const int block = group * kTkGroup + within % gsize, span = within / gsize;
  if (span >= n_spans) return;                      // (the last group is smaller: its surplus workgroups have nothing to do)
  const int64_t rbase = (int64_t)block * kTkRows;
  const int64_t jbeg = (int64_t)span * kTkSpan;
  const int64_t jend = jbeg + kTkSpan < M ? jbeg + kTkSpan : M;

  float qs[2];
#pragma unroll
  for (int tn = 0; tn < 2; ++tn) {
    const int64_t r = rbase + wn * 64 + tn * 32 + fr;
    qs[tn] = r < rows ? qscale[r] : 0.f;
  }
  const float ninf = __int_as_float(0xff800000);
  float key[2][TC];
  int idx[2][TC];
#pragma unroll
  for (int tn = 0; tn < 2; ++tn)
#pragma unroll
    for (int p = 0; p < TC; ++p) {
      key[tn][p] = ninf;
      idx[tn][p] = kTkEmpty;
    }

  int parity = 0;
  for (int64_t jt = jbeg; jt < jend; jt += kTkCols, parity ^= 1) {
    if (tid < kTkCols) {
      const int64_t j = jt + tid;
      css[parity][tid] = j < jend ? cscale[j] : 0.f;
      shs[parity][tid] = j < jend ? cshift[j] : 0.f;
    }
    tk_f32x16 acc[2][2];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
      for (int b = 0; b < 2; ++b)
#pragma unroll
        for (int q = 0; q < 16; ++q) acc[a][b][q] = 0.f;

    float rg[kTkLoads];
    auto gload = [&](int k0) {
      const int k = k0 + col;
      const int kc = k < K ? k : K - 1;
#pragma unroll
      for (int i = 0; i < kTkCols / 8; ++i) {
        const int64_t j = jt + i * 8 + row0;
        rg[i] = y[(j < M ? j : M - 1) * y_row_stride + kc];
      }
#pragma unroll
      for (int i = 0; i < kTkRows / 8; ++i) {
        const int64_t r = rbase + i * 8 + row0;
        rg[kTkCols / 8 + i] = x[(r < rows ? r : rows - 1) * x_row_stride + kc];
      }
    };
    gload(0);
    for (int k0 = 0; k0 < K; k0 += kTkKC) {
      const bool kin = k0 + col < K;
#pragma unroll
      for (int i = 0; i < kTkCols / 8; ++i) ys[(i * 8 + row0) * kTkPitch + col] = (kin && jt + i * 8 + row0 < jend) ? rg[i] : 0.f;
#pragma unroll
      for (int i = 0; i < kTkRows / 8; ++i)
        xs[(i * 8 + row0) * kTkPitch + col] = (kin && rbase + i * 8 + row0 < rows) ? rg[kTkCols / 8 + i] : 0.f;
      __syncthreads();
      if (k0 + kTkKC < K) gload(k0 + kTkKC);
#pragma unroll
      for (int g = 0; g < kTkKC; g += 8) {
        tk_f32x4 av[2], bv[2];
#pragma unroll
        for (int t = 0; t < 2; ++t) {
          av[t] = *reinterpret_cast<const tk_f32x4*>(&ys[(wm * 64 + t * 32 + fr) * kTkPitch + g + 4 * fh]);
          bv[t] = *reinterpret_cast<const tk_f32x4*>(&xs[(wn * 64 + t * 32 + fr) * kTkPitch + g + 4 * fh]);
        }
#pragma unroll
        for (int e = 0; e < 4; ++e)
#pragma unroll
          for (int tm = 0; tm < 2; ++tm)
#pragma unroll
            for (int tn = 0; tn < 2; ++tn) acc[tm][tn] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[tm][e], bv[tn][e], acc[tm][tn], 0, 0, 0);
      }
      __syncthreads();
    }

    // the tile's candidates, inside the lane and in rising frame order.  kSelf: self_jl is the tile's frame that IS this lane's first query
    // row (the second one's lies 32 further on) where the diagonal crosses the tile, and no frame of the tile anywhere else
    int self_jl = -64;
    if constexpr (kSelf) {
      if (jt < rbase + kTkRows && jt + kTkCols > rbase) self_jl = wn * 64 + fr - (int)(jt - rbase);
    }
#pragma unroll
    for (int tm = 0; tm < 2; ++tm)
#pragma unroll
      for (int q = 0; q < 16; ++q) {
        const int jl = wm * 64 + tm * 32 + (q & 3) + 8 * (q >> 2) + 4 * fh;
        const int64_t j = jt + jl;
        const float cs = css[parity][jl], sh = shs[parity][jl];
#pragma unroll
        for (int tn = 0; tn < 2; ++tn) {
          const float c = fminf(fmaxf(__fadd_rn(__fmul_rn(__fmul_rn(acc[tm][tn][q], qs[tn]), cs), sh), key_min), key_max);
          bool take = j < jend && c > key[tn][TC - 1];
          if constexpr (kSelf) take = take && jl != self_jl + tn * 32;
          if (take) tk_push<TC, false>(key[tn], idx[tn], c, (int)j);
        }
      }
  }

  // the other half of the wave holds the same query rows against other frames: its list is pushed into this one (both halves end up with
  // the same list), then the two waves that share these query rows leave theirs in LDS, slot-major: [wave half][slot][row]
  float* red_key = ys;                                // (every read of the operands lies before the K loop's last barrier)
  int* red_idx = reinterpret_cast<int*>(xs);
#pragma unroll
  for (int tn = 0; tn < 2; ++tn) {
    float ok[TC];
    int oj[TC];
#pragma unroll
    for (int p = 0; p < TC; ++p) {
      ok[p] = __shfl_xor(key[tn][p], 32);
      oj[p] = __shfl_xor(idx[tn][p], 32);
    }
#pragma unroll
    for (int p = 0; p < TC; ++p)
      if (tk_better(ok[p], oj[p], key[tn][TC - 1], idx[tn][TC - 1])) tk_push<TC, true>(key[tn], idx[tn], ok[p], oj[p]);
    if (fh == 0) {
#pragma unroll
      for (int p = 0; p < TC; ++p) {
        red_key[(wm * TC + p) * kTkRows + wn * 64 + tn * 32 + fr] = key[tn][p];
        red_idx[(wm * TC + p) * kTkRows + wn * 64 + tn * 32 + fr] = idx[tn][p];
      }
    }
  }
  __syncthreads();
  if (tid < kTkRows && rbase + tid < rows) {
    const int64_t out = ((int64_t)span * rows + rbase + tid) * T;
    int a = 0, b = 0;                                 // a + b = p < T <= TC: both cursors stay inside their lists
    for (int p = 0; p < T; ++p) {
      const float ka = red_key[a * kTkRows + tid], kb = red_key[(TC + b) * kTkRows + tid];
      const int ja = red_idx[a * kTkRows + tid], jb = red_idx[(TC + b) * kTkRows + tid];
      const bool second = tk_better(kb, jb, ka, ja);
      ws_key[out + p] = second ? kb : ka;
      ws_idx[out + p] = second ? jb : ja;
      a += second ? 0 : 1;
      b += second ? 1 : 0;
    }
  }
}

template <int TC>
__global__ __launch_bounds__(256) void nn_topk_merge_kernel(const float* __restrict__ ws_key, const int32_t* __restrict__ ws_idx, int64_t rows,
                                                            int32_t T, int32_t n_spans, int64_t* __restrict__ index,
                                                            float* __restrict__ key_out) {
  const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= rows) return;
  float key[TC];
  int idx[TC];
#pragma unroll
  for (int p = 0; p < TC; ++p) {
    key[p] = __int_as_float(0xff800000);
    idx[p] = kTkEmpty;
  }
  for (int s = 0; s < n_spans; ++s) {
    const int64_t at = ((int64_t)s * rows + r) * T;
    for (int p = 0; p < T; ++p) {
      const float c = ws_key[at + p];
      if (!(c > key[TC - 1])) break;                  // (the span's list falls: nothing behind this pair enters either)
      tk_push<TC, false>(key, idx, c, ws_idx[at + p]);
    }
  }
#pragma unroll
  for (int p = 0; p < TC; ++p)
    if (p < T) {
      index[r * T + p] = idx[p] == kTkEmpty ? (int64_t)-1 : (int64_t)idx[p];
      key_out[r * T + p] = key[p];
    }
}

__global__ __launch_bounds__(256) void half_neg_sqnorm_kernel(const float* __restrict__ y, int64_t y_row_stride, int64_t rows, int32_t K,
                                                              float* __restrict__ out) {
  const int lane = threadIdx.x & 63;
  const int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  const float* row = y + (r < rows ? r : rows - 1) * y_row_stride;
  double acc = 0.0;
  for (int k = lane; k < K; k += 64) {
    const double v = (double)row[k];
    acc = fma(v, v, acc);
  }
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) acc += __shfl_xor(acc, off);
  if (lane == 0 && r < rows) out[r] = (float)(-0.5 * acc);
}

static int tk_spans(int64_t m) { return (int)((m + kTkSpan - 1) / kTkSpan); }

template <int TC>
static int tk_launch(bool self, const float* x, int64_t x_row_stride, const float* qscale, int64_t rows, const float* y, int64_t y_row_stride,
                     const float* cscale, const float* cshift, float key_min, float key_max, int64_t m, int32_t k, int32_t t, int64_t* index,
                     float* key, void* workspace, hipStream_t st) {
  const int n_spans = tk_spans(m);
  const int64_t n_blocks = (rows + kTkRows - 1) / kTkRows;
  const int64_t groups = (n_blocks + kTkGroup - 1) / kTkGroup;
  const int64_t grid = groups * kTkGroup * n_spans;
  if (grid > 0x7fffffffLL)
    return fail(MMK_ERR_UNSUPPORTED, "nn_topk: %lld rows against %lld frames are more than one launch takes", (long long)rows, (long long)m);
  float* ws_key = static_cast<float*>(workspace);
  int32_t* ws_idx = reinterpret_cast<int32_t*>(ws_key + rows * n_spans * t);
  if (self)
    hipLaunchKernelGGL((nn_topk_kernel<TC, true>), dim3((unsigned)grid), dim3(kTkThreads), 0, st, x, x_row_stride, qscale, rows, y, y_row_stride,
                       cscale, cshift, key_min, key_max, m, k, t, (int32_t)n_blocks, n_spans, ws_key, ws_idx);
  else
    hipLaunchKernelGGL((nn_topk_kernel<TC, false>), dim3((unsigned)grid), dim3(kTkThreads), 0, st, x, x_row_stride, qscale, rows, y, y_row_stride,
                       cscale, cshift, key_min, key_max, m, k, t, (int32_t)n_blocks, n_spans, ws_key, ws_idx);
  MMK_HIP(hipGetLastError());
  hipLaunchKernelGGL(nn_topk_merge_kernel<TC>, dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, st, ws_key, ws_idx, rows, t, n_spans, index,
                     key);
  MMK_HIP(hipGetLastError());
  return MMK_OK;
}

}  // namespace mmk

extern "C" size_t mmk_nn_topk_workspace_bytes(int64_t rows, int64_t m, int32_t t) {
  using namespace mmk;
  if (rows < 1 || m < 1 || t < 1 || t > MMK_NN_TOPK_MAX) return 0;
  return (size_t)rows * (size_t)tk_spans(m) * (size_t)t * (sizeof(float) + sizeof(int32_t));
}

extern "C" int mmk_nn_topk_f32(const float* x, int64_t x_row_stride, const float* qscale, int64_t rows, const float* y, int64_t y_row_stride,
                               const float* cscale, const float* cshift, float key_min, float key_max, int64_t m, int32_t k, int32_t t,
                               int32_t self_exclude, int64_t* index, float* key, void* workspace, size_t workspace_bytes, mmk_stream_t stream) {
  using namespace mmk;
  if (rows < 1) return fail(MMK_ERR_INVALID, "nn_topk: rows = %lld < 1 (query frames)", (long long)rows);
  if (m < 1) return fail(MMK_ERR_INVALID, "nn_topk: m = %lld < 1 (corpus frames)", (long long)m);
  if (k < 1) return fail(MMK_ERR_INVALID, "nn_topk: k = %d < 1 (bins)", k);
  if (t < 1) return fail(MMK_ERR_INVALID, "nn_topk: t = %d < 1 (neighbours kept per row)", t);
  if (!(key_min < key_max)) return fail(MMK_ERR_INVALID, "nn_topk: key_min = %g must lie below key_max = %g (-inf and +inf: no clamp)", key_min, key_max);
  if (t > MMK_NN_TOPK_MAX)
    return fail(MMK_ERR_UNSUPPORTED, "nn_topk: t = %d neighbours per row, more than the %d (MMK_NN_TOPK_MAX) a lane keeps in registers", t,
                MMK_NN_TOPK_MAX);
  if (m > 0x7fffffffLL - kTkSpan)
    return fail(MMK_ERR_UNSUPPORTED, "nn_topk: m = %lld corpus frames: indices are kept in 32 bits across the spans", (long long)m);
  if (self_exclude && (m != rows || y != x || y_row_stride != x_row_stride))
    return fail(MMK_ERR_INVALID, "nn_topk: self_exclude takes the corpus = the queries (y == x, the same stride, m == rows = %lld, got m = %lld)",
                (long long)rows, (long long)m);
  if (!x || !y || !qscale || !cscale || !cshift || !index || !key || !workspace || x_row_stride < 0 || y_row_stride < 0)
    return fail(MMK_ERR_INVALID, "nn_topk: bad arguments (null pointer or negative stride %lld / %lld)", (long long)x_row_stride,
                (long long)y_row_stride);
  if ((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(y) | reinterpret_cast<uintptr_t>(qscale) | reinterpret_cast<uintptr_t>(cscale) |
       reinterpret_cast<uintptr_t>(cshift) | reinterpret_cast<uintptr_t>(key) | reinterpret_cast<uintptr_t>(workspace)) & 3)
    return fail(MMK_ERR_INVALID, "nn_topk: x, y, qscale, cscale, cshift, key and the workspace must be 4-byte aligned");
  if (reinterpret_cast<uintptr_t>(index) & 7) return fail(MMK_ERR_INVALID, "nn_topk: index must be 8-byte aligned");
  if (workspace_bytes < mmk_nn_topk_workspace_bytes(rows, m, t))
    return fail(MMK_ERR_WORKSPACE, "nn_topk: the workspace has %zu bytes, %zu are needed", workspace_bytes,
                mmk_nn_topk_workspace_bytes(rows, m, t));
  hipStream_t st = (hipStream_t)stream;
  const bool self = self_exclude != 0;
  if (t == 1) return tk_launch<1>(self, x, x_row_stride, qscale, rows, y, y_row_stride, cscale, cshift, key_min, key_max, m, k, t, index, key, workspace, st);
  if (t <= 4) return tk_launch<4>(self, x, x_row_stride, qscale, rows, y, y_row_stride, cscale, cshift, key_min, key_max, m, k, t, index, key, workspace, st);
  if (t <= 8) return tk_launch<8>(self, x, x_row_stride, qscale, rows, y, y_row_stride, cscale, cshift, key_min, key_max, m, k, t, index, key, workspace, st);
  return tk_launch<16>(self, x, x_row_stride, qscale, rows, y, y_row_stride, cscale, cshift, key_min, key_max, m, k, t, index, key, workspace, st);
}

extern "C" int mmk_half_neg_sqnorm_f32(const float* y, int64_t y_row_stride, int64_t rows, int32_t k, float* out, mmk_stream_t stream) {
  using namespace mmk;
  if (rows < 1 || k < 1) return fail(MMK_ERR_INVALID, "half_neg_sqnorm: rows = %lld, k = %d (both at least 1)", (long long)rows, k);
  if ((rows + 3) / 4 > 0x7fffffffLL) return fail(MMK_ERR_UNSUPPORTED, "half_neg_sqnorm: %lld rows are more than one launch takes", (long long)rows);
  if (!y || !out || y_row_stride < 0 || ((reinterpret_cast<uintptr_t>(y) | reinterpret_cast<uintptr_t>(out)) & 3))
    return fail(MMK_ERR_INVALID, "half_neg_sqnorm: bad arguments (null or misaligned pointer, negative stride %lld)", (long long)y_row_stride);
  hipLaunchKernelGGL(half_neg_sqnorm_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, (hipStream_t)stream, y, y_row_stride, rows, k, out);
  MMK_HIP(hipGetLastError());
  return MMK_OK;
}
