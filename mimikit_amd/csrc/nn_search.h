// The best corpus frames of every query frame: a GEMM whose epilogue keeps the TC best keys of every row and which never writes the matrix.
// ONE kernel for the self-excluding nearest-frame search (neighbors.hip: mmk_nn_cosine_self_f32 - TC = 1, the cosine key) and the k-best
// search (qcluster.hip: mmk_nn_topk_f32 - TC = 1, 4, 8, 16, the affine key).  The plain nearest-frame search (mmk_nn_cosine_f32) keeps
// nn_cosine_kernel of neighbors.hip, a kernel of its own for the reason given there; it uses the constants, nn_better and
// nn_merge_kernel<1> of this header.  How the bins are walked - staging, fragments, products, the accumulator's rows - is frame_walk.h.
//
//   nn_search_kernel<TC, kSelf, Key>   key[r, j] = Key::key(<x_r, y_j>, ...) for `rows` query frames against m corpus frames over k bins.
//                         A workgroup of four waves owns kNnRows = 128 query rows and one SPAN of MMK_NN_SPAN corpus frames, which it
//                         walks in tiles of kNnCols = 128 frames; a wave owns a 64 x 64 corner of the tile as 2 x 2 products with
//                         A = corpus frames and B = query rows: the query row on the lane and 16 corpus frames in the registers, so a
//                         tile's candidates are met inside the lane, in rising frame order.  Two identical corpus frames have
//                         bit-identical keys, under either key and any TC (frame_walk.h: one order of the sum).
//                         A lane keeps, for each of its two query rows, a list of TC (key, index) pairs in registers, sorted by falling key,
//                         across the whole span.  It meets its frames in rising index order, so "strictly greater than the list's last
//                         key" is the whole guard: one compare per candidate once the list has filled with good keys, and an insertion (the
//                         new pair replaces the last and rises by compare-and-swap, all register numbers fixed at compile time; with
//                         TC = 1 an assignment: the arg-max) only behind that branch.  Equal keys keep the earlier, lower index in front.
//                         Empty slots hold (-inf, int max).
//                         At the end of the span the four lists of a query row are merged by "greater key, then lower index": the other
//                         half-wave's list arrives by shuffles and is pushed into the lane's own, then the two waves that share the rows leave
//                         their lists in LDS (the operands' LDS, free by then) and one thread per row walks the two with two cursors.  The
//                         first T pairs go to the workspace, span-major: key[span][row][T] floats, then index[span][row][T] int32.
//                         Workgroups are numbered so that those in flight together share few query blocks and few spans (kNnGroup query
//                         blocks by all spans, query block fastest).
//                         kSelf: the corpus IS the queries (the host passes y = x, m = rows) and frame r is left out of row r's list.
//                         The instances fill the 256 registers of two waves per SIMD; what does not fit (the lists, from TC = 8 on) lies
//                         in scratch while the products run, read and written once per tile outside the loop over the bins.
//   nn_merge_kernel<TC>   one thread per query row pushes the spans' lists into one list in rising span order (strictly greater wins:
//                         the lower index stays in front; a span's list is left at its first pair that does not enter) and writes
//                         index (rows, T) int64 and key (rows, T) fp32; empty slots leave as (-1, -inf).
// No atomics, no workgroup waits for another; every sum has one order, so two calls give the same bits.  NaN in the inputs is not handled
// (> drops it silently; a key of -inf never enters a list).
#pragma once
#include "entry_util.h"
#include "frame_walk.h"

namespace mmk {

constexpr int kNnSpan = MMK_NN_SPAN;
constexpr int kNnThreads = 256;
constexpr int kNnRows = 128;      // query rows of a workgroup, 64 per wave pair
constexpr int kNnCols = 128;      // corpus frames of a tile, 64 per wave pair
constexpr int kNnGroup = 16;      // query blocks that are in flight together
constexpr int kNnLoads = (kNnRows + kNnCols) / 8;      // dwords a thread loads per chunk
constexpr int kNnEmpty = 0x7fffffff;
static_assert(kNnSpan % kNnCols == 0, "a span is a whole number of tiles");
static_assert(kNnRows == 128 && kNnCols == 128 && kNnThreads == 256, "four waves, each a 64 x 64 corner of 2 x 2 MFMA products");
static_assert(MMK_NN_TOPK_MAX == 16, "the list capacities end at 16");
static_assert(2 * MMK_NN_TOPK_MAX * kNnRows <= kNnCols * kFwPitch, "the two waves' lists of a span fit the LDS of one operand");

// What the epilogue makes of a sum, and the per-frame vectors it needs: a kernel argument, so an instance carries its own key's data and no
// other.  `row` is the query row's factor (in a register across the span), `cs` and - where kShift - `sh` are the corpus frame's scale[j] and
// shift[j], staged in LDS per tile.  A key without a shift stages and reads none and adds no zero (-0.f stays -0.f).
struct NnCosineKey {      // clamp(<x, y> rx ry, -1, 1): no shift, and its limits are constants
  const float* __restrict__ scale;
  static constexpr bool kShift = false;
  __device__ __forceinline__ float key(float acc, float row, float cs, float) const { return fminf(fmaxf(acc * row * cs, -1.f), 1.f); }
};
struct NnAffineKey {      // clamp((<x, y> qscale) scale + shift, lo, hi), three separate roundings after the sum (no contraction);
  const float* __restrict__ scale;      // the limits are the caller's, -inf and +inf for none
  const float* __restrict__ shift;
  float lo, hi;
  static constexpr bool kShift = true;
  __device__ __forceinline__ float key(float acc, float row, float cs, float sh) const {
    return fminf(fmaxf(__fadd_rn(__fmul_rn(__fmul_rn(acc, row), cs), sh), lo), hi);
  }
};

__device__ __forceinline__ bool nn_better(float v, int j, float bv, int bj) { return v > bv || (v == bv && j < bj); }

// (c, j) takes the last place of the sorted list and rises.  kTies: equal keys are ordered by index as well (a merge of lists whose indices
// interleave); without it an equal key stays behind (the candidates arrive in rising index order).  The caller has tested the guard.
template <int TC, bool kTies>
__device__ __forceinline__ void nn_push(float (&key)[TC], int (&idx)[TC], float c, int j) {
  key[TC - 1] = c;
  idx[TC - 1] = j;
#pragma unroll
  for (int p = TC - 1; p > 0; --p) {
    const bool up = kTies ? nn_better(key[p], idx[p], key[p - 1], idx[p - 1]) : key[p] > key[p - 1];
    const float k_hi = up ? key[p] : key[p - 1], k_lo = up ? key[p - 1] : key[p];
    const int j_hi = up ? idx[p] : idx[p - 1], j_lo = up ? idx[p - 1] : idx[p];
    key[p - 1] = k_hi;
    key[p] = k_lo;
    idx[p - 1] = j_hi;
    idx[p] = j_lo;
  }
}

template <int TC, bool kSelf, class Key>
__global__ __launch_bounds__(kNnThreads, 2) void nn_search_kernel(const float* __restrict__ x, int64_t x_row_stride, const float* __restrict__ qscale,
                                                                int64_t rows, const float* __restrict__ y, int64_t y_row_stride,
                                                                const Key kp, int64_t M, int32_t K, int32_t T, int32_t n_blocks, int32_t n_spans,
                                                                float* __restrict__ ws_key, int32_t* __restrict__ ws_idx) {
  __shared__ __attribute__((aligned(16))) float ys[kNnCols * kFwPitch];
  __shared__ __attribute__((aligned(16))) float xs[kNnRows * kFwPitch];
  __shared__ float css[2][kNnCols];                 // the tile's frames' scale and shift, two tiles deep;
  __shared__ float shs[2][kNnCols];                 // (an instance whose key has no shift never names shs, and it takes no LDS)
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int col = tid & 31, row0 = tid >> 5;       // loads: bin `col` of rows row0, row0 + 8, ...
  const int fr = lane & 31, fh = lane >> 5;         // MFMA fragments: row / column fr, bin half fh
  const int wm = wave & 1, wn = wave >> 1;          // this wave's corpus half and query half of the tile

  // workgroup -> (query block, span): groups of kNnGroup query blocks by all spans, the query block fastest
  const int per_group = kNnGroup * n_spans;
  const int group = blockIdx.x / per_group, within = blockIdx.x % per_group;
  const int gsize = min(kNnGroup, n_blocks - group * kNnGroup);
  const int block = group * kNnGroup + within % gsize, span = within / gsize;
  if (span >= n_spans) return;                      // (the last group is smaller: its surplus workgroups have nothing to do)
  const int64_t rbase = (int64_t)block * kNnRows;
  const int64_t jbeg = (int64_t)span * kNnSpan;
  const int64_t jend = jbeg + kNnSpan < M ? jbeg + kNnSpan : M;

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
      idx[tn][p] = kNnEmpty;
    }

  int parity = 0;
  for (int64_t jt = jbeg; jt < jend; jt += kNnCols, parity ^= 1) {
    if (tid < kNnCols) {
      const int64_t j = jt + tid;
      css[parity][tid] = j < jend ? kp.scale[j] : 0.f;
      if constexpr (Key::kShift) shs[parity][tid] = j < jend ? kp.shift[j] : 0.f;
    }
    fw_f32x16 acc[2][2];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
      for (int b = 0; b < 2; ++b)
#pragma unroll
        for (int q = 0; q < 16; ++q) acc[a][b][q] = 0.f;

    float rg[kNnLoads];
    auto gload = [&](int k0) {
      fw_load<kNnCols / 8, 8, 0>(rg, y, y_row_stride, jt, M, row0, col, k0, K);
      fw_load<kNnRows / 8, 8, kNnCols / 8>(rg, x, x_row_stride, rbase, rows, row0, col, k0, K);
    };
    gload(0);
    for (int k0 = 0; k0 < K; k0 += kFwKC) {
      const bool kin = k0 + col < K;
#pragma unroll
      for (int i = 0; i < kNnCols / 8; ++i) ys[(i * 8 + row0) * kFwPitch + col] = (kin && jt + i * 8 + row0 < jend) ? rg[i] : 0.f;
#pragma unroll
      for (int i = 0; i < kNnRows / 8; ++i)
        xs[(i * 8 + row0) * kFwPitch + col] = (kin && rbase + i * 8 + row0 < rows) ? rg[kNnCols / 8 + i] : 0.f;
      __syncthreads();
      if (k0 + kFwKC < K) gload(k0 + kFwKC);
#pragma unroll
      for (int g = 0; g < kFwKC; g += 8) {
        fw_f32x4 av[2], bv[2];
#pragma unroll
        for (int t = 0; t < 2; ++t) {
          av[t] = fw_frag(ys, wm * 64 + t * 32 + fr, g, fh);
          bv[t] = fw_frag(xs, wn * 64 + t * 32 + fr, g, fh);
        }
#pragma unroll
        for (int e = 0; e < 4; ++e)
#pragma unroll
          for (int tm = 0; tm < 2; ++tm)
#pragma unroll
            for (int tn = 0; tn < 2; ++tn) fw_mfma(acc[tm][tn], av[tm], bv[tn], e);
      }
      __syncthreads();
    }

    // the tile's candidates, inside the lane and in rising frame order.  kSelf: self_jl is the tile's frame that IS this lane's first query
    // row (the second one's lies 32 further on) where the diagonal crosses the tile, and no frame of the tile anywhere else - one epilogue,
    // since a second copy of it for the diagonal's tiles does not fit the registers
    int self_jl = -64;
    if constexpr (kSelf) {
      if (jt < rbase + kNnRows && jt + kNnCols > rbase) self_jl = wn * 64 + fr - (int)(jt - rbase);
    }
#pragma unroll
    for (int tm = 0; tm < 2; ++tm)
#pragma unroll
      for (int q = 0; q < 16; ++q) {
        const int jl = fw_acc_row(wm * 64 + tm * 32, q, fh);
        const int64_t j = jt + jl;
        const float cs = css[parity][jl];
        float sh = 0.f;
        if constexpr (Key::kShift) sh = shs[parity][jl];
#pragma unroll
        for (int tn = 0; tn < 2; ++tn) {
          const float c = kp.key(acc[tm][tn][q], qs[tn], cs, sh);
          bool take = j < jend && c > key[tn][TC - 1];
          if constexpr (kSelf) take = take && jl != self_jl + tn * 32;
          if (take) nn_push<TC, false>(key[tn], idx[tn], c, (int)j);
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
      if (nn_better(ok[p], oj[p], key[tn][TC - 1], idx[tn][TC - 1])) nn_push<TC, true>(key[tn], idx[tn], ok[p], oj[p]);
    if (fh == 0) {
#pragma unroll
      for (int p = 0; p < TC; ++p) {
        red_key[(wm * TC + p) * kNnRows + wn * 64 + tn * 32 + fr] = key[tn][p];
        red_idx[(wm * TC + p) * kNnRows + wn * 64 + tn * 32 + fr] = idx[tn][p];
      }
    }
  }
  __syncthreads();
  if (tid < kNnRows && rbase + tid < rows) {
    const int64_t out = ((int64_t)span * rows + rbase + tid) * T;
    int a = 0, b = 0;                                 // a + b = p < T <= TC: both cursors stay inside their lists
    for (int p = 0; p < T; ++p) {
      const float ka = red_key[a * kNnRows + tid], kb = red_key[(TC + b) * kNnRows + tid];
      const int ja = red_idx[a * kNnRows + tid], jb = red_idx[(TC + b) * kNnRows + tid];
      const bool second = nn_better(kb, jb, ka, ja);
      ws_key[out + p] = second ? kb : ka;
      ws_idx[out + p] = second ? jb : ja;
      a += second ? 0 : 1;
      b += second ? 1 : 0;
    }
  }
}

template <int TC>
__global__ __launch_bounds__(256) void nn_merge_kernel(const float* __restrict__ ws_key, const int32_t* __restrict__ ws_idx, int64_t rows, int32_t T,
                                                       int32_t n_spans, int64_t* __restrict__ index, float* __restrict__ key_out) {
  const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= rows) return;
  float key[TC];
  int idx[TC];
#pragma unroll
  for (int p = 0; p < TC; ++p) {
    key[p] = __int_as_float(0xff800000);
    idx[p] = kNnEmpty;
  }
  for (int s = 0; s < n_spans; ++s) {
    const int64_t at = ((int64_t)s * rows + r) * T;
    for (int p = 0; p < T; ++p) {
      const float c = ws_key[at + p];
      if (!(c > key[TC - 1])) break;                  // (the span's list falls: nothing behind this pair enters either)
      nn_push<TC, false>(key, idx, c, ws_idx[at + p]);
    }
  }
#pragma unroll
  for (int p = 0; p < TC; ++p)
    if (p < T) {
      index[r * T + p] = idx[p] == kNnEmpty ? (int64_t)-1 : (int64_t)idx[p];
      key_out[r * T + p] = key[p];
    }
}

static inline int nn_spans(int64_t m) { return (int)((m + kNnSpan - 1) / kNnSpan); }

// the two launches of one call.  kSelf: y = x, m = rows.  The workspace holds rows x spans x t keys, then as many int32 indices.
template <int TC, bool kSelf, class Key>
static int nn_search_launch(const char* who, const float* x, int64_t x_row_stride, const float* qscale, int64_t rows, const float* y,
                            int64_t y_row_stride, Key kp, int64_t m, int32_t k, int32_t t, int64_t* index, float* key, void* workspace,
                            hipStream_t st) {
  const int n_spans = nn_spans(m);
  const int64_t n_blocks = (rows + kNnRows - 1) / kNnRows;
  const int64_t groups = (n_blocks + kNnGroup - 1) / kNnGroup;
  const int64_t grid = groups * kNnGroup * n_spans;
  if (grid > 0x7fffffffLL)
    return fail(MMK_ERR_UNSUPPORTED, "%s: %lld rows against %lld frames are more than one launch takes", who, (long long)rows, (long long)m);
  float* ws_key = static_cast<float*>(workspace);
  int32_t* ws_idx = reinterpret_cast<int32_t*>(ws_key + rows * n_spans * t);
  MMK_TRY(launch(nn_search_kernel<TC, kSelf, Key>, dim3((unsigned)grid), dim3(kNnThreads), 0, st, x, x_row_stride, qscale, rows, y, y_row_stride, kp, m, k, t,
                 (int32_t)n_blocks, n_spans, ws_key, ws_idx));
  return launch(nn_merge_kernel<TC>, dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, st, ws_key, ws_idx, rows, t, n_spans, index, key);
}

}  // namespace mmk
