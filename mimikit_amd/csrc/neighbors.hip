// Scoring generated clips against the training corpus (mimikit/extract/from_neighbors.py:13-19, :44-55 and demos/checkpoint_k_bests.py:36-46):
// every generated frame's nearest corpus frame by angular distance, and the cumulative entropy of the series of those neighbours.
//
//   mmk_nn_cosine_f32     nn_cosine_kernel, the tiles of nn_search.h with a list of one and the cosine key, kept as its own kernel (see
//                         there): the row arg-max of c[r, j] = clamp(<x_r, y_j> rx[r] ry[j], -1, 1), greater value, then lower index;
//                         nn_merge_kernel<1> of nn_search.h joins the spans and writes index (int64) and cos_best.
//   mmk_nn_cosine_self_f32   nn_search_kernel<1, true, NnCosineKey> of nn_search.h, the corpus = the queries and frame r left out of row r:
//                         the nearest OTHER frame, every level of HCluster (hcluster.hip holds the rest of a level).
//   cum_entropy_kernel    one workgroup per row of t items.  e[s] = log(s + 1) - S(s) / (s + 1) with S(s) = sum_{u <= s} (f(r_u + 1) - f(r_u)),
//                         f(c) = c log c, r_u = the number of earlier occurrences of item u in the row: the entropy of the running histogram
//                         without an items x t table.  The row is walked in chunks of 256 positions: a thread counts its item's earlier
//                         occurrences (the row is read through the scalar / L1 path: every lane asks for the same address), a Hillis-Steele
//                         scan in LDS adds the chunk in one fixed order on top of the carry, all in fp64; e is clamped at 0 (and IS 0 while the row has shown
//                         one item only: the telescoped sum leaves a rounding residue there) and rounded to
//                         fp32 once, the total is a fixed-order fp64 sum of the clamped values rounded once.
// No atomics, no workgroup waits for another; every sum has one order, so results are the same from run to run.
// NaN in the inputs is not handled (> drops it silently).
#include "nn_search.h"

namespace mmk {

// The plain arg-max keeps the kernel it had before nn_search.h.  It walks the tiles of nn_search_kernel<1, false, NnCosineKey> with the
// same pieces of frame_walk.h and gives its bits (scripts/walk_parity.py); but as that instance it measured 0.2 % slower on
// scripts/neighbors_bench.py than this kernel, outside the range of three runs, with the same instructions in the loop over the bins and in
// the tile's epilogue (DESIGN.md section 5.6.3 has the figures).  Until the cause is known this entry point does not move.  Its own: the
// arg-max in two registers per row and the join arrays.
__global__ __launch_bounds__(kNnThreads, 2) void nn_cosine_kernel(const float* __restrict__ x, int64_t x_row_stride, const float* __restrict__ rx,
                                                               int64_t rows, const float* __restrict__ y, int64_t y_row_stride,
                                                               const float* __restrict__ ry, int64_t M, int32_t K, int32_t n_blocks,
                                                               int32_t n_spans, float* __restrict__ ws_val, int32_t* __restrict__ ws_idx) {
  __shared__ __attribute__((aligned(16))) float ys[kNnCols * kFwPitch];
  __shared__ __attribute__((aligned(16))) float xs[kNnRows * kFwPitch];
  __shared__ float rys[2][kNnCols];
  __shared__ float red_val[2][kNnRows];
  __shared__ int red_idx[2][kNnRows];
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

  float rxq[2];
#pragma unroll
  for (int tn = 0; tn < 2; ++tn) {
    const int64_t r = rbase + wn * 64 + tn * 32 + fr;
    rxq[tn] = r < rows ? rx[r] : 0.f;
  }
  const float ninf = __int_as_float(0xff800000);
  float best[2] = {ninf, ninf};
  int bidx[2] = {kNnEmpty, kNnEmpty};

  int parity = 0;
  for (int64_t jt = jbeg; jt < jend; jt += kNnCols, parity ^= 1) {
    if (tid < kNnCols) {
      const int64_t j = jt + tid;
      rys[parity][tid] = j < jend ? ry[j] : 0.f;
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

    // the tile's arg-max, inside the lane and in rising frame order: strictly greater wins, so the lowest index stays
#pragma unroll
    for (int tm = 0; tm < 2; ++tm)
#pragma unroll
      for (int q = 0; q < 16; ++q) {
        const int jl = fw_acc_row(wm * 64 + tm * 32, q, fh);
        const int64_t j = jt + jl;
        const float ryj = rys[parity][jl];
#pragma unroll
        for (int tn = 0; tn < 2; ++tn) {
          const float c = fminf(fmaxf(acc[tm][tn][q] * rxq[tn] * ryj, -1.f), 1.f);
          if (j < jend && c > best[tn]) {
            best[tn] = c;
            bidx[tn] = (int)j;
          }
        }
      }
  }

  // join the two halves of the wave, then the two waves that share these query rows
#pragma unroll
  for (int tn = 0; tn < 2; ++tn) {
    const float ov = __shfl_xor(best[tn], 32);
    const int oj = __shfl_xor(bidx[tn], 32);
    if (nn_better(ov, oj, best[tn], bidx[tn])) {
      best[tn] = ov;
      bidx[tn] = oj;
    }
    if (fh == 0) {
      red_val[wm][wn * 64 + tn * 32 + fr] = best[tn];
      red_idx[wm][wn * 64 + tn * 32 + fr] = bidx[tn];
    }
  }
  __syncthreads();
  if (tid < kNnRows && rbase + tid < rows) {
    float v = red_val[0][tid];
    int j = red_idx[0][tid];
    if (nn_better(red_val[1][tid], red_idx[1][tid], v, j)) {
      v = red_val[1][tid];
      j = red_idx[1][tid];
    }
    ws_val[(int64_t)span * rows + rbase + tid] = v;
    ws_idx[(int64_t)span * rows + rbase + tid] = j;
  }
}

constexpr int kCeThreads = 256;

__device__ __forceinline__ double ce_f(double c) { return c > 0.0 ? c * log(c) : 0.0; }

__global__ __launch_bounds__(kCeThreads) void cum_entropy_kernel(const int64_t* __restrict__ items, int64_t row_stride, int32_t T,
                                                                 float* __restrict__ total, float* __restrict__ e, int64_t e_row_stride) {
  __shared__ double scan[2][kCeThreads];
  const int tid = threadIdx.x;
  const int64_t* row = items + (int64_t)blockIdx.x * row_stride;
  float* er = e ? e + (int64_t)blockIdx.x * e_row_stride : nullptr;
  double carry = 0.0;       // S at the end of the chunk before this one
  double mine = 0.0;        // this thread's e values, added in chunk order
  for (int s0 = 0; s0 < T; s0 += kCeThreads) {
    const int s = s0 + tid;
    const bool in = s < T;
    const int64_t it = row[in ? s : T - 1];
    // earlier occurrences: u runs over the same positions for every lane (a uniform address), each lane keeps those before its own
    const int last = min(s0 + kCeThreads, T);
    int r = 0;
    for (int u = 0; u < last; ++u) r += (row[u] == it && u < s) ? 1 : 0;
    double d = in ? ce_f((double)(r + 1)) - ce_f((double)r) : 0.0;
    // inclusive scan of the chunk, Hillis-Steele: position p adds position p - 2^i at step i - one order for every chunk
    int cur = 0;
    scan[0][tid] = d;
    __syncthreads();
#pragma unroll
    for (int off = 1; off < kCeThreads; off <<= 1) {
      const double v = scan[cur][tid] + (tid >= off ? scan[cur][tid - off] : 0.0);
      scan[cur ^ 1][tid] = v;
      cur ^= 1;
      __syncthreads();
    }
    const double S = carry + scan[cur][tid];
    const double next = carry + scan[cur][kCeThreads - 1];
    __syncthreads();        // (the next chunk writes scan[0] again)
    carry = next;
    if (in) {
      const double n1 = (double)(s + 1);
      double h = log(n1) - S / n1;
      h = (h > 0.0 && r != s) ? h : 0.0;      // r == s: every item so far is this one - a histogram of one bin, exactly 0
      mine += h;
      if (er) er[s] = (float)h;
    }
  }
  // the threads' sums, a binary tree in LDS: one fixed order
  scan[0][tid] = mine;
  __syncthreads();
#pragma unroll
  for (int off = kCeThreads / 2; off >= 1; off >>= 1) {
    if (tid < off) scan[0][tid] += scan[0][tid + off];
    __syncthreads();
  }
  if (tid == 0) total[blockIdx.x] = (float)scan[0][0];
}

}  // namespace mmk

extern "C" size_t mmk_nn_cosine_workspace_bytes(int64_t rows, int64_t m) {
  using namespace mmk;
  if (rows < 1 || m < 1) return 0;
  return (size_t)rows * (size_t)nn_spans(m) * (sizeof(float) + sizeof(int32_t));
}

extern "C" int mmk_nn_cosine_f32(const float* x, int64_t x_row_stride, const float* rx, int64_t rows, const float* y, int64_t y_row_stride,
                                 const float* ry, int64_t m, int32_t k, int64_t* index, float* cos_best, void* workspace,
                                 size_t workspace_bytes, mmk_stream_t stream) {
  using namespace mmk;
  if (rows < 1) return fail(MMK_ERR_INVALID, "nn_cosine: rows = %lld < 1 (query frames)", (long long)rows);
  if (m < 1) return fail(MMK_ERR_INVALID, "nn_cosine: m = %lld < 1 (corpus frames)", (long long)m);
  if (k < 1) return fail(MMK_ERR_INVALID, "nn_cosine: k = %d < 1 (bins)", k);
  if (m > 0x7fffffffLL - kNnSpan)
    return fail(MMK_ERR_UNSUPPORTED, "nn_cosine: m = %lld corpus frames: indices are kept in 32 bits across the spans", (long long)m);
  if (!x || !y || !rx || !ry || !index || !cos_best || !workspace || x_row_stride < 0 || y_row_stride < 0)
    return fail(MMK_ERR_INVALID, "nn_cosine: bad arguments (null pointer or negative stride %lld / %lld)", (long long)x_row_stride,
                (long long)y_row_stride);
  if (misaligned(x, 4) || misaligned(y, 4) || misaligned(rx, 4) || misaligned(ry, 4) || misaligned(cos_best, 4) || misaligned(workspace, 4))
    return fail(MMK_ERR_INVALID, "nn_cosine: x, y, rx, ry, cos_best and the workspace must be 4-byte aligned");
  if (misaligned(index, 8)) return fail(MMK_ERR_INVALID, "nn_cosine: index must be 8-byte aligned");
  MMK_TRY(workspace_check("nn_cosine", workspace, 4, workspace_bytes, mmk_nn_cosine_workspace_bytes(rows, m)));
  // nn_search_launch's grid and workspace (T = 1) around the kernel above: a second copy of that arithmetic, as the kernel is of the walk -
  // a change to the kNnGroup numbering or to the workspace layout is made there, in nn_search_kernel and here
  const int n_spans = nn_spans(m);
  const int64_t n_blocks = (rows + kNnRows - 1) / kNnRows;
  const int64_t grid = (n_blocks + kNnGroup - 1) / kNnGroup * kNnGroup * n_spans;
  if (grid > 0x7fffffffLL)
    return fail(MMK_ERR_UNSUPPORTED, "nn_cosine: %lld rows against %lld frames are more than one launch takes", (long long)rows, (long long)m);
  float* ws_val = static_cast<float*>(workspace);
  int32_t* ws_idx = reinterpret_cast<int32_t*>(ws_val + rows * n_spans);
  MMK_TRY(launch(nn_cosine_kernel, dim3((unsigned)grid), dim3(kNnThreads), 0, (hipStream_t)stream, x, x_row_stride, rx, rows, y, y_row_stride,
                 ry, m, k, (int32_t)n_blocks, n_spans, ws_val, ws_idx));
  return launch(nn_merge_kernel<1>, dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, (hipStream_t)stream, ws_val, ws_idx, rows, 1, n_spans,
                index, cos_best);
}

extern "C" int mmk_nn_cosine_self_f32(const float* x, int64_t x_row_stride, const float* rx, int64_t rows, int32_t k, int64_t* index,
                                      float* cos_best, void* workspace, size_t workspace_bytes, mmk_stream_t stream) {
  using namespace mmk;
  if (rows < 2) return fail(MMK_ERR_INVALID, "nn_cosine_self: rows = %lld < 2 (a frame needs another one)", (long long)rows);
  if (k < 1) return fail(MMK_ERR_INVALID, "nn_cosine_self: k = %d < 1 (bins)", k);
  if (rows > 0x7fffffffLL - kNnSpan)
    return fail(MMK_ERR_UNSUPPORTED, "nn_cosine_self: %lld frames: indices are kept in 32 bits across the spans", (long long)rows);
  if (!x || !rx || !index || !cos_best || !workspace || x_row_stride < 0)
    return fail(MMK_ERR_INVALID, "nn_cosine_self: bad arguments (null pointer or negative stride %lld)", (long long)x_row_stride);
  if (misaligned(x, 4) || misaligned(rx, 4) || misaligned(cos_best, 4) || misaligned(workspace, 4))
    return fail(MMK_ERR_INVALID, "nn_cosine_self: x, rx, cos_best and the workspace must be 4-byte aligned");
  if (misaligned(index, 8)) return fail(MMK_ERR_INVALID, "nn_cosine_self: index must be 8-byte aligned");
  MMK_TRY(workspace_check("nn_cosine_self", workspace, 4, workspace_bytes, mmk_nn_cosine_workspace_bytes(rows, rows)));
  return nn_search_launch<1, true>("nn_cosine_self", x, x_row_stride, rx, rows, x, x_row_stride, NnCosineKey{rx}, rows, k, 1, index, cos_best,
                             workspace, (hipStream_t)stream);
}

extern "C" int mmk_cum_entropy_i64(const int64_t* items, int64_t row_stride, int32_t batch, int64_t t, float* total, float* e,
                                   int64_t e_row_stride, mmk_stream_t stream) {
  using namespace mmk;
  if (batch < 1) return fail(MMK_ERR_INVALID, "cum_entropy: batch = %d < 1", batch);
  if (t < 1) return fail(MMK_ERR_INVALID, "cum_entropy: t = %lld < 1 (items per row)", (long long)t);
  if (t > MMK_CUM_ENTROPY_MAX_T)
    return fail(MMK_ERR_UNSUPPORTED, "cum_entropy: t = %lld items per row, more than the %d (MMK_CUM_ENTROPY_MAX_T) one workgroup ranks",
                (long long)t, MMK_CUM_ENTROPY_MAX_T);
  if (!items || !total || row_stride < 0 || e_row_stride < 0 || misaligned(items, 8) || misaligned(total, 4) || misaligned(e, 4))
    return fail(MMK_ERR_INVALID, "cum_entropy: bad arguments (null or misaligned pointer, negative stride %lld / %lld)", (long long)row_stride,
                (long long)e_row_stride);
  return launch(cum_entropy_kernel, dim3((unsigned)batch), dim3(kCeThreads), 0, (hipStream_t)stream, items, row_stride, (int32_t)t, total, e,
                e_row_stride);
}
