// NearestNextNeighbor's alignment (mimikit/models/nnn.py:14-49): the cosine distances of B prompts of N <= 64 frames against a corpus of M
// frames over K bins, and the subsequence DTW over them of which only the last row's first minimum is wanted.
//
//   inv_row_norm_kernel   rx / ry: 1 / |row|, 0 for a row of norm 0.  One wave per row: lane l adds the squares of bins l, l + 64, ... in
//                         turn, a butterfly joins the lanes - one fixed order.
//   cosine_cost_kernel    cost[b][j][i] = clamp(1 - <|x_b,i|, |y_j|> rx[b,i] ry[j], 0, 2), corpus-frame-major: the costs of corpus frame j
//                         against the N rows of clip b are contiguous, padded to n_pad = N rounded up to MMK_NNN_ROW_PAD (padding = 1).
//                         A workgroup of four waves owns kCcJT = 64 corpus frames, 16 per wave.  The prompt rows of all clips are cut into
//                         tiles of 16 (a tile never spans two clips) and taken RT tiles at a time; with RT = 16 the 256 rows of a pass stay
//                         in accumulators, so the workgroup's corpus frames come from memory ONCE for up to 256 prompt rows and once per
//                         256 rows beyond that (the repeats find them in the L2: 64 frames are 262 KB at K = 1025).  Both operands go
//                         through LDS in chunks of kCcKC = 32 bins: rows are loaded dword by dword with consecutive lanes on consecutive
//                         bins (coalesced whatever the row stride and the base alignment), |.| applied, rows and bins beyond the ends
//                         stored as zeros - nothing is padded by the caller.  v_mfma_f32_16x16x4_f32, A = prompt rows, B = corpus frames:
//                         lane (r = l & 15, g = l >> 4) reads bins 16 h + 4 g .. + 3 of its row as one 16-byte LDS read and feeds MFMA e
//                         with bin 16 h + 4 g + e - the same permutation of the bins on both operands, so a fixed order of the sum.  The
//                         row pitch of 36 floats keeps those reads apart in the banks.  D (column l & 15 = corpus frame, rows 4 g + e =
//                         prompt rows) is four consecutive costs of one corpus frame: one 16-byte store per lane and tile.
//   dtw_subseq_kernel     one wave per clip, lane i owns prompt row i, anti-diagonal s puts lane i on column j = s - i:
//                             D[0, j] = C[0, j],   D[i, j] = C[i, j] + min(D[i-1, j-1], D[i, j-1], D[i-1, j])   (+inf outside the matrix)
//                         D[i, j-1] is the lane's own last value, D[i-1, j] the last value of the lane below (a DPP wave shift, +inf into
//                         lane 0), D[i-1, j-1] what that shift brought one step earlier.  Every D is one rounded add of an exact minimum:
//                         the result is that of the sequential fp32 loop, bit for bit.  Costs do not depend on the chain and are loaded
//                         MMK_NNN_LOOKAHEAD steps ahead; blocks of that many steps in which every row is inside the matrix run without
//                         masks.  Lane N - 1 keeps its row's minimum and the first column that attains it (updates on < only).
// No atomics, no workgroup waits for another, no scratch; every sum has one order, so results are the same from run to run.
// NaN in the inputs is not handled (min and < drop it silently).
#include "entry_util.h"
#include "wave_ops.h"

namespace mmk {

typedef float nnn_f32x4 __attribute__((ext_vector_type(4)));

constexpr int kNnnMaxRows = MMK_NNN_MAX_ROWS;
constexpr int kNnnRowPad = MMK_NNN_ROW_PAD;
constexpr int kNnnLook = MMK_NNN_LOOKAHEAD;
static_assert(kNnnMaxRows == 64 && kNnnRowPad == 16, "one wave per clip, MFMA tiles of 16 rows");
static_assert((kNnnLook - 1) * kNnnMaxRows * 4 < 4096, "the look-ahead loads address their column by an immediate offset");

// ---- inverse row norms -------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void inv_row_norm_kernel(const float* __restrict__ x, int64_t batch_stride, int64_t row_stride, int64_t rows,
                                                           int64_t total, int32_t K, float* __restrict__ out) {
  const int lane = threadIdx.x & 63;
  const int64_t g = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (g >= total) return;
  const float* p = x + (g / rows) * batch_stride + (g % rows) * row_stride;
  const float r = wave_inv_row_norm(p, K, lane);
  if (lane == 0) out[g] = r;
}

// ---- cosine cost -------------------------------------------------------------------------------------------------------------------
constexpr int kCcThreads = 256;
constexpr int kCcJT = 64;       // corpus frames of a workgroup, 16 per wave
constexpr int kCcKC = 32;       // bins per LDS chunk
constexpr int kCcPitch = 36;    // floats between LDS rows: 16-byte aligned, and lanes (r, g) of one read fall into 64 different banks

template <int RT>
__global__ __launch_bounds__(kCcThreads) void cosine_cost_kernel(const float* __restrict__ x, int64_t x_batch_stride, int64_t x_row_stride,
                                                                 const float* __restrict__ rx, int32_t batch, int32_t N, int32_t nt,
                                                                 const float* __restrict__ y, int64_t y_row_stride,
                                                                 const float* __restrict__ ry, int64_t M, int32_t K, float* __restrict__ cost) {
  __shared__ __attribute__((aligned(16))) float xs[RT * 16 * kCcPitch];
  __shared__ __attribute__((aligned(16))) float ys[kCcJT * kCcPitch];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int col = tid & 31, row0 = tid >> 5;      // loads: bin `col` of rows row0, row0 + 8, ...
  const int fr = lane & 15, fg = lane >> 4;       // MFMA fragments: row / column fr, bin group fg
  const int64_t jbase = (int64_t)blockIdx.x * kCcJT;
  const int T = batch * nt;                       // prompt row tiles: tile t = row tile t % nt of clip t / nt
  const int n_pad = nt * 16;

  for (int t0 = 0; t0 < T; t0 += RT) {
    const int b0 = t0 / nt, it0 = t0 % nt;
    nnn_f32x4 acc[RT];
#pragma unroll
    for (int q = 0; q < RT; ++q) acc[q] = nnn_f32x4{0.f, 0.f, 0.f, 0.f};

    for (int k0 = 0; k0 < K; k0 += kCcKC) {
      const int k = k0 + col;
      const bool kin = k < K;
      const int kc = kin ? k : K - 1;             // every load is unconditional at a clamped, valid address; the mask picks zero afterwards
#pragma unroll
      for (int r = 0; r < kCcJT; r += 8) {
        const int64_t j = jbase + r + row0;
        const float v = y[(j < M ? j : M - 1) * y_row_stride + kc];
        ys[(r + row0) * kCcPitch + col] = (kin && j < M) ? fabsf(v) : 0.f;
      }
      {
        int b = b0, it = it0;
#pragma unroll
        for (int q = 0; q < RT; ++q) {
#pragma unroll
          for (int h = 0; h < 16; h += 8) {
            const int i = it * 16 + h + row0;
            const float v = x[(int64_t)(b < batch ? b : batch - 1) * x_batch_stride + (int64_t)(i < N ? i : N - 1) * x_row_stride + kc];
            xs[(q * 16 + h + row0) * kCcPitch + col] = (kin && b < batch && i < N) ? fabsf(v) : 0.f;
          }
          if (++it == nt) { it = 0; ++b; }
        }
      }
      __syncthreads();
#pragma unroll
      for (int h = 0; h < kCcKC; h += 16) {
        const nnn_f32x4 bv = *reinterpret_cast<const nnn_f32x4*>(&ys[(wave * 16 + fr) * kCcPitch + h + 4 * fg]);
#pragma unroll
        for (int q = 0; q < RT; ++q) {
          const nnn_f32x4 av = *reinterpret_cast<const nnn_f32x4*>(&xs[(q * 16 + fr) * kCcPitch + h + 4 * fg]);
#pragma unroll
          for (int e = 0; e < 4; ++e) acc[q] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[e], bv[e], acc[q], 0, 0, 0);
        }
      }
      __syncthreads();
    }

    const int64_t j = jbase + wave * 16 + fr;
    if (j < M) {
      const float ryj = ry[j];
      int b = b0, it = it0;
#pragma unroll
      for (int q = 0; q < RT; ++q) {
        if (b < batch) {
          const int i0 = it * 16 + 4 * fg;
          nnn_f32x4 o;
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const float rxi = (i0 + e < N) ? rx[(int64_t)b * N + i0 + e] : 0.f;
            o[e] = fminf(fmaxf(1.0f - acc[q][e] * rxi * ryj, 0.f), 2.f);
          }
          *reinterpret_cast<nnn_f32x4*>(cost + ((int64_t)b * M + j) * n_pad + i0) = o;
        }
        if (++it == nt) { it = 0; ++b; }
      }
    }
  }
}

// ---- subsequence DTW ---------------------------------------------------------------------------------------------------------------
// lane l receives lane l - 1's v, lane 0 +inf (DPP wave_shr:1; a lane without a source keeps `old`)
__device__ __forceinline__ float nnn_from_lane_below(float v) {
  return dpp_move<kDppWaveShr1>(v, INFINITY);
}

template <int NPAD, bool kRow>
__global__ __launch_bounds__(64) void dtw_subseq_kernel(const float* __restrict__ cost, int32_t N, int32_t M, int64_t* __restrict__ end_col,
                                                        float* __restrict__ end_val, float* __restrict__ last_row) {
  const int lane = threadIdx.x;
  const int i = lane < N ? lane : N - 1;          // lanes beyond the prompt shadow row N - 1: their loads stay in bounds, nobody reads them
  const bool first = lane == 0, last = lane == N - 1;
  const float* c = cost + (int64_t)blockIdx.x * M * NPAD + i;      // C[i, j] = c[j NPAD]
  float* lr = kRow ? last_row + (int64_t)blockIdx.x * M : nullptr;
  const float inf = __int_as_float(0x7f800000);
  float cur = inf, diag = inf, best = inf;        // D[i, j-1], D[i-1, j-1]; the row's minimum so far
  int best_j = 0;
  const int S = M + N - 1;                         // anti-diagonals (M + N < 2^31)

  float cb[kNnnLook];
#pragma unroll
  for (int u = 0; u < kNnnLook; ++u) {
    const int j = u - i;
    cb[u] = c[(int64_t)(j < 0 ? 0 : j < M ? j : M - 1) * NPAD];      // (outside the matrix: any valid address, the step masks the result)
  }
  for (int s0 = 0; s0 < S; s0 += kNnnLook) {
    const int j0 = s0 - i;                        // this lane's column at the block's first step
    // a block whose steps find every row inside the matrix: s0 >= N - 1 and s0 + kNnnLook - 1 <= M - 1
    const bool whole = s0 >= N - 1 && s0 + kNnnLook <= M;
    const bool whole_next = s0 + kNnnLook >= N - 1 && s0 + 2 * kNnnLook <= M;
    float cn[kNnnLook];
    if (whole_next) {
      const float* p = c + (int64_t)(j0 + kNnnLook) * NPAD;
#pragma unroll
      for (int u = 0; u < kNnnLook; ++u) cn[u] = p[u * NPAD];
    } else {
#pragma unroll
      for (int u = 0; u < kNnnLook; ++u) {
        const int j = j0 + kNnnLook + u;
        cn[u] = c[(int64_t)(j < 0 ? 0 : j < M ? j : M - 1) * NPAD];
      }
    }
    if (whole) {
#pragma unroll
      for (int u = 0; u < kNnnLook; ++u) {
        const float up = nnn_from_lane_below(cur);
        const float m = fminf(fminf(up, diag), cur);
        cur = cb[u] + (first ? 0.f : m);
        diag = up;
        const bool lower = cur < best;
        best = lower ? cur : best;
        best_j = lower ? j0 + u : best_j;
        if (kRow && last) lr[j0 + u] = cur;
      }
    } else {
#pragma unroll
      for (int u = 0; u < kNnnLook; ++u) {
        const int j = j0 + u;
        const float up = nnn_from_lane_below(cur);
        const float m = fminf(fminf(up, diag), cur);
        const float d = cb[u] + (first ? 0.f : m);
        diag = up;
        if (j >= 0 && j < M) {
          cur = d;
          if (d < best) { best = d; best_j = j; }
          if (kRow && last) lr[j] = d;
        }
      }
    }
#pragma unroll
    for (int u = 0; u < kNnnLook; ++u) cb[u] = cn[u];
  }
  if (last) {
    end_col[blockIdx.x] = best_j;
    end_val[blockIdx.x] = best;
  }
}

static int nnn_sizes_check(const char* what, int32_t batch, int32_t n, int64_t m, int32_t k) {
  if (batch < 1) return fail(MMK_ERR_INVALID, "%s: batch = %d < 1", what, batch);
  if (batch > (1 << 24)) return fail(MMK_ERR_UNSUPPORTED, "%s: batch = %d clips are more than one launch takes", what, batch);
  if (n < 1) return fail(MMK_ERR_INVALID, "%s: n = %d < 1 (prompt frames)", what, n);
  if (n > kNnnMaxRows)
    return fail(MMK_ERR_UNSUPPORTED, "%s: n = %d prompt frames, more than the %d (MMK_NNN_MAX_ROWS) one wave aligns", what, n, kNnnMaxRows);
  if (m < 1) return fail(MMK_ERR_INVALID, "%s: m = %lld < 1 (corpus frames)", what, (long long)m);
  if (m > 0x7fffffffLL - 2 * kNnnMaxRows)
    return fail(MMK_ERR_UNSUPPORTED, "%s: m = %lld corpus frames: columns are counted in 32 bits", what, (long long)m);
  if (k < 1) return fail(MMK_ERR_INVALID, "%s: k = %d < 1 (bins)", what, k);
  return MMK_OK;
}

}  // namespace mmk

extern "C" int mmk_inv_row_norm_f32(const float* x, int64_t x_batch_stride, int64_t x_row_stride, int32_t batch, int64_t rows, int32_t k,
                                    float* inv_norm, mmk_stream_t stream) {
  using namespace mmk;
  if (batch < 1) return fail(MMK_ERR_INVALID, "inv_row_norm: batch = %d < 1", batch);
  if (rows < 1) return fail(MMK_ERR_INVALID, "inv_row_norm: rows = %lld < 1", (long long)rows);
  if (k < 1) return fail(MMK_ERR_INVALID, "inv_row_norm: k = %d < 1 (bins)", k);
  if (!x || !inv_norm || x_batch_stride < 0 || x_row_stride < 0 || misaligned(x, 4) || misaligned(inv_norm, 4))
    return fail(MMK_ERR_INVALID, "inv_row_norm: bad arguments (null or misaligned pointer, negative stride %lld / %lld)",
                (long long)x_batch_stride, (long long)x_row_stride);
  const int64_t total = (int64_t)batch * rows;
  if ((total + 3) / 4 > 0x7fffffffLL) return fail(MMK_ERR_UNSUPPORTED, "inv_row_norm: %lld rows are more than one launch takes", (long long)total);
  return launch(inv_row_norm_kernel, dim3((unsigned)((total + 3) / 4)), dim3(256), 0, (hipStream_t)stream, x, x_batch_stride, x_row_stride, rows,
                total, k, inv_norm);
}

extern "C" int mmk_cosine_cost_f32(const float* x, int64_t x_batch_stride, int64_t x_row_stride, const float* rx, int32_t batch, int32_t n,
                                   const float* y, int64_t y_row_stride, const float* ry, int64_t m, int32_t k, float* cost,
                                   mmk_stream_t stream) {
  using namespace mmk;
  MMK_TRY(nnn_sizes_check("cosine_cost", batch, n, m, k));
  if (!x || !y || !rx || !ry || !cost || x_row_stride < 0 || y_row_stride < 0 || x_batch_stride < 0)
    return fail(MMK_ERR_INVALID, "cosine_cost: bad arguments (null pointer or negative stride %lld / %lld / %lld)", (long long)x_batch_stride,
                (long long)x_row_stride, (long long)y_row_stride);
  if (misaligned(x, 4) || misaligned(y, 4) || misaligned(rx, 4) || misaligned(ry, 4))
    return fail(MMK_ERR_INVALID, "cosine_cost: x, y, rx and ry must be 4-byte aligned");
  if (misaligned(cost, 16)) return fail(MMK_ERR_INVALID, "cosine_cost: cost must be 16-byte aligned");
  const int nt = (n + kNnnRowPad - 1) / kNnnRowPad;
  const int T = batch * nt;
  const dim3 grid((unsigned)((m + kCcJT - 1) / kCcJT)), wg(kCcThreads);
  hipStream_t st = (hipStream_t)stream;
#define MMK_CC_LAUNCH(RT) \
  launch(cosine_cost_kernel<RT>, grid, wg, 0, st, x, x_batch_stride, x_row_stride, rx, batch, n, nt, y, y_row_stride, ry, m, k, cost)
  if (T <= 1) return MMK_CC_LAUNCH(1);
  if (T <= 4) return MMK_CC_LAUNCH(4);
  return MMK_CC_LAUNCH(16);
#undef MMK_CC_LAUNCH
}

extern "C" int mmk_dtw_subseq_f32(const float* cost, int32_t batch, int32_t n, int64_t m, int64_t* end_col, float* end_val, float* last_row,
                                  mmk_stream_t stream) {
  using namespace mmk;
  MMK_TRY(nnn_sizes_check("dtw_subseq", batch, n, m, 1));
  if (!cost || !end_col || !end_val) return fail(MMK_ERR_INVALID, "dtw_subseq: cost, end_col and end_val must not be null");
  if (misaligned(cost, 4) || misaligned(end_val, 4) || misaligned(last_row, 4))
    return fail(MMK_ERR_INVALID, "dtw_subseq: cost, end_val and last_row must be 4-byte aligned");
  if (misaligned(end_col, 8)) return fail(MMK_ERR_INVALID, "dtw_subseq: end_col must be 8-byte aligned");
  const int nt = (n + kNnnRowPad - 1) / kNnnRowPad;
  const dim3 grid((unsigned)batch), wg(64);
  hipStream_t st = (hipStream_t)stream;
#define MMK_DTW_LAUNCH(NPAD)                                                                                           \
  last_row ? launch(dtw_subseq_kernel<NPAD, true>, grid, wg, 0, st, cost, n, (int32_t)m, end_col, end_val, last_row) \
           : launch(dtw_subseq_kernel<NPAD, false>, grid, wg, 0, st, cost, n, (int32_t)m, end_col, end_val, last_row)
  switch (nt) {
    case 1: return MMK_DTW_LAUNCH(16);
    case 2: return MMK_DTW_LAUNCH(32);
    case 3: return MMK_DTW_LAUNCH(48);
    default: return MMK_DTW_LAUNCH(64);
  }
#undef MMK_DTW_LAUNCH
}
