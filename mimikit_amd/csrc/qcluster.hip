// The k nearest frames of every frame (mimikit/extract/clusters.py:27-98 QCluster; any k-nearest-neighbour graph).
//
//   mmk_nn_topk_f32       nn_search_kernel<TC, kSelf, NnAffineKey> of nn_search.h, the tile walk with lists of TC, the smallest of 1, 4, 8, 16
//                         that holds T: key[r, j] = clamp((<x_r, y_j> * qscale[r]) * cscale[j] + cshift[j], key_min, key_max).  The limits are
//                         the caller's, -inf and +inf for none: the euclidean key has no range, a cosine is clamped to [-1, 1] as
//                         NnCosineKey clamps it - where k = 1 every cosine is +-1 give or take an ulp, and only the clamp makes those a tie
//                         that the lower index wins.  nn_merge_kernel<TC> joins the spans and writes index (rows, T) int64 and key (rows, T).
//   half_neg_sqnorm_kernel      cshift of the euclidean metric: -|y_j|^2 / 2, a wave per row, the squares added in fp64 in one fixed order
//                         and rounded to fp32 once.  With scales 1 the largest key <x, y> - |y|^2 / 2 is the smallest |x - y|^2.
// No atomics, no workgroup waits for another; two calls give the same bits.  NaN and inf in the inputs are not handled (a key of -inf never
// enters a list).
#include "nn_search.h"

namespace mmk {

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

template <int TC>
static auto topk_launch(bool self) { return self ? nn_search_launch<TC, true, NnAffineKey> : nn_search_launch<TC, false, NnAffineKey>; }

}  // namespace mmk

extern "C" size_t mmk_nn_topk_workspace_bytes(int64_t rows, int64_t m, int32_t t) {
  using namespace mmk;
  if (rows < 1 || m < 1 || t < 1 || t > MMK_NN_TOPK_MAX) return 0;
  return (size_t)rows * (size_t)nn_spans(m) * (size_t)t * (sizeof(float) + sizeof(int32_t));
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
  if (m > 0x7fffffffLL - kNnSpan)
    return fail(MMK_ERR_UNSUPPORTED, "nn_topk: m = %lld corpus frames: indices are kept in 32 bits across the spans", (long long)m);
  if (self_exclude && (m != rows || y != x || y_row_stride != x_row_stride))
    return fail(MMK_ERR_INVALID, "nn_topk: self_exclude takes the corpus = the queries (y == x, the same stride, m == rows = %lld, got m = %lld)",
                (long long)rows, (long long)m);
  if (!x || !y || !qscale || !cscale || !cshift || !index || !key || !workspace || x_row_stride < 0 || y_row_stride < 0)
    return fail(MMK_ERR_INVALID, "nn_topk: bad arguments (null pointer or negative stride %lld / %lld)", (long long)x_row_stride,
                (long long)y_row_stride);
  if (misaligned(x, 4) || misaligned(y, 4) || misaligned(qscale, 4) || misaligned(cscale, 4) || misaligned(cshift, 4) || misaligned(key, 4) ||
      misaligned(workspace, 4))
    return fail(MMK_ERR_INVALID, "nn_topk: x, y, qscale, cscale, cshift, key and the workspace must be 4-byte aligned");
  if (misaligned(index, 8)) return fail(MMK_ERR_INVALID, "nn_topk: index must be 8-byte aligned");
  MMK_TRY(workspace_check("nn_topk", workspace, 4, workspace_bytes, mmk_nn_topk_workspace_bytes(rows, m, t)));
  const bool self = self_exclude != 0;
  const auto search = t == 1 ? topk_launch<1>(self) : t <= 4 ? topk_launch<4>(self) : t <= 8 ? topk_launch<8>(self) : topk_launch<16>(self);
  return search("nn_topk", x, x_row_stride, qscale, rows, y, y_row_stride, NnAffineKey{cscale, cshift, key_min, key_max}, m, k, t,
                index, key, workspace, (hipStream_t)stream);
}

extern "C" int mmk_half_neg_sqnorm_f32(const float* y, int64_t y_row_stride, int64_t rows, int32_t k, float* out, mmk_stream_t stream) {
  using namespace mmk;
  if (rows < 1 || k < 1) return fail(MMK_ERR_INVALID, "half_neg_sqnorm: rows = %lld, k = %d (both at least 1)", (long long)rows, k);
  if ((rows + 3) / 4 > 0x7fffffffLL) return fail(MMK_ERR_UNSUPPORTED, "half_neg_sqnorm: %lld rows are more than one launch takes", (long long)rows);
  if (!y || !out || y_row_stride < 0 || misaligned(y, 4) || misaligned(out, 4))
    return fail(MMK_ERR_INVALID, "half_neg_sqnorm: bad arguments (null or misaligned pointer, negative stride %lld)", (long long)y_row_stride);
  return launch(half_neg_sqnorm_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, (hipStream_t)stream, y, y_row_stride, rows, k, out);
}
