// The host half that the feature and corpus entry points share (features, filters, envelope, nnn, neighbors, hcluster, qcluster, kmeans,
// nn_filter, pca, nmf, samplify, hpss, melbank, novelty and nn_search.h): the alignment test, the checked launch, the workspace refusal
// and the row-argument checks.  The network plans have plan_util.h; nothing here is for them.  A new kernel family starts from this
// header: its checks keep their own order and their own texts, and only what is one test with one text everywhere lives here.
#pragma once
#include "mmk_common.h"

namespace mmk {

// `bytes` is a power of two; a null pointer is aligned (an optional argument passes, a required one is refused by its null check)
inline bool misaligned(const void* p, size_t bytes) { return (reinterpret_cast<uintptr_t>(p) & (uintptr_t)(bytes - 1)) != 0; }

// one launch and its check: MMK_TRY(launch(kernel, grid, wg, lds, st, args...)), a template kernel as launch(kernel<KP, 0>, ...)
template <typename... K, typename... A>
inline int launch(void (*kernel)(K...), dim3 grid, dim3 wg, size_t lds, hipStream_t st, A... args) {
  hipLaunchKernelGGL(kernel, grid, wg, lds, st, args...);
  MMK_HIP(hipGetLastError());
  return MMK_OK;
}

// the workspace of a *_workspace_bytes entry point: there, `align`-byte aligned and of at least `need` bytes
inline int workspace_check(const char* who, const void* workspace, size_t align, size_t given, size_t need) {
  if (!workspace || misaligned(workspace, align) || given < need)
    return fail(MMK_ERR_WORKSPACE, "%s: the workspace has %zu bytes, %zu are needed", who, given, need);
  return MMK_OK;
}

// (batch, n) rows x -> (batch, n_y) rows y, both strided views of float32 tensors; need_n: an empty row is refused here too.  The limit
// of a launch differs per kernel and stays with it
inline int rows_check(const char* who, const void* x, int64_t x_row_stride, int32_t batch, int64_t n, const void* y, int64_t y_row_stride,
                      int64_t n_y, bool need_n) {
  if (!x || !y || batch <= 0 || (need_n && n <= 0) || (batch > 1 && (x_row_stride < 0 || y_row_stride < n_y)))
    return fail(MMK_ERR_INVALID, "%s: bad arguments (batch=%d, n=%lld, row strides %lld / %lld)", who, batch, (long long)n,
                (long long)x_row_stride, (long long)y_row_stride);
  if (misaligned(x, 4) || misaligned(y, 4)) return fail(MMK_ERR_INVALID, "%s: x and y must be 4-byte aligned", who);
  return MMK_OK;
}

}  // namespace mmk
