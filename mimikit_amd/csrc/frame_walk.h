// The walk over the bins that every kernel multiplying fp32 frames against fp32 frames makes, written once: nn_search_kernel (nn_search.h),
// nn_cosine_kernel (neighbors.hip), kmeans_assign_kernel (kmeans.hip) and novelty_kernel (novelty.hip) are built from these pieces and own
// only their tile shape, who holds which rows, and their epilogue.
//
//   staging     Rows go through LDS in chunks of kFwKC = 32 bins at a pitch of kFwPitch = 36 floats.  A thread loads dword by dword, bin
//               `col` of rows row0, row0 + RS, ...: consecutive lanes on consecutive bins, coalesced whatever the row stride and the base
//               alignment.  Every load is unconditional at a clamped, valid address (fw_load); afterwards the kernel's store picks zero
//               where the bin or the row lies outside - rows[(i RS + row0) kFwPitch + col] = (bin and row inside) ? rg[i] : 0 - so nothing
//               is padded by the caller.  That one statement per operand stays in the kernels: as a function of this header, in every
//               form tried, it is compiled into other control flow and moves the register counts of half the instances.
//               A kernel issues the next chunk's fw_load behind the barrier that follows the stores, so those loads are in flight while
//               this chunk's products run.
//   products    Lane (fr = l & 31, fh = l >> 5) reads bins g + 4 fh .. + 3 of row fr of each operand as one 16-byte LDS read per group g of
//               8 bins (fw_frag) and feeds MFMA e of the group with bin g + 4 fh + e (fw_mfma: v_mfma_f32_32x32x2_f32) - the same
//               permutation of the bins on both operands and for every row, so ONE order of the sum over the bins wherever a frame sits
//               in a tile: two identical frames have bit-identical sums, in every kernel built from this header.  A bin that a kernel
//               leaves out (the narrow form of kmeans.hip) is a product with zero.
//   accumulator With A = the rows that end up in the registers and B = the rows that end up on the lanes, register q of lane l holds row
//               fw_acc_row(0, q, l >> 5) = (q & 3) + 8 (q >> 2) + 4 (l >> 5) of A's 32 against row l & 31 of B's: rising with q inside a lane.
#pragma once
#include "mmk_common.h"

namespace mmk {

typedef float fw_f32x4 __attribute__((ext_vector_type(4)));
typedef float fw_f32x16 __attribute__((ext_vector_type(16)));

constexpr int kFwKC = 32;         // bins per LDS chunk: four groups of 8, and one dword per lane of a half-wave and row
constexpr int kFwPitch = 36;      // floats between LDS rows: 16-byte aligned, and the 16 lanes of one read group fall into 64 different banks

// (base: the first of A's 32 rows; the sum is formed in this order, base first)
__device__ __forceinline__ int fw_acc_row(int base, int q, int fh) { return base + (q & 3) + 8 * (q >> 2) + 4 * fh; }

__device__ __forceinline__ int fw_bin(int k, int K) { return k < K ? k : K - 1; }

// rg[OFF + i] = post(bin k0 + col of row base + i * RS + row0 of src) for i < N, the row clamped below n (kBelow: and at 0), the bin below K.
// post: what a kernel makes of the dword while it is loaded (kmeans.hip subtracts the offset), nothing by default
struct FwAsLoaded {
  __device__ __forceinline__ float operator()(float v) const { return v; }
};
template <int N, int RS, int OFF, bool kBelow = false, int NR, class I, class Post = FwAsLoaded>
__device__ __forceinline__ void fw_load(float (&rg)[NR], const float* __restrict__ src, int64_t row_stride, I base, I n, int row0, int col, int k0,
                                        int K, Post post = Post{}) {
  static_assert(OFF + N <= NR, "the loads fit the register array");
  const int kc = fw_bin(k0 + col, K);
#pragma unroll
  for (int i = 0; i < N; ++i) {
    const I r = base + i * RS + row0;
    if constexpr (kBelow) rg[OFF + i] = post(src[(int64_t)(r < 0 ? 0 : (r < n ? r : n - 1)) * row_stride + kc]);
    else rg[OFF + i] = post(src[(int64_t)(r < n ? r : n - 1) * row_stride + kc]);
  }
}

// bins g + 4 fh .. + 3 of staged row `row`
__device__ __forceinline__ fw_f32x4 fw_frag(const float* rows, int row, int g, int fh) {
  return *reinterpret_cast<const fw_f32x4*>(&rows[row * kFwPitch + g + 4 * fh]);
}

// product e of a group of bins: bin g + 4 fh + e of both fragments.  A kernel that holds independent accumulators interleaves them itself,
// e outermost (for e, for accumulator: fw_mfma); fw_mma is the four products of one fragment pair into one accumulator
__device__ __forceinline__ void fw_mfma(fw_f32x16& acc, const fw_f32x4 a, const fw_f32x4 b, int e) {
  acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[e], b[e], acc, 0, 0, 0);
}
__device__ __forceinline__ void fw_mma(fw_f32x16& acc, const fw_f32x4 a, const fw_f32x4 b) {
#pragma unroll
  for (int e = 0; e < 4; ++e) fw_mfma(acc, a, b, e);
}

}  // namespace mmk
