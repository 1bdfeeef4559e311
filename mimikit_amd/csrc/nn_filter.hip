// NearestNeighborFilter (mimikit/features/functionals.py:1083-1111; include/mmk_nn_filter.h): every frame replaced by the per-bin median,
// mean, max or min of the frames its k-nearest list names - optionally only those that name it back - in one launch behind mmk_nn_topk_f32.
//
//   nn_aggregate_kernel<OP>  one WAVE per output row, four rows per workgroup, no LDS and no barrier.
//     the list   lane p < t reads slot p of the row's list; a slot outside [0, n) or equal to the row is empty.  With `mutual`, lane l
//                compares the row number against slot (l >> 4) + 4 pass of the list of the row's slot l & 15, in four passes: t x t <= 256
//                comparisons, each pass one ballot, the four lanes of a slot folded by two shifts.  The mask of the slots that count is
//                wave-uniform from here on, and so is the count: the bin loop has no divergence.
//     the rows   lane k takes the k-th slot that counts (rising slot order) and its row's offset; the at most 16 offsets are then read
//                into scalar registers (readlane with a constant lane), once per row.
//     the bins   lanes stride over the bins, two bins 64 apart per lane and step: the 2 C loads of a step are issued before the first
//                use (the second bin is clamped into the row where the tail has none, and not stored).  The C values of a bin stay in
//                registers: the loop body is compiled once per count C = 1 .. 16 and entered through a switch on the uniform count, so
//                every index into the values is a constant (a runtime-indexed private array would live in scratch memory).
//                median: Batcher's odd-even merge network for 16 inputs without the comparators that touch an input >= C (63 at C = 16;
//                checked for every C by the 0-1 principle), compare-and-select so that only bits of x move; the middle one, or
//                (a + b) * 0.5f of the two middle ones - numpy's float32 mean of two.  max / min: a chain of compare-and-selects.
//                mean: a float64 chain in rising slot order, one division, one rounding.
//   Rows of 1025 floats are 4-byte aligned only: the loads and stores are one float per lane, 256 contiguous bytes per wave.
// No atomics, no workgroup waits for another; out must not alias x.  NaN is not handled.
#include "entry_util.h"

#include "../../include/mmk_nn_filter.h"

namespace mmk {

constexpr int kNfWaves = 4;                  // rows of a workgroup, one per wave
constexpr int kNfSlots = MMK_NN_TOPK_MAX;
static_assert(kNfSlots == 16, "the mutual test folds four lanes per slot, the network is the one for 16 inputs");

#define NF_CS(a, b)                          \
  if constexpr ((b) < C) {                   \
    const float lo__ = v[a], hi__ = v[b];    \
    const bool sw__ = hi__ < lo__;           \
    v[a] = sw__ ? hi__ : lo__;               \
    v[b] = sw__ ? lo__ : hi__;               \
  }

// the aggregate of the C values of one bin; every index is a constant
template <int OP, int C>
__device__ __forceinline__ float nf_aggregate(float (&v)[C]) {
  if constexpr (OP == MMK_NN_AGG_MEAN) {
    double s = (double)v[0];
#pragma unroll
    for (int k = 1; k < C; ++k) s += (double)v[k];
    return (float)(s / (double)C);
  } else if constexpr (OP == MMK_NN_AGG_MAX) {
    float m = v[0];
#pragma unroll
    for (int k = 1; k < C; ++k) m = v[k] > m ? v[k] : m;
    return m;
  } else if constexpr (OP == MMK_NN_AGG_MIN) {
    float m = v[0];
#pragma unroll
    for (int k = 1; k < C; ++k) m = v[k] < m ? v[k] : m;
    return m;
  } else {
    NF_CS(0, 1) NF_CS(2, 3) NF_CS(4, 5) NF_CS(6, 7) NF_CS(8, 9) NF_CS(10, 11) NF_CS(12, 13) NF_CS(14, 15)
    NF_CS(0, 2) NF_CS(1, 3) NF_CS(4, 6) NF_CS(5, 7) NF_CS(8, 10) NF_CS(9, 11) NF_CS(12, 14) NF_CS(13, 15)
    NF_CS(1, 2) NF_CS(5, 6) NF_CS(9, 10) NF_CS(13, 14)
    NF_CS(0, 4) NF_CS(1, 5) NF_CS(2, 6) NF_CS(3, 7) NF_CS(8, 12) NF_CS(9, 13) NF_CS(10, 14) NF_CS(11, 15)
    NF_CS(2, 4) NF_CS(3, 5) NF_CS(10, 12) NF_CS(11, 13)
    NF_CS(1, 2) NF_CS(3, 4) NF_CS(5, 6) NF_CS(9, 10) NF_CS(11, 12) NF_CS(13, 14)
    NF_CS(0, 8) NF_CS(1, 9) NF_CS(2, 10) NF_CS(3, 11) NF_CS(4, 12) NF_CS(5, 13) NF_CS(6, 14) NF_CS(7, 15)
    NF_CS(4, 8) NF_CS(5, 9) NF_CS(6, 10) NF_CS(7, 11)
    NF_CS(2, 4) NF_CS(3, 5) NF_CS(6, 8) NF_CS(7, 9) NF_CS(10, 12) NF_CS(11, 13)
    NF_CS(1, 2) NF_CS(3, 4) NF_CS(5, 6) NF_CS(7, 8) NF_CS(9, 10) NF_CS(11, 12) NF_CS(13, 14)
    if constexpr (C % 2 == 1) return v[C / 2];
    return (v[C / 2 - 1] + v[C / 2]) * 0.5f;
  }
}
#undef NF_CS

// one output row from its C neighbour rows; lane k < C holds the k-th neighbour's offset into x
template <int OP, int C>
__device__ __forceinline__ void nf_row(const float* __restrict__ x, int64_t my_off, int32_t d, float* __restrict__ orow, int lane) {
  const float* nb[C];
#pragma unroll
  for (int k = 0; k < C; ++k) {
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)my_off, k);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)((uint64_t)my_off >> 32), k);
    nb[k] = x + (int64_t)(((uint64_t)hi << 32) | lo);
  }
  for (int32_t b = lane; b < d; b += 128) {
    const bool two = b + 64 < d;
    const int32_t b1 = two ? b + 64 : d - 1;           // inside the row: loaded whatever `two` says, stored only with it
    float v0[C], v1[C];
#pragma unroll
    for (int k = 0; k < C; ++k) v0[k] = nb[k][b];
#pragma unroll
    for (int k = 0; k < C; ++k) v1[k] = nb[k][b1];
    orow[b] = nf_aggregate<OP, C>(v0);
    const float r1 = nf_aggregate<OP, C>(v1);
    if (two) orow[b + 64] = r1;
  }
}

template <int OP>
__global__ __launch_bounds__(64 * kNfWaves) void nn_aggregate_kernel(const float* __restrict__ x, int64_t x_row_stride, int64_t n, int32_t d,
                                                                     const int64_t* __restrict__ index, int32_t t, int32_t mutual,
                                                                     float* __restrict__ out, int64_t out_row_stride, int32_t* __restrict__ count) {
  const int lane = (int)(threadIdx.x & 63), wave = (int)(threadIdx.x >> 6);
  const int64_t i = (int64_t)blockIdx.x * kNfWaves + wave;
  if (i >= n) return;                                   // (no barrier below)
  long long j = -1;
  if (lane < t) j = index[i * t + lane];
  const bool valid = lane < t && j >= 0 && j < n && j != i;
  const uint32_t listed = (uint32_t)__ballot(valid) & 0xffffu;
  uint32_t mask = listed;
  if (mutual) {
    const int p = lane & 15;
    const long long jp = __shfl(j, p);
    const bool look = ((listed >> p) & 1u) != 0;        // never an address from an empty slot
    unsigned long long hit = 0;
#pragma unroll
    for (int pass = 0; pass < 4; ++pass) {
      const int q = (lane >> 4) + 4 * pass;
      bool h = false;
      if (look && q < t) h = index[jp * t + q] == i;
      hit |= __ballot(h);
    }
    hit |= hit >> 32;
    hit |= hit >> 16;
    mask = listed & (uint32_t)hit;
  }
  mask = (uint32_t)__builtin_amdgcn_readfirstlane((int)mask);
  const int c = __popc(mask);
  if (count && lane == 0) count[i] = c;
  float* orow = out + i * out_row_stride;
  if (c == 0) {
    const float* xrow = x + i * x_row_stride;
    for (int32_t b = lane; b < d; b += 64) orow[b] = xrow[b];
    return;
  }
  // lane k: the k-th slot that counts, in rising slot order
  int pos = -1, seen = 0;
#pragma unroll
  for (int p = 0; p < kNfSlots; ++p) {
    if ((mask >> p) & 1u) {
      if (seen == lane) pos = p;
      ++seen;
    }
  }
  const long long jk = __shfl(j, pos < 0 ? 0 : pos);
  const int64_t my_off = pos < 0 ? 0 : (int64_t)jk * x_row_stride;
  switch (c) {
#define NF_CASE(C) case C: nf_row<OP, C>(x, my_off, d, orow, lane); break;
    NF_CASE(1) NF_CASE(2) NF_CASE(3) NF_CASE(4) NF_CASE(5) NF_CASE(6) NF_CASE(7) NF_CASE(8)
    NF_CASE(9) NF_CASE(10) NF_CASE(11) NF_CASE(12) NF_CASE(13) NF_CASE(14) NF_CASE(15) NF_CASE(16)
#undef NF_CASE
    default: break;
  }
}

}  // namespace mmk

using namespace mmk;

extern "C" int mmk_nn_aggregate_f32(const float* x, int64_t x_row_stride, int64_t n, int32_t d, const int64_t* index, int32_t t, int32_t mutual,
                                    int32_t op, float* out, int64_t out_row_stride, int32_t* count, mmk_stream_t stream) {
  if (n < 1 || d < 1 || t < 1) return fail(MMK_ERR_INVALID, "nn_aggregate: n = %lld, d = %d, t = %d (all at least 1)", (long long)n, d, t);
  if (t > MMK_NN_TOPK_MAX)
    return fail(MMK_ERR_UNSUPPORTED, "nn_aggregate: t = %d slots per row, more than the %d (MMK_NN_TOPK_MAX) a wave keeps in registers", t, MMK_NN_TOPK_MAX);
  if (op != MMK_NN_AGG_MEDIAN && op != MMK_NN_AGG_MEAN && op != MMK_NN_AGG_MAX && op != MMK_NN_AGG_MIN)
    return fail(MMK_ERR_UNSUPPORTED, "nn_aggregate: op = %d is none of MMK_NN_AGG_MEDIAN, _MEAN, _MAX, _MIN", op);
  if (!x || !index || !out || x_row_stride < 0 || (out_row_stride < d && n > 1))
    return fail(MMK_ERR_INVALID, "nn_aggregate: bad arguments (null pointer, x_row_stride %lld < 0 or out_row_stride %lld < d = %d)",
                (long long)x_row_stride, (long long)out_row_stride, d);
  if (misaligned(x, 4) || misaligned(out, 4) || misaligned(count, 4)) return fail(MMK_ERR_INVALID, "nn_aggregate: x, out and count must be 4-byte aligned");
  if (misaligned(index, 8)) return fail(MMK_ERR_INVALID, "nn_aggregate: index must be 8-byte aligned");
  if (x == out) return fail(MMK_ERR_INVALID, "nn_aggregate: out must not alias x");
  const int64_t n_blocks = (n + kNfWaves - 1) / kNfWaves;
  if (n_blocks > 0x7fffffffLL) return fail(MMK_ERR_UNSUPPORTED, "nn_aggregate: %lld rows are more than one launch takes", (long long)n);
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid((unsigned)n_blocks), block(64 * kNfWaves);
#define NF_LAUNCH(OP) \
  launch(nn_aggregate_kernel<OP>, grid, block, 0, st, x, x_row_stride, n, d, index, t, mutual, out, out_row_stride, count)
  switch (op) {
    case MMK_NN_AGG_MEDIAN: return NF_LAUNCH(MMK_NN_AGG_MEDIAN);
    case MMK_NN_AGG_MEAN: return NF_LAUNCH(MMK_NN_AGG_MEAN);
    case MMK_NN_AGG_MAX: return NF_LAUNCH(MMK_NN_AGG_MAX);
    default: return NF_LAUNCH(MMK_NN_AGG_MIN);
  }
#undef NF_LAUNCH
}
