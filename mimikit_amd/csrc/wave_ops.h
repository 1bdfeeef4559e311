// Wave-level primitives of the kernels (gfx950, 64 lanes = 4 DPP rows of 16), once: the DPP row moves, the sums and reduce-scatters
// inside a row, and the butterflies and the scan across the whole wave.  Every function has ONE fixed order of additions.
// Look-alikes that are other operations, and stay where they are:
//   * transformer.hip's attention takes a MAXIMUM over lanes n, n + 16, n + 32, n + 48; nn_search.h joins (key, index) lists with
//     the lane 32 further only;
//   * filters.hip's lf_wave_scan is a scan that multiplies by powers;
//   * sampler256.h's wave_max_dpp / wave_scan_dpp / wave_argmax_first go through the DPP rows and four scalar reads, where wave_max
//     and wave_incl_scan go through ds_bpermute (and the scan adds in another order);
//   * beside block_sum: kmeans.hip's reduce_slabs is a tree in LDS and adds in another order, samplify.hip's block_scan_incl / block_max /
//     block_arg are integer or argmax forms, and the Hillis-Steele scans of hcluster.hip and neighbors.hip differ from each other too.
// The general class picker, still written out at five sites (wavenet_persist.hip, wavenet_chain.hip, srnn_bottom.hip twice,
// srnn_resident.hip), uses the named moves and wave_max; its scan and its index butterflies are still its own loops: as shared calls they change
// the instruction streams of those kernels (so does wave_max in srnn_resident.hip alone, which keeps that loop too).
#pragma once
#include <hip/hip_runtime.h>

namespace mmk {

// ---- DPP moves: lane l receives the value of the lane that `CTRL` names; a lane without a source (shifts, masked rows) keeps `old` -------
constexpr int kDppXor1 = 0xB1;                              // quad_perm [1,0,3,2]: lane ^ 1
constexpr int kDppXor2 = 0x4E;                              // quad_perm [2,3,0,1]: lane ^ 2
constexpr int kDppHalfMirror = 0x141;                       // row_half_mirror: 7 - l inside each half row
constexpr int kDppMirror = 0x140;                           // row_mirror: 15 - l inside the row
constexpr int kDppWaveShr1 = 0x138;                         // wave_shr:1: lane l - 1 of the wave
constexpr int kDppRowBcast15 = 0x142, kDppRowBcast31 = 0x143;
constexpr int dpp_row_shl(int n) { return 0x100 + n; }      // lane l + n of the row
constexpr int dpp_row_shr(int n) { return 0x110 + n; }      // lane l - n of the row

template <int CTRL, int ROW_MASK = 0xf, bool BOUND_CTRL = false>
__device__ __forceinline__ int dpp_move(int v, int old = 0) {
  return __builtin_amdgcn_update_dpp(old, v, CTRL, ROW_MASK, 0xf, BOUND_CTRL);
}
template <int CTRL, int ROW_MASK = 0xf, bool BOUND_CTRL = false>
__device__ __forceinline__ float dpp_move(float v, float old = 0.f) {
  return __int_as_float(__builtin_amdgcn_update_dpp(__float_as_int(old), __float_as_int(v), CTRL, ROW_MASK, 0xf, BOUND_CTRL));
}
// (every lane has a source in these four, so `old` never shows in a result - but it is an operand of the instruction: 0 costs a
//  register write, the value itself ties the destination to the source.  Each site keeps the one it was tuned with.)
__device__ __forceinline__ float dpp_xor1(float v, float old = 0.f) { return dpp_move<kDppXor1>(v, old); }
__device__ __forceinline__ float dpp_xor2(float v, float old = 0.f) { return dpp_move<kDppXor2>(v, old); }
__device__ __forceinline__ float dpp_half_mirror(float v, float old = 0.f) { return dpp_move<kDppHalfMirror>(v, old); }
__device__ __forceinline__ float dpp_mirror(float v, float old = 0.f) { return dpp_move<kDppMirror>(v, old); }
__device__ __forceinline__ int dpp_xor1(int v, int old = 0) { return dpp_move<kDppXor1>(v, old); }
__device__ __forceinline__ int dpp_xor2(int v, int old = 0) { return dpp_move<kDppXor2>(v, old); }
__device__ __forceinline__ int dpp_half_mirror(int v, int old = 0) { return dpp_move<kDppHalfMirror>(v, old); }
__device__ __forceinline__ int dpp_mirror(int v, int old = 0) { return dpp_move<kDppMirror>(v, old); }

// (the readlane builtin is an integer one: a float argument would be CONVERTED, not reinterpreted)
__device__ __forceinline__ float readlane_f(float v, int lane) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), lane)); }

// ---- inside a row of 16 lanes ---------------------------------------------------------------------------------------------------------
// sum over the four lanes of a quad, in every lane of it
__device__ __forceinline__ float quad_sum(float v) {
  v += dpp_xor1(v);
  v += dpp_xor2(v);
  return v;
}
// sum over the 16 lanes of a row, in every lane of it: the quad, + the half-mirror partner, + the mirror partner
__device__ __forceinline__ float row_sum(float v) {
  v = quad_sum(v);
  v += dpp_half_mirror(v);
  v += dpp_mirror(v);
  return v;
}

// Four partial sums per lane, 16 lanes (one DPP row) that each hold a different K slice: add them up across the row and leave column c's
// total in lanes 4 c .. 4 c + 3 of the row (lane l of the wave ends with column l / 4 of the wave's 16).  Fixed order: own + mirror
// partner, + half-mirror partner, then the quad.  A lane reads 1/4 of the inputs it would need with one column per lane: the LDS, which
// all four SIMDs share, is what bounds a visit otherwise.
__device__ __forceinline__ float row_reduce_scatter4(float v0, float v1, float v2, float v3, int ks) {
  const bool hi = (ks & 8) != 0, q4 = (ks & 4) != 0;
  float t0 = hi ? v2 : v0, t1 = hi ? v3 : v1;
  const float u0 = hi ? v0 : v2, u1 = hi ? v1 : v3;
  t0 += dpp_mirror(u0);
  t1 += dpp_mirror(u1);
  float w = q4 ? t1 : t0;
  const float sd = q4 ? t0 : t1;
  w += dpp_half_mirror(sd);
  return quad_sum(w);
}
// two partial sums per lane: lanes 0-7 of the row end with column 0's total, lanes 8-15 with column 1's
__device__ __forceinline__ float row_reduce_scatter2(float v0, float v1, int ks) {
  const bool hi = (ks & 8) != 0;
  float t = hi ? v1 : v0;
  const float u = hi ? v0 : v1;
  t += dpp_mirror(u);
  t += dpp_half_mirror(t);
  return quad_sum(t);
}
// eight partial sums per lane: lanes 2 c, 2 c + 1 of the row end with column c's total (own + mirror partner, + half-mirror partner, + the lane
// two further, + the neighbour)
__device__ __forceinline__ float row_reduce_scatter8(const float (&v)[8], int ks) {
  const bool b3 = (ks & 8) != 0, b2 = (ks & 4) != 0, b1 = (ks & 2) != 0;
  float k4[4], k2[2];
#pragma unroll
  for (int i = 0; i < 4; ++i) k4[i] = (b3 ? v[4 + i] : v[i]) + dpp_mirror(b3 ? v[i] : v[4 + i]);
#pragma unroll
  for (int i = 0; i < 2; ++i) k2[i] = (b2 ? k4[2 + i] : k4[i]) + dpp_half_mirror(b2 ? k4[i] : k4[2 + i]);
  float r = (b1 ? k2[1] : k2[0]) + dpp_xor2(b1 ? k2[0] : k2[1]);
  r += dpp_xor1(r);
  return r;
}

// ---- across the wave (ds_bpermute) ----------------------------------------------------------------------------------------------------
// sum / maximum over the 64 lanes, the same in every lane: the xor butterfly, steps 32 down to 1
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}
// float64 sum over the workgroup (pca.hip, nmf.hip): the same butterfly, then the waves' sums in rising order; every thread gets the sum.
// `red` holds blockDim.x / 64 doubles
__device__ __forceinline__ double block_sum(double v, double* red) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off);
  const int nw = blockDim.x >> 6;
  __syncthreads();                                   // (red may still be read from the call before)
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  double s = 0.0;
  for (int w = 0; w < nw; ++w) s += red[w];
  return s;
}
// 1 / |row|_2 of K floats at p, 0 for a row of norm 0: lane l adds the squares of bins l, l + 64, ... in turn, the butterfly joins the lanes.
// The whole of inv_row_norm_kernel (nnn.hip); novelty.hip calls it for the rows of a tile where the caller passes no norms.
__device__ __forceinline__ float wave_inv_row_norm(const float* __restrict__ p, int K, int lane) {
  float a = 0.f;
  for (int k = lane; k < K; k += 64) {
    const float v = p[k];
    a = fmaf(v, v, a);
  }
  a = wave_sum(a);
  return a > 0.f ? 1.0f / sqrtf(a) : 0.f;
}
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o));
  return v;
}
// inclusive prefix sum over the lanes: Hillis-Steele, steps 1 up to 32
__device__ __forceinline__ float wave_incl_scan(float v, int lane) {
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const float up = __shfl_up(v, o);
    if (lane >= o) v += up;
  }
  return v;
}
// sum over the four K sub-slices of the 4x4-block MFMA layout (lanes n, n + 16, n + 32, n + 48), in each of them: ((0 + 1) + (2 + 3))
__device__ __forceinline__ float subslice_sum(float v) {
  v += __shfl_xor(v, 16);
  v += __shfl_xor(v, 32);
  return v;
}

}  // namespace mmk
