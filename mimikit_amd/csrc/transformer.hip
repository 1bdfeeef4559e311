// SimpleTransformer step kernels (gfx950).
//
// Attention: one workgroup of four waves takes 64 query rows of one (clip, head); each wave owns 16 of them.  Keys and values come in
// tiles of 64 rows through LDS (shared by the four waves), and every wave walks its tile in sub-tiles of 16 keys on
// v_mfma_f32_16x16x4_f32 (exact fp32 fmaf chains):
//   * S^T = K Q^T: A = K (row = key, lane & 15), B = Q^T (column = query, lane & 15), one MFMA per 4 head channels.  A lane then holds
//     S[query lane & 15][key 4 (lane >> 4) + r] in register r: the softmax statistics of its query sit in its own lane (plus the three
//     lanes 16, 32, 48 apart), no LDS round trip.
//   * online, max-subtracted softmax in fp32 (running max m, running sum l, the accumulators rescaled by exp(m_old - m_new));
//   * O^T += V^T P^T: A = V^T (row = channel, lane & 15), B = P^T taken straight from the S registers (register r = k slot of MFMA r),
//     so the output row of a lane is again its query.
//   Sub-tiles beyond a wave's last visible key are skipped, tiles beyond the workgroup's are never loaded: rf up to 2048 needs 2 x 64 key
//   rows of LDS whatever the window.
// Residual add + LayerNorm: one wave per row, the row in registers, mean then centred second moment in fp32.
#include "transformer.h"
#include "wave_ops.h"

namespace mmk {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int kAttnRows = 64;      // query rows per workgroup (16 per wave)
constexpr int kAttnKeys = 64;      // key rows per LDS tile

template <int NC>    // NC >= head_dim / 4 (head channels in groups of 4: one MFMA each)
__global__ __launch_bounds__(256) void tr_attention_kernel(const TrAttnArgs a) {
  extern __shared__ float smem[];
  constexpr int ND = (4 * NC + 15) / 16;                       // 16-wide channel tiles of the output
  const int hd = a.head_dim;
  const int nc = hd >> 2;
  const int lds_ld = hd + 1;                                   // odd row stride: the 16 key rows of a K read hit 16 banks
  float* ks = smem;
  float* vs = smem + kAttnKeys * lds_ld;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int g = lane >> 4, li = lane & 15;
  const int b = blockIdx.z, h = blockIdx.y;
  const int qblk = blockIdx.x * kAttnRows;
  const int qrow0 = qblk + wave * 16;
  const int my_row = qrow0 + li;
  const bool row_ok = my_row < a.n_q;
  const int my_pos = row_ok ? a.q_pos0 + my_row : 0;          // (rows beyond n_q see key 0 only: finite, never stored)
  const int blk_last = min(qblk + kAttnRows, a.n_q) - 1;
  const int kend = min(a.q_pos0 + blk_last + 1, a.n_keys);     // keys this workgroup needs
  const int wave_kend = qrow0 < a.n_q ? min(a.q_pos0 + min(qrow0 + 15, a.n_q - 1) + 1, a.n_keys) : 0;
  const int hoff = h * hd;

  float qv[NC];
  {
    const float* qp = a.q + (int64_t)b * a.q_cs + (int64_t)(row_ok ? my_row : 0) * a.q_ld + hoff;
#pragma unroll
    for (int c = 0; c < NC; ++c) qv[c] = (row_ok && c < nc) ? qp[4 * c + g] : 0.f;
  }
  float m_i = -INFINITY, l_i = 0.f;
  f32x4 o[ND];
#pragma unroll
  for (int dt = 0; dt < ND; ++dt) o[dt] = f32x4{0.f, 0.f, 0.f, 0.f};
  const float* kbase = a.k + (int64_t)b * a.kv_cs + hoff;
  const float* vbase = a.v + (int64_t)b * a.kv_cs + hoff;

  for (int t0 = 0; t0 < kend; t0 += kAttnKeys) {
    __syncthreads();                                           // every wave is done with the previous tile
    const int nk = min(kAttnKeys, kend - t0);
    for (int e = tid; e < kAttnKeys * hd; e += 256) {
      const int jj = e / hd, d = e - jj * hd;
      float kx = 0.f, vx = 0.f;
      if (jj < nk) {
        const int64_t off = (int64_t)(t0 + jj) * a.kv_ld + d;
        kx = kbase[off];
        vx = vbase[off];
      }
      ks[jj * lds_ld + d] = kx;
      vs[jj * lds_ld + d] = vx;
    }
    __syncthreads();
#pragma unroll 1
    for (int sub = 0; sub < kAttnKeys / 16; ++sub) {
      const int j0 = t0 + sub * 16;
      if (j0 >= wave_kend) break;                              // wave-uniform: every key from here on is masked for all 16 rows
      f32x4 s = f32x4{0.f, 0.f, 0.f, 0.f};
      const float* kr = ks + (sub * 16 + li) * lds_ld + g;
#pragma unroll
      for (int c = 0; c < NC; ++c)
        if (c < nc) s = __builtin_amdgcn_mfma_f32_16x16x4f32(kr[4 * c], qv[c], s, 0, 0, 0);
      float p[4];
      float tmax = -INFINITY;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int j = j0 + 4 * g + r;
        const float x = (j > my_pos || j >= a.n_keys) ? -INFINITY : s[r] * a.scale;
        p[r] = x;
        tmax = fmaxf(tmax, x);
      }
      tmax = fmaxf(tmax, __shfl_xor(tmax, 16));
      tmax = fmaxf(tmax, __shfl_xor(tmax, 32));
      // key j0 = 0 is visible to every row, so m is finite from the first sub-tile on
      const float m_new = fmaxf(m_i, tmax);
      const float alpha = m_i == -INFINITY ? 0.f : expf(m_i - m_new);
      float rs = 0.f;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        p[r] = expf(p[r] - m_new);
        rs += p[r];
      }
      rs = subslice_sum(rs);
      l_i = l_i * alpha + rs;
      m_i = m_new;
#pragma unroll
      for (int dt = 0; dt < ND; ++dt) o[dt] *= alpha;
      const float* vr = vs + (sub * 16 + 4 * g) * lds_ld + li;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
#pragma unroll
        for (int dt = 0; dt < ND; ++dt) {
          const float vx = dt * 16 + li < hd ? vr[r * lds_ld + dt * 16] : 0.f;
          o[dt] = __builtin_amdgcn_mfma_f32_16x16x4f32(vx, p[r], o[dt], 0, 0, 0);
        }
      }
    }
  }
  if (!row_ok) return;
  const float inv = 1.f / l_i;
  float* op = a.out + (int64_t)b * a.o_cs + (int64_t)my_row * a.o_ld + hoff;
#pragma unroll
  for (int dt = 0; dt < ND; ++dt)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int d = dt * 16 + 4 * g + r;
      if (d < hd) op[d] = o[dt][r] * inv;
    }
}

size_t tr_attention_lds_bytes(int head_dim) { return (size_t)2 * kAttnKeys * (head_dim + 1) * sizeof(float); }

int prepare_tr_attention(int head_dim) {
  // head_dim 128: 66 KiB of dynamic LDS.  ROCm launches a kernel with up to the CU's 160 KiB without this attribute (gemm_f32_kernel asks
  // for 157 KiB at K = 624 and sets none: tests/test_gpu_kernels_f64.py); it is set anyway, as the API's way of asking for more than 64 KiB
  const size_t lds = tr_attention_lds_bytes(head_dim);
  if (lds > 65536)
    MMK_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&tr_attention_kernel<32>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  return MMK_OK;
}

int launch_tr_attention(const TrAttnArgs& a, int batch, hipStream_t stream) {
  if (batch <= 0 || a.n_q <= 0) return MMK_OK;
  if (a.head_dim < 4 || a.head_dim > 128 || a.head_dim % 4 != 0 || a.n_keys < 1)
    return fail(MMK_ERR_INVALID, "tr attention: head_dim %d, %d keys", a.head_dim, a.n_keys);
  dim3 grid((a.n_q + kAttnRows - 1) / kAttnRows, a.n_heads, batch), block(256);
  const size_t lds = tr_attention_lds_bytes(a.head_dim);
  const int nc = a.head_dim / 4;
  if (nc <= 2) hipLaunchKernelGGL(tr_attention_kernel<2>, grid, block, lds, stream, a);
  else if (nc <= 4) hipLaunchKernelGGL(tr_attention_kernel<4>, grid, block, lds, stream, a);
  else if (nc <= 8) hipLaunchKernelGGL(tr_attention_kernel<8>, grid, block, lds, stream, a);
  else if (nc <= 16) hipLaunchKernelGGL(tr_attention_kernel<16>, grid, block, lds, stream, a);
  else hipLaunchKernelGGL(tr_attention_kernel<32>, grid, block, lds, stream, a);
  MMK_HIP(hipGetLastError());
  return MMK_OK;
}

constexpr int kLnPer = 16;   // columns per lane: D <= 1024

// (no __restrict__: out may be res - a wave holds its whole row in registers before it writes)
__global__ __launch_bounds__(256) void tr_add_ln_kernel(const float* y, int64_t y_ld, const float* res, int64_t res_ld,
                                                        const float* __restrict__ w, const float* __restrict__ bb, float* out,
                                                        int64_t out_ld, int rows, int D) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  const float* yr = y + (int64_t)row * y_ld;
  const float* rr = res ? res + (int64_t)row * res_ld : nullptr;
  float v[kLnPer];
  float s = 0.f;
#pragma unroll
  for (int k = 0; k < kLnPer; ++k) {
    const int c = lane + 64 * k;
    float x = 0.f;
    if (c < D) {
      x = yr[c];
      if (rr) x = rr[c] + x;
    }
    v[k] = x;
    s += x;
  }
  const float mean = wave_sum(s) / (float)D;
  float q = 0.f;
#pragma unroll
  for (int k = 0; k < kLnPer; ++k) {
    const int c = lane + 64 * k;
    if (c < D) {
      const float d = v[k] - mean;
      q = fmaf(d, d, q);
    }
  }
  const float var = wave_sum(q) / (float)D;
  const float rstd = 1.f / sqrtf(var + 1e-5f);
  float* orow = out + (int64_t)row * out_ld;
#pragma unroll
  for (int k = 0; k < kLnPer; ++k) {
    const int c = lane + 64 * k;
    if (c < D) orow[c] = (v[k] - mean) * rstd * w[c] + bb[c];
  }
}

int launch_tr_add_ln(const float* y, int64_t y_ld, const float* res, int64_t res_ld, const float* w, const float* b, float* out,
                     int64_t out_ld, int rows, int D, hipStream_t stream) {
  if (rows <= 0) return MMK_OK;
  if (D < 1 || D > 64 * kLnPer) return fail(MMK_ERR_INVALID, "tr layer norm: %d columns (at most %d)", D, 64 * kLnPer);
  hipLaunchKernelGGL(tr_add_ln_kernel, dim3((rows + 3) / 4), dim3(256), 0, stream, y, y_ld, res, res_ld, w, b, out, out_ld, rows, D);
  MMK_HIP(hipGetLastError());
  return MMK_OK;
}

// nn.Embedding under ZipReduceVariables (weight 1 for one input), then + pe[0:rf] (transformers.py:160-164).  An index outside the
// table (torch raises for it) reads the nearest row.
__global__ void tr_embed_pe_kernel(const int64_t* __restrict__ x, int64_t x_bs, int64_t x_ts, const int64_t* __restrict__ tau_ptr,
                                   const float* __restrict__ table, int n_classes, const float* __restrict__ pe, float* __restrict__ out,
                                   int rf, int D) {
  const int row = blockIdx.x;
  const int b = row / rf, t = row - b * rf;
  const int64_t tau = *tau_ptr;
  int64_t k = x[(int64_t)b * x_bs + (tau + t) * x_ts];
  k = k < 0 ? 0 : (k >= n_classes ? n_classes - 1 : k);
  const float* src = table + k * D;
  const float* pr = pe + (int64_t)t * D;
  float* dst = out + (int64_t)row * D;
  for (int c = threadIdx.x; c < D; c += blockDim.x) dst[c] = src[c] * 1.f + pr[c];
}

int launch_tr_embed_pe(const int64_t* x, int64_t x_bs, int64_t x_ts, const int64_t* tau_ptr, const float* table, int n_classes,
                       const float* pe, float* out, int B, int rf, int D, hipStream_t stream) {
  if (B <= 0) return MMK_OK;
  hipLaunchKernelGGL(tr_embed_pe_kernel, dim3(B * rf), dim3(256), 0, stream, x, x_bs, x_ts, tau_ptr, table, n_classes, pe, out, rf, D);
  MMK_HIP(hipGetLastError());
  return MMK_OK;
}

__global__ void tr_gather_frames_kernel(const float* __restrict__ x, int64_t x_bs, int64_t x_ts, const int64_t* __restrict__ tau_ptr,
                                        int n_bins, float* __restrict__ out, int out_ld, int rf) {
  const int row = blockIdx.x;
  const int b = row / rf, t = row - b * rf;
  const float* src = x + (int64_t)b * x_bs + (*tau_ptr + t) * x_ts;
  float* dst = out + (int64_t)row * out_ld;
  for (int c = threadIdx.x; c < out_ld; c += blockDim.x) dst[c] = c < n_bins ? src[c] : 0.f;
}

int launch_tr_gather_frames(const float* x, int64_t x_bs, int64_t x_ts, const int64_t* tau_ptr, int n_bins, float* out, int out_ld,
                            int B, int rf, hipStream_t stream) {
  if (B <= 0) return MMK_OK;
  hipLaunchKernelGGL(tr_gather_frames_kernel, dim3(B * rf), dim3(128), 0, stream, x, x_bs, x_ts, tau_ptr, n_bins, out, out_ld, rf);
  MMK_HIP(hipGetLastError());
  return MMK_OK;
}

__global__ void tr_add_pe_kernel(float* __restrict__ x, const float* __restrict__ pe, int rf, int D) {
  const int row = blockIdx.x;
  const int t = row % rf;
  float* dst = x + (int64_t)row * D;
  const float* pr = pe + (int64_t)t * D;
  for (int c = threadIdx.x; c < D; c += blockDim.x) dst[c] = dst[c] + pr[c];
}

int launch_tr_add_pe(float* x, const float* pe, int B, int rf, int D, hipStream_t stream) {
  if (B <= 0) return MMK_OK;
  hipLaunchKernelGGL(tr_add_pe_kernel, dim3(B * rf), dim3(256), 0, stream, x, pe, rf, D);
  MMK_HIP(hipGetLastError());
  return MMK_OK;
}

}  // namespace mmk

extern "C" int mmk_tr_attention_f32(const float* q, int64_t q_ld, int64_t q_cs, const float* k, const float* v, int64_t kv_ld, int64_t kv_cs,
                                    float* out, int64_t o_ld, int64_t o_cs, int32_t n_q, int32_t q_pos0, int32_t n_keys, int32_t n_heads,
                                    int32_t head_dim, float scale, int32_t batch, mmk_stream_t stream) {
  using namespace mmk;
  if (!q || !k || !v || !out || n_q < 0 || q_pos0 < 0 || n_heads < 1 || batch < 0)
    return fail(MMK_ERR_INVALID, "tr attention: bad arguments");
  if (head_dim < 4 || head_dim > 128 || head_dim % 4 != 0 || n_keys < 1)
    return fail(MMK_ERR_INVALID, "tr attention: head_dim %d, %d keys", head_dim, n_keys);
  MMK_TRY(prepare_tr_attention(head_dim));
  TrAttnArgs a;
  a.q = q; a.q_ld = q_ld; a.q_cs = q_cs;
  a.k = k; a.v = v; a.kv_ld = kv_ld; a.kv_cs = kv_cs;
  a.out = out; a.o_ld = o_ld; a.o_cs = o_cs;
  a.n_q = n_q; a.q_pos0 = q_pos0; a.n_keys = n_keys; a.n_heads = n_heads; a.head_dim = head_dim;
  a.scale = scale;
  return launch_tr_attention(a, batch, (hipStream_t)stream);
}

extern "C" int mmk_tr_add_ln_f32(const float* y, int64_t y_ld, const float* res, int64_t res_ld, const float* w, const float* b, float* out,
                                 int64_t out_ld, int32_t rows, int32_t d, mmk_stream_t stream) {
  using namespace mmk;
  if (!y || !w || !b || !out || rows < 0) return fail(MMK_ERR_INVALID, "tr layer norm: bad arguments");
  return launch_tr_add_ln(y, y_ld, res, res_ld, w, b, out, out_ld, rows, d, (hipStream_t)stream);
}
