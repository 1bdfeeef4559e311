// SimpleTransformer step kernels (transformer.hip): causal multi-head attention on the fp32 matrix cores, fused residual add +
// LayerNorm, and the window inputs (embedding gather / frame gather + positional encoding).
#pragma once
#include "mmk_common.h"

namespace mmk {

// Causal multi-head attention of one window per clip.  Query row i (0 <= i < n_q) of clip b sits at q + b q_cs + i q_ld and is the
// window position q_pos0 + i: it sees keys 0 .. q_pos0 + i.  Key / value row j at k / v + b kv_cs + j kv_ld; head h reads and writes
// the columns [h head_dim, (h + 1) head_dim) of every row.  Output row i at out + b o_cs + i o_ld.
struct TrAttnArgs {
  const float* q;
  int64_t q_ld, q_cs;
  const float* k;
  const float* v;
  int64_t kv_ld, kv_cs;
  float* out;
  int64_t o_ld, o_cs;
  int32_t n_q, q_pos0, n_keys, n_heads, head_dim;
  float scale;
};
int launch_tr_attention(const TrAttnArgs& a, int batch, hipStream_t stream);
// once per plan, before the first launch (outside a graph capture): the kernel's LDS limit for this head_dim
int prepare_tr_attention(int head_dim);

// out[r] = LayerNorm(y[r] (+ res[r])) * w + b over D columns (eps 1e-5); res == nullptr: no residual.  out may alias res.
int launch_tr_add_ln(const float* y, int64_t y_ld, const float* res, int64_t res_ld, const float* w, const float* b, float* out,
                     int64_t out_ld, int rows, int D, hipStream_t stream);

// X0[b rf + t] = table[x[b][tau + t]] + pe[t]: the window of step tau (*tau_ptr) of clip b starts at x + b x_bs, positions x_ts apart
int launch_tr_embed_pe(const int64_t* x, int64_t x_bs, int64_t x_ts, const int64_t* tau_ptr, const float* table, int n_classes,
                       const float* pe, float* out, int B, int rf, int D, hipStream_t stream);
// out[b rf + t][c] = x[b][tau + t][c] for c < n_bins, zeros up to out_ld (the A operand of the input Linear)
int launch_tr_gather_frames(const float* x, int64_t x_bs, int64_t x_ts, const int64_t* tau_ptr, int n_bins, float* out, int out_ld,
                            int B, int rf, hipStream_t stream);
// x[b rf + t] += pe[t]
int launch_tr_add_pe(float* x, const float* pe, int B, int rf, int D, hipStream_t stream);

}  // namespace mmk
