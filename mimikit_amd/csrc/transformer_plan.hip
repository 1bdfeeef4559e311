// SimpleTransformer generate plan (host side).
//
// Reference: SimpleTransformer.forward (transformers.py:159-178) over nn.TransformerDecoder (post-norm layers, ReLU, LayerNorm eps
// 1e-5) with tgt = memory = X0 = input(x[t-rf:t]) + pe[0:rf] and the causal mask on both attentions.  Every step recomputes the whole
// window - the same arithmetic as the reference, no key / value cache (the positional encoding is tied to window positions, so every
// key changes at every step).  Per step, for B clips and M = B rf rows:
//   X0 (embedding gather or Linear over the frames, + pe)          1 - 3 launches
//   the cross-attention keys / values of ALL layers from X0        one GEMM, N = 2 D L
//   each layer but the last: QKV GEMM, attention, out-projection, add + LN1, CA query GEMM, attention, out-projection, add + LN2,
//     FFN (two GEMMs, ReLU in the first one's epilogue), add + LN3
//   the last layer: the QKV GEMM over all rows (its keys / values), everything else for the last query row only (M = B)
//   final LayerNorm (with_layer_norm), the head, the sampler / Abs - written into the loop's tensor at t.
// A generate block is one serial stream of launches, replayed as a hipGraph of kGraphSteps steps (no parallel branches); the step
// position is a device counter every step kernel reads.
#include "plan_util.h"
#include "transformer.h"

using namespace mmk;

namespace {
constexpr int kGraphSteps = 8;
}

struct TrLayer {
  PackedLinear qkv, o_sa, q_ca, o_ca, ff1, ff2;
  float* ln_w[3] = {nullptr, nullptr, nullptr};
  float* ln_b[3] = {nullptr, nullptr, nullptr};
};

// everything the workspace holds (carved twice: once to size it, once to place it)
struct TrState {
  std::vector<TrLayer> layers;
  PackedLinear kv_ca, in_lin, out_lin;
  MlpHead head;
  float *embed = nullptr, *pe = nullptr, *fn_w = nullptr, *fn_b = nullptr;
  float *x0 = nullptr, *x = nullptr, *qkv = nullptr, *att = nullptr, *tmp = nullptr, *qc = nullptr, *hff = nullptr, *kvc = nullptr;
  float* frames = nullptr;
  float *xl = nullptr, *att_l = nullptr, *tmp_l = nullptr, *qc_l = nullptr, *hff_l = nullptr, *xf = nullptr;
  float* hid[2] = {nullptr, nullptr};
  float* partial = nullptr;
  int64_t partial_floats = 0;
  int64_t* tau = nullptr;
};

struct mmk_tr_plan {
  Tuning tune;
  mmk_tr_config cfg;
  Binder binder;
  bool committed = false;
  int D = 0, H = 0, hd = 0, FF = 0, L = 0, rf = 0, Bmax = 0, in_pad = 0;
  TrState s;
  hipStream_t cap_stream = nullptr;
  GraphCache gc;
  ~mmk_tr_plan() {
    gc.reset();
    if (cap_stream) (void)hipStreamDestroy(cap_stream);
  }
};

static void tr_layout(const mmk_tr_plan* p, TrState& s, Carver& cv) {
  const mmk_tr_config& c = p->cfg;
  const int D = p->D, L = p->L, FF = p->FF;
  const int64_t M = (int64_t)p->Bmax * p->rf, B = p->Bmax;
  for (auto& l : s.layers) {
    l.qkv.carve(cv, true); l.o_sa.carve(cv, true); l.q_ca.carve(cv, true); l.o_ca.carve(cv, true);
    l.ff1.carve(cv, true); l.ff2.carve(cv, true);
    for (int k = 0; k < 3; ++k) { l.ln_w[k] = cv.take<float>(D); l.ln_b[k] = cv.take<float>(D); }
  }
  s.kv_ca.carve(cv, true);
  if (c.in_kind == 0) s.embed = cv.take<float>((int64_t)c.in_classes * D);
  else { s.in_lin.carve(cv, true); s.frames = cv.take<float>(M * p->in_pad); }
  s.pe = cv.take<float>((int64_t)p->rf * D);
  if (c.final_norm) { s.fn_w = cv.take<float>(D); s.fn_b = cv.take<float>(D); }
  if (c.head_kind == 0) {
    s.head.carve(cv, B);
    s.hid[0] = cv.take<float>(B * c.mlp_hidden);
    s.hid[1] = cv.take<float>(B * c.mlp_hidden);
  } else {
    s.out_lin.carve(cv, true);
  }
  s.x0 = cv.take<float>(M * D);
  s.x = cv.take<float>(M * D);
  s.qkv = cv.take<float>(M * 3 * D);
  s.att = cv.take<float>(M * D);
  s.tmp = cv.take<float>(M * D);
  s.qc = cv.take<float>(M * D);
  s.hff = cv.take<float>(M * FF);
  s.kvc = cv.take<float>(M * 2 * D * L);
  s.xl = cv.take<float>(B * D);
  s.att_l = cv.take<float>(B * D);
  s.tmp_l = cv.take<float>(B * D);
  s.qc_l = cv.take<float>(B * D);
  s.hff_l = cv.take<float>(B * FF);
  s.xf = cv.take<float>(B * D);
  // split-K partial sums of the GEMM launches that would not fill the chip (gemm.hip): room for the largest split any of them takes
  int64_t part = 0;
  auto need = [&](const PackedLinear& w, int64_t rows) {
    if (rows >= 128) part = std::max<int64_t>(part, gemm_bias_act_partial_floats((int)rows, w.n_tiles, w.k_chunks));
  };
  for (auto& l : s.layers) { need(l.qkv, M); need(l.o_sa, M); need(l.q_ca, M); need(l.o_ca, M); need(l.ff1, M); need(l.ff2, M); }
  need(s.kv_ca, M);
  s.partial_floats = part;
  s.partial = part > 0 ? cv.take<float>(part) : nullptr;
  s.tau = reinterpret_cast<int64_t*>(cv.take<float>(64));
}

static int derive(mmk_tr_plan* p) {
  const mmk_tr_config& c = p->cfg;
  if (c.model_dim < 16 || c.model_dim > 1024 || c.model_dim % 16 != 0)
    return fail(MMK_ERR_INVALID, "tr: model_dim %d (a multiple of 16, 16 .. 1024)", c.model_dim);
  if (c.n_heads < 1 || c.model_dim % c.n_heads != 0)
    return fail(MMK_ERR_INVALID, "tr: n_heads %d does not divide model_dim %d", c.n_heads, c.model_dim);
  const int hd = c.model_dim / c.n_heads;
  if (hd % 4 != 0 || hd > 128)
    return fail(MMK_ERR_INVALID, "tr: head_dim = model_dim / n_heads = %d (a multiple of 4, up to 128)", hd);
  if (c.feedforward_dim < 1 || c.feedforward_dim > 4096)
    return fail(MMK_ERR_INVALID, "tr: feedforward_dim %d (1 .. 4096)", c.feedforward_dim);
  if (c.num_layers < 1 || c.num_layers > 16) return fail(MMK_ERR_INVALID, "tr: num_layers %d (1 .. 16)", c.num_layers);
  if (c.rf < 1 || c.rf > 2048) return fail(MMK_ERR_INVALID, "tr: rf %d (1 .. 2048, the positional encoding's length)", c.rf);
  if (c.max_batch < 1 || c.max_batch > 512) return fail(MMK_ERR_INVALID, "tr: max_batch %d (1 .. 512)", c.max_batch);
  if (c.in_kind == 0) {
    if (c.in_classes < 1) return fail(MMK_ERR_INVALID, "tr: in_classes %d", c.in_classes);
  } else if (c.in_kind == 1) {
    if (c.in_dim < 1) return fail(MMK_ERR_INVALID, "tr: in_dim %d", c.in_dim);
  } else {
    return fail(MMK_ERR_UNSUPPORTED, "tr: in_kind %d is not covered", c.in_kind);
  }
  if (c.head_kind == 0) {
    if (c.out_dim < 1 || c.out_dim > 1024) return fail(MMK_ERR_UNSUPPORTED, "tr: out_dim %d classes (the sampler takes 1 .. 1024)", c.out_dim);
    MMK_TRY(p->s.head.set_geometry("tr", MMK_ERR_UNSUPPORTED, c.model_dim, c.mlp_hidden, c.mlp_n_hidden, c.out_dim, c.learn_temp, c.min_temp, 1));
    if (c.mlp_act < 0 || c.mlp_act > MMK_ACT_COS) return fail(MMK_ERR_INVALID, "tr: mlp_act %d", c.mlp_act);
    if (c.in_kind != 0) return fail(MMK_ERR_UNSUPPORTED, "tr: class indices in and out go together (the loop feeds the outputs back)");
  } else if (c.head_kind == 1) {
    if (c.out_dim < 1) return fail(MMK_ERR_INVALID, "tr: out_dim %d", c.out_dim);
    if (c.in_kind != 1 || c.out_dim != c.in_dim)
      return fail(MMK_ERR_UNSUPPORTED, "tr: frames in and out go together with as many bins (in_dim %d, out_dim %d)", c.in_dim, c.out_dim);
  } else {
    return fail(MMK_ERR_UNSUPPORTED, "tr: head_kind %d is not covered", c.head_kind);
  }
  p->D = c.model_dim; p->H = c.n_heads; p->hd = hd; p->FF = c.feedforward_dim; p->L = c.num_layers; p->rf = c.rf;
  p->Bmax = c.max_batch;
  p->in_pad = c.in_kind == 1 ? (int)round_up(c.in_dim, 16) : 0;
  const int D = p->D;
  p->s.layers.assign(p->L, TrLayer());
  for (auto& l : p->s.layers) {
    l.qkv.set_geometry(3 * D, {D});
    l.o_sa.set_geometry(D, {D});
    l.q_ca.set_geometry(D, {D});
    l.o_ca.set_geometry(D, {D});
    l.ff1.set_geometry(p->FF, {D});
    l.ff2.set_geometry(D, {p->FF});
  }
  p->s.kv_ca.set_geometry(2 * D * p->L, {D});
  if (c.in_kind == 1) p->s.in_lin.set_geometry(D, {c.in_dim});
  if (c.head_kind != 0) p->s.out_lin.set_geometry(c.out_dim, {D});
  return MMK_OK;
}

extern "C" int mmk_tr_plan_create(const mmk_tr_config* cfg, mmk_tr_plan** out) { return plan_create("tr_plan_create", cfg, out, derive); }

extern "C" void mmk_tr_plan_destroy(mmk_tr_plan* p) { delete p; }

extern "C" int mmk_tr_plan_bind(mmk_tr_plan* p, const char* key, const float* dev_ptr, int64_t numel) {
  return plan_bind("tr_plan_bind", p, key, dev_ptr, numel);
}

extern "C" size_t mmk_tr_workspace_bytes(const mmk_tr_plan* p) {
  if (!p) return 0;
  TrState tmp = p->s;
  Carver c(nullptr);
  tr_layout(p, tmp, c);
  return c.used();
}

// rows [row_off, row_off + n_rows) of a bound (rows, K) weight and its bias -> packed rows [row0, row0 + n_rows) of w
static int pack_rows(mmk_tr_plan* p, PackedLinear& w, const std::string& base, const char* wname, const char* bname, int64_t total_rows,
                     int row_off, int n_rows, int row0, hipStream_t st) {
  Binder& b = p->binder;
  const int K = w.segK[0];
  const float* wp = b.need(base + wname, total_rows * K);
  const float* bp = b.need(base + bname, total_rows);
  if (wp) MMK_TRY(pack_rect(w.Wp, w.k_chunks, row0, 1, n_rows, 0, K, wp + (int64_t)row_off * K, K, 1, st));
  if (bp) MMK_TRY(pack_bias(w.bias, row0, 1, n_rows, bp + row_off, 0, st));
  return MMK_OK;
}

static int copy_vec(mmk_tr_plan* p, float* dst, const std::string& key, int64_t n, hipStream_t st) {
  if (const float* src = p->binder.need(key, n)) MMK_HIP(hipMemcpyAsync(dst, src, (size_t)n * sizeof(float), hipMemcpyDeviceToDevice, st));
  return MMK_OK;
}

extern "C" int mmk_tr_commit(mmk_tr_plan* p, void* workspace, size_t workspace_bytes, mmk_stream_t stream) {
  if (!p || !workspace) return fail(MMK_ERR_INVALID, "tr_commit: null argument");
  if ((reinterpret_cast<uintptr_t>(workspace) & 255) != 0) return fail(MMK_ERR_WORKSPACE, "tr_commit: workspace must be 256-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  if (p->gc.exec) {                     // a cached graph holds the previous workspace's addresses and may still be in flight
    MMK_HIP(hipStreamSynchronize(st));
    p->gc.reset();
  }
  const mmk_tr_config& c = p->cfg;
  MMK_TRY(prepare_tr_attention(p->hd));
  Carver carve(workspace);
  tr_layout(p, p->s, carve);
  if (carve.used() > workspace_bytes)
    return fail(MMK_ERR_WORKSPACE, "tr_commit: workspace of %zu bytes, %zu needed", workspace_bytes, carve.used());
  MMK_HIP(hipMemsetAsync(workspace, 0, carve.used(), st));
  Binder& b = p->binder;
  b.clear_missing();
  const int D = p->D, L = p->L;
  for (int l = 0; l < L; ++l) {
    TrLayer& ly = p->s.layers[l];
    const std::string base = "model.layers." + std::to_string(l) + ".";
    MMK_TRY(pack_rows(p, ly.qkv, base + "self_attn.", "in_proj_weight", "in_proj_bias", 3 * D, 0, 3 * D, 0, st));
    MMK_TRY(pack_rows(p, ly.o_sa, base + "self_attn.out_proj.", "weight", "bias", D, 0, D, 0, st));
    // cross-attention: the query rows [0, D) of in_proj here, its key / value rows [D, 3 D) into the all-layer K / V matrix
    MMK_TRY(pack_rows(p, ly.q_ca, base + "multihead_attn.", "in_proj_weight", "in_proj_bias", 3 * D, 0, D, 0, st));
    MMK_TRY(pack_rows(p, p->s.kv_ca, base + "multihead_attn.", "in_proj_weight", "in_proj_bias", 3 * D, D, 2 * D, 2 * D * l, st));
    MMK_TRY(pack_rows(p, ly.o_ca, base + "multihead_attn.out_proj.", "weight", "bias", D, 0, D, 0, st));
    MMK_TRY(pack_rows(p, ly.ff1, base + "linear1.", "weight", "bias", p->FF, 0, p->FF, 0, st));
    MMK_TRY(pack_rows(p, ly.ff2, base + "linear2.", "weight", "bias", D, 0, D, 0, st));
    for (int k = 0; k < 3; ++k) {
      const std::string nb = base + "norm" + std::to_string(k + 1) + ".";
      MMK_TRY(copy_vec(p, ly.ln_w[k], nb + "weight", D, st));
      MMK_TRY(copy_vec(p, ly.ln_b[k], nb + "bias", D, st));
    }
  }
  if (c.final_norm) {
    MMK_TRY(copy_vec(p, p->s.fn_w, "model.norm.weight", D, st));
    MMK_TRY(copy_vec(p, p->s.fn_b, "model.norm.bias", D, st));
  }
  // the checkpoint's positional-encoding buffer as stored, (2048, 1, D): its first rf rows
  if (const float* pe = b.need("pe.pe", (int64_t)2048 * D))
    MMK_HIP(hipMemcpyAsync(p->s.pe, pe, (size_t)p->rf * D * sizeof(float), hipMemcpyDeviceToDevice, st));
  if (c.in_kind == 0) {
    MMK_TRY(copy_vec(p, p->s.embed, "input_module.heads.0.0.weight", (int64_t)c.in_classes * D, st));
  } else {
    MMK_TRY(pack_rows(p, p->s.in_lin, "input_module.heads.0.0.", "weight", "bias", D, 0, D, 0, st));
  }
  if (c.head_kind == 0) {
    MMK_TRY(p->s.head.pack(b, "output_modules.0.estimator.0.fc.", st));
  } else {
    MMK_TRY(pack_rows(p, p->s.out_lin, "output_modules.0.0.", "weight", "bias", c.out_dim, 0, c.out_dim, 0, st));
  }
  if (!b.missing().empty()) return fail(MMK_ERR_KEY, "tr_commit: state_dict tensor %s", b.missing().c_str());
  p->committed = true;
  return MMK_OK;
}

// Y[M, N] = act(X W^T + b): the tiled GEMM where it applies (M >= 128), else the row-tile kernel
static int tr_linear(mmk_tr_plan* p, const PackedLinear& w, const float* x, int64_t ldx, int M, float* y, int64_t ldy, int act,
                     hipStream_t st) {
  if (gemm_bias_act_supported(x, ldx, M, w.segK[0]))
    return launch_gemm_bias_act(x, ldx, w.Wp, w.bias, w.n_tiles, w.k_chunks, w.N, w.segK[0], y, ldy, M, act, st, GemmRowMap(),
                                p->s.partial, p->s.partial_floats);
  LinearArgs a = {};
  w.fill(a);
  a.seg[0].x = addr_static(x);
  a.seg[0].ld = ldx;
  a.M = M;
  a.epilogue = EPI_STORE;
  a.act = act;
  a.out = addr_static(y);
  a.out_ld = ldy;
  return launch_linear(a, st);
}

// one step's input and output: the window of step *tau starts at in + tau in_ts; its result goes to out + tau out_ts
struct TrCall {
  int B = 0;
  const void* in = nullptr;
  int64_t in_bs = 0, in_ts = 0;
  void* out = nullptr;
  int64_t out_bs = 0, out_ts = 0;
  const float* temperature = nullptr;
  const float* uniforms = nullptr;
  int64_t uni_ld = 0;
};

static int attention(mmk_tr_plan* p, const float* q, int64_t q_ld, int64_t q_cs, const float* k, const float* v, int64_t kv_ld,
                     int64_t kv_cs, float* out, int64_t o_ld, int64_t o_cs, int n_q, int q_pos0, int B, hipStream_t st) {
  TrAttnArgs a;
  a.q = q; a.q_ld = q_ld; a.q_cs = q_cs;
  a.k = k; a.v = v; a.kv_ld = kv_ld; a.kv_cs = kv_cs;
  a.out = out; a.o_ld = o_ld; a.o_cs = o_cs;
  a.n_q = n_q; a.q_pos0 = q_pos0; a.n_keys = p->rf; a.n_heads = p->H; a.head_dim = p->hd;
  a.scale = 1.f / sqrtf((float)p->hd);
  return launch_tr_attention(a, B, st);
}

static int emit_step(mmk_tr_plan* p, const TrCall& call, hipStream_t st) {
  const mmk_tr_config& c = p->cfg;
  TrState& s = p->s;
  const int D = p->D, L = p->L, FF = p->FF, rf = p->rf, B = call.B, M = B * rf;
  const int64_t D3 = 3 * (int64_t)D, DL2 = 2 * (int64_t)D * L;
  // X0 = input(window) + pe[0:rf]
  if (c.in_kind == 0) {
    MMK_TRY(launch_tr_embed_pe((const int64_t*)call.in, call.in_bs, call.in_ts, s.tau, s.embed, c.in_classes, s.pe, s.x0, B, rf, D, st));
  } else {
    MMK_TRY(launch_tr_gather_frames((const float*)call.in, call.in_bs, call.in_ts, s.tau, c.in_dim, s.frames, p->in_pad, B, rf, st));
    MMK_TRY(tr_linear(p, s.in_lin, s.frames, p->in_pad, M, s.x0, D, ACT_NONE, st));
    MMK_TRY(launch_tr_add_pe(s.x0, s.pe, B, rf, D, st));
  }
  // the cross-attention keys / values of every layer: memory = X0 for all of them
  MMK_TRY(tr_linear(p, s.kv_ca, s.x0, D, M, s.kvc, DL2, ACT_NONE, st));
  for (int l = 0; l < L; ++l) {
    TrLayer& ly = s.layers[l];
    const float* xin = l == 0 ? s.x0 : s.x;
    const float* kc = s.kvc + 2 * (int64_t)D * l;
    MMK_TRY(tr_linear(p, ly.qkv, xin, D, M, s.qkv, D3, ACT_NONE, st));
    if (l + 1 < L) {
      MMK_TRY(attention(p, s.qkv, D3, rf * D3, s.qkv + D, s.qkv + 2 * D, D3, rf * D3, s.att, D, (int64_t)rf * D, rf, 0, B, st));
      MMK_TRY(tr_linear(p, ly.o_sa, s.att, D, M, s.tmp, D, ACT_NONE, st));
      MMK_TRY(launch_tr_add_ln(s.tmp, D, xin, D, ly.ln_w[0], ly.ln_b[0], s.x, D, M, D, st));
      MMK_TRY(tr_linear(p, ly.q_ca, s.x, D, M, s.qc, D, ACT_NONE, st));
      MMK_TRY(attention(p, s.qc, D, (int64_t)rf * D, kc, kc + D, DL2, rf * DL2, s.att, D, (int64_t)rf * D, rf, 0, B, st));
      MMK_TRY(tr_linear(p, ly.o_ca, s.att, D, M, s.tmp, D, ACT_NONE, st));
      MMK_TRY(launch_tr_add_ln(s.tmp, D, s.x, D, ly.ln_w[1], ly.ln_b[1], s.x, D, M, D, st));
      MMK_TRY(tr_linear(p, ly.ff1, s.x, D, M, s.hff, FF, ACT_RELU, st));
      MMK_TRY(tr_linear(p, ly.ff2, s.hff, FF, M, s.tmp, D, ACT_NONE, st));
      MMK_TRY(launch_tr_add_ln(s.tmp, D, s.x, D, ly.ln_w[2], ly.ln_b[2], s.x, D, M, D, st));
    } else {
      // last layer: keys / values of every row, the rest for the query at window position rf - 1 only (one row per clip)
      const int64_t last = (int64_t)(rf - 1);
      MMK_TRY(attention(p, s.qkv + last * D3, D3, rf * D3, s.qkv + D, s.qkv + 2 * D, D3, rf * D3, s.att_l, D, D, 1, rf - 1, B, st));
      MMK_TRY(tr_linear(p, ly.o_sa, s.att_l, D, B, s.tmp_l, D, ACT_NONE, st));
      MMK_TRY(launch_tr_add_ln(s.tmp_l, D, xin + last * D, (int64_t)rf * D, ly.ln_w[0], ly.ln_b[0], s.xl, D, B, D, st));
      MMK_TRY(tr_linear(p, ly.q_ca, s.xl, D, B, s.qc_l, D, ACT_NONE, st));
      MMK_TRY(attention(p, s.qc_l, D, D, kc, kc + D, DL2, rf * DL2, s.att_l, D, D, 1, rf - 1, B, st));
      MMK_TRY(tr_linear(p, ly.o_ca, s.att_l, D, B, s.tmp_l, D, ACT_NONE, st));
      MMK_TRY(launch_tr_add_ln(s.tmp_l, D, s.xl, D, ly.ln_w[1], ly.ln_b[1], s.xl, D, B, D, st));
      MMK_TRY(tr_linear(p, ly.ff1, s.xl, D, B, s.hff_l, FF, ACT_RELU, st));
      MMK_TRY(tr_linear(p, ly.ff2, s.hff_l, FF, B, s.tmp_l, D, ACT_NONE, st));
      MMK_TRY(launch_tr_add_ln(s.tmp_l, D, s.xl, D, ly.ln_w[2], ly.ln_b[2], s.xl, D, B, D, st));
    }
  }
  const float* hx = s.xl;
  if (c.final_norm) {
    MMK_TRY(launch_tr_add_ln(s.xl, D, nullptr, 0, s.fn_w, s.fn_b, s.xf, D, B, D, st));
    hx = s.xf;
  }
  if (c.head_kind == 0) {
    MMK_TRY(s.head.run(hx, D, s.hid, c.mlp_act, [&](const PackedLinear& w, const float* x, int64_t x_ld, float* o, int64_t o_ld, int act) {
      return tr_linear(p, w, x, x_ld, B, o, o_ld, act, st);
    }));
    SampleArgs sa = {};
    s.head.fill(sa);
    sa.rows = B;
    sa.temperature = call.temperature; sa.uniforms = call.uniforms; sa.uniform_ld = call.uni_ld; sa.uni_off = 0;
    sa.out = (int64_t*)call.out; sa.out_row_stride = call.out_bs; sa.out_tau_off = 0;   // (class tensors: unit stride along time)
    sa.tau_ptr = s.tau; sa.tau_off = 0;
    return launch_sample(sa, st);
  }
  LinearArgs a = {};
  s.out_lin.fill(a);
  a.seg[0].x = addr_static(hx);
  a.seg[0].ld = D;
  a.M = B;
  a.tau_ptr = s.tau;
  a.tau_off = 0;
  a.epilogue = EPI_STORE;
  a.act = c.out_abs ? ACT_ABS : ACT_NONE;
  a.out = addr_time(call.out, call.out_ts, 0, 1, 0);
  a.out_ld = call.out_bs;
  return launch_linear(a, st);
}

static int run_steps(mmk_tr_plan* p, const TrCall& call, int64_t n, hipStream_t st) {
  if (n <= 0) return MMK_OK;
  MMK_TRY(launch_set_i64(p->s.tau, 0, st));
  int64_t done = 0;
  if (n >= 2 * kGraphSteps) {
    const std::vector<int64_t> key = {call.B, (int64_t)(uintptr_t)call.in, call.in_bs, call.in_ts, (int64_t)(uintptr_t)call.out, call.out_bs,
                                      call.out_ts, (int64_t)(uintptr_t)call.temperature, (int64_t)(uintptr_t)call.uniforms, call.uni_ld};
    if (!p->gc.exec || p->gc.key != key) {
      MMK_HIP(hipStreamSynchronize(st));   // a cached graph may still be in flight
      p->gc.reset();
      if (!p->cap_stream) MMK_HIP(hipStreamCreateWithFlags(&p->cap_stream, hipStreamNonBlocking));
      MMK_HIP(hipStreamBeginCapture(p->cap_stream, hipStreamCaptureModeThreadLocal));
      int rc = MMK_OK;
      for (int k = 0; k < kGraphSteps && rc == MMK_OK; ++k) {
        rc = emit_step(p, call, p->cap_stream);
        if (rc == MMK_OK) rc = launch_bump(p->s.tau, 1, p->cap_stream);
      }
      hipGraph_t g = nullptr;
      const hipError_t e = hipStreamEndCapture(p->cap_stream, &g);
      if (rc != MMK_OK) {
        if (g) (void)hipGraphDestroy(g);
        return rc;
      }
      if (e != hipSuccess) return fail(MMK_ERR_HIP, "hipStreamEndCapture failed: %s", hipGetErrorString(e));
      p->gc.graph = g;
      MMK_HIP(hipGraphInstantiate(&p->gc.exec, g, nullptr, nullptr, 0));
      p->gc.key = key;
      p->gc.steps = kGraphSteps;
    }
    const int64_t reps = n / kGraphSteps;
    for (int64_t r = 0; r < reps; ++r) MMK_HIP(hipGraphLaunch(p->gc.exec, st));
    done = reps * kGraphSteps;
  }
  for (int64_t k = done; k < n; ++k) {
    MMK_TRY(emit_step(p, call, st));
    MMK_TRY(launch_bump(p->s.tau, 1, st));
  }
  return MMK_OK;
}

static int check_call(mmk_tr_plan* p, int32_t batch, const void* a, const void* b, const float* temperature, const float* uniforms,
                      const char* what) {
  if (!p || !a || !b) return fail(MMK_ERR_INVALID, "%s: null argument", what);
  if (!p->committed) return fail(MMK_ERR_STATE, "%s: plan not committed (bind the state_dict, then mmk_tr_commit)", what);
  if (batch < 1 || batch > p->Bmax) return fail(MMK_ERR_INVALID, "%s: batch %d outside [1, %d]", what, batch, p->Bmax);
  if (temperature && p->cfg.head_kind != 0) return fail(MMK_ERR_INVALID, "%s: a temperature needs the MLP head", what);
  if (temperature && !uniforms) return fail(MMK_ERR_INVALID, "%s: temperature given without uniforms", what);
  return MMK_OK;
}

extern "C" int mmk_tr_step(mmk_tr_plan* p, int32_t batch, const void* x, int64_t x_batch_stride, int64_t x_time_stride, void* y,
                           int64_t y_batch_stride, const float* temperature, const float* uniforms, mmk_stream_t stream) {
  MMK_TRY(check_call(p, batch, x, y, temperature, uniforms, "tr_step"));
  TrCall call;
  call.B = batch;
  call.in = x; call.in_bs = x_batch_stride; call.in_ts = x_time_stride;
  call.out = y; call.out_bs = y_batch_stride; call.out_ts = 0;
  call.temperature = temperature; call.uniforms = uniforms; call.uni_ld = 1;
  return run_steps(p, call, 1, (hipStream_t)stream);
}

extern "C" int mmk_tr_generate(mmk_tr_plan* p, int32_t batch, void* data, int64_t batch_stride, int64_t time_stride, int64_t t0,
                               int64_t n_steps, const float* temperature, const float* uniforms, mmk_stream_t stream) {
  MMK_TRY(check_call(p, batch, data, data, temperature, uniforms, "tr_generate"));
  if (t0 < p->rf) return fail(MMK_ERR_INVALID, "tr_generate: t0=%lld is shorter than rf=%d", (long long)t0, p->rf);
  if (n_steps < 0) return fail(MMK_ERR_INVALID, "tr_generate: n_steps %lld", (long long)n_steps);
  if (p->cfg.head_kind == 0 && time_stride != 1) return fail(MMK_ERR_INVALID, "tr_generate: class tensors need time_stride 1");
  const size_t esz = p->cfg.in_kind == 0 ? sizeof(int64_t) : sizeof(float);
  TrCall call;
  call.B = batch;
  call.in = (const char*)data + (t0 - p->rf) * time_stride * (int64_t)esz;
  call.in_bs = batch_stride; call.in_ts = time_stride;
  call.out = (char*)data + t0 * time_stride * (int64_t)esz;
  call.out_bs = batch_stride; call.out_ts = time_stride;
  call.temperature = temperature; call.uniforms = uniforms; call.uni_ld = n_steps;
  return run_steps(p, call, n_steps, (hipStream_t)stream);
}

extern "C" int mmk_tr_last_logits(mmk_tr_plan* p, int32_t batch, float* out, int64_t out_ld, mmk_stream_t stream) {
  if (!p || !out) return fail(MMK_ERR_INVALID, "tr_last_logits: null argument");
  if (!p->committed || p->cfg.head_kind != 0) return fail(MMK_ERR_STATE, "tr_last_logits: only for a committed plan with the MLP head");
  if (batch < 1 || batch > p->Bmax) return fail(MMK_ERR_INVALID, "tr_last_logits: batch %d outside [1, %d]", batch, p->Bmax);
  if (out_ld < p->s.head.n_out()) return fail(MMK_ERR_INVALID, "tr_last_logits: out_ld %lld < %d", (long long)out_ld, p->s.head.n_out());
  return p->s.head.copy_logits(out, out_ld, batch, (hipStream_t)stream);
}
