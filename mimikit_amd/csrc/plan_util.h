// Host-side helpers shared by the network plans: state_dict binding, workspace
// carving, packed-linear descriptors, the MLP head, the entry points the plans
// have in common and the hipGraph step cache.
#pragma once
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include <vector>

#include "mmk_common.h"

namespace mmk {

// The execution switches of ONE plan: the `tuning` text of its config ("MMK_WN_CHAIN=0;MMK_WN_PIPE=1"), parsed when the plan is created.
// Nothing comes from the environment in the product library - a stray variable, or another thread's setenv between two plan creations,
// must not change which kernel a plan gets.  The diagnostic build (-DMMK_DIAG: stamps and timing experiments) falls back to the
// environment for names the text does not set; `diag_only` is the same fall-back for switches that exist in that build only.
inline const char* diag_only(const char* name) {
#ifdef MMK_DIAG
  return getenv(name);
#else
  (void)name;
  return nullptr;
#endif
}
class Tuning {
 public:
  void parse(const char* text, size_t cap) {
    kv_.clear();
    std::string s(text, strnlen(text, cap));
    size_t at = 0;
    while (at < s.size()) {
      size_t end = s.find(';', at);
      if (end == std::string::npos) end = s.size();
      const std::string item = s.substr(at, end - at);
      const size_t eq = item.find('=');
      if (eq != std::string::npos && eq > 0) kv_[item.substr(0, eq)] = item.substr(eq + 1);
      at = end + 1;
    }
  }
  // the value's text, or nullptr when the switch is not set (the pointer lives as long as the plan)
  const char* get(const char* name) const {
    auto it = kv_.find(name);
    if (it != kv_.end()) return it->second.c_str();
    return diag_only(name);
  }

 private:
  std::map<std::string, std::string> kv_;
};

struct Bound {
  const float* ptr = nullptr;
  int64_t numel = 0;
};

class Binder {
 public:
  void bind(const std::string& key, const float* p, int64_t n) { map_[key] = Bound{p, n}; }
  // returns nullptr (and records the key) when missing or mis-sized
  const float* need(const std::string& key, int64_t numel) {
    auto it = map_.find(key);
    if (it == map_.end()) {
      if (missing_.empty()) missing_ = key + " (not bound)";
      return nullptr;
    }
    if (it->second.numel != numel) {
      if (missing_.empty())
        missing_ = key + " (expected " + std::to_string(numel) + " elements, got " + std::to_string(it->second.numel) + ")";
      return nullptr;
    }
    return it->second.ptr;
  }
  bool has(const std::string& key) const { return map_.count(key) != 0; }
  const std::string& missing() const { return missing_; }
  void clear_missing() { missing_.clear(); }

 private:
  std::map<std::string, Bound> map_;
  std::string missing_;
};

// Bump allocator over the caller's workspace; first pass (base == nullptr) sizes it.
class Carver {
 public:
  explicit Carver(void* base = nullptr) : base_((char*)base) {}
  template <typename T>
  T* take(int64_t count) {
    off_ = (size_t)round_up((int64_t)off_, 256);
    T* p = base_ ? reinterpret_cast<T*>(base_ + off_) : nullptr;
    off_ += (size_t)count * sizeof(T);
    return p;
  }
  size_t used() const { return (size_t)round_up((int64_t)off_, 256); }

 private:
  char* base_;
  size_t off_ = 0;
};

// A weight matrix in MFMA fragment order plus its K-segment geometry.
struct PackedLinear {
  float* Wp = nullptr;
  float* bias = nullptr;  // packed order, n_tiles*16 entries (zero padded) or nullptr
  int N = 0;              // packed rows in use
  int n_tiles = 0;
  int nseg = 0;
  int segK[kMaxSeg] = {0, 0, 0, 0};
  int seg_chunk0[kMaxSeg + 1] = {0, 0, 0, 0, 0};
  int k_chunks = 0;

  void set_geometry(int n_rows_packed, const std::vector<int>& ks) {
    N = n_rows_packed;
    n_tiles = (n_rows_packed + 15) / 16;
    nseg = (int)ks.size();
    k_chunks = 0;
    for (int s = 0; s < nseg; ++s) {
      segK[s] = ks[s];
      seg_chunk0[s] = k_chunks;
      k_chunks += (ks[s] + 15) / 16;
    }
    for (int s = nseg; s <= kMaxSeg; ++s) seg_chunk0[s] = k_chunks;
  }
  int64_t weight_floats() const { return (int64_t)n_tiles * 16 * k_chunks * 16; }
  int64_t bias_floats() const { return (int64_t)n_tiles * 16; }
  void carve(Carver& c, bool with_bias) {
    Wp = c.take<float>(weight_floats());
    bias = with_bias ? c.take<float>(bias_floats()) : nullptr;
  }
  int clear(hipStream_t st) const {
    MMK_HIP(hipMemsetAsync(Wp, 0, weight_floats() * sizeof(float), st));
    if (bias) MMK_HIP(hipMemsetAsync(bias, 0, bias_floats() * sizeof(float), st));
    return MMK_OK;
  }
  // fill the common LinearArgs fields; the caller sets seg[].x/ld/kind and the epilogue
  void fill(LinearArgs& a) const {
    a.nseg = nseg;
    for (int s = 0; s < nseg; ++s) {
      a.seg[s].K = segK[s];
      a.seg[s].kind = SEG_F32;
      a.seg[s].class_size = 1.f;
    }
    for (int s = 0; s <= kMaxSeg; ++s) a.seg_chunk0[s] = seg_chunk0[s];
    a.k_chunks = k_chunks;
    a.N = N;
    a.n_tiles = n_tiles;
    a.Wp = Wp;
    a.bias = bias;
  }
};

// One output module as every network ends in it (networks/mlp.py:42-53, modules/io.py:205): Linear, act, [Linear, act] * n_hidden, Linear
// with an optional learned-temperature column, then the categorical sampler.  The two hidden-row buffers its layers ping-pong through belong
// to the plan: a plan's heads share them.
struct MlpHead {
  std::vector<PackedLinear> layers;
  int in_dim = 0, hidden = 0, n_classes = 0, learn_temp = 0;
  float min_temp = 0.f;
  float* logits = nullptr;      // (rows, logits_ld): the last Linear's outputs, before the temperature division
  int logits_ld = 0;

  int n_out() const { return n_classes + (learn_temp ? 1 : 0); }

  // `who` names the head in the message, `bad` is the code a refused geometry returns; logits_ld = n_out() rounded up to `ld_align`
  int set_geometry(const char* who, int bad, int in_dim_, int hidden_, int n_hidden, int n_classes_, int learn_temp_, float min_temp_, int ld_align) {
    if (hidden_ < 1 || n_hidden < 0 || n_hidden > MMK_MAX_MLP_HIDDEN)
      return fail(bad, "%s: bad MLP head geometry (hidden %d, %d extra blocks)", who, hidden_, n_hidden);
    in_dim = in_dim_; hidden = hidden_; n_classes = n_classes_; learn_temp = learn_temp_; min_temp = min_temp_;
    layers.assign((size_t)n_hidden + 2, PackedLinear());
    layers.front().set_geometry(hidden, {in_dim});
    for (int i = 1; i <= n_hidden; ++i) layers[i].set_geometry(hidden, {hidden});
    layers.back().set_geometry(n_out(), {hidden});
    logits_ld = (int)round_up(n_out(), ld_align);
    return MMK_OK;
  }
  void carve(Carver& c, int64_t rows) {
    for (auto& m : layers) m.carve(c, true);
    logits = c.take<float>(rows * logits_ld);
  }
  // binds <prefix>{0, 2, 4, ..}.weight / .bias; a missing or mis-sized tensor is recorded in the binder
  int pack(Binder& b, const std::string& prefix, hipStream_t st) {
    for (size_t i = 0; i < layers.size(); ++i) {
      PackedLinear& m = layers[i];
      const std::string kb = prefix + std::to_string(2 * i) + ".";
      const float* w = b.need(kb + "weight", (int64_t)m.N * m.segK[0]);
      const float* bb = b.need(kb + "bias", m.N);
      if (w) MMK_TRY(pack_rect(m.Wp, m.k_chunks, 0, 1, m.N, 0, m.segK[0], w, m.segK[0], 1, st));
      if (bb) MMK_TRY(pack_bias(m.bias, 0, 1, m.N, bb, 0, st));
    }
    return MMK_OK;
  }
  // x -> logits through the plan's hid[0] / hid[1]; `linear(w, x, x_ld, out, out_ld, act)` launches one layer the plan's way
  template <typename Linear>
  int run(const float* x, int64_t x_ld, float* const* hid, int act, Linear&& linear) const {
    for (size_t i = 0; i < layers.size(); ++i) {
      const bool last = i + 1 == layers.size();
      float* o = last ? logits : hid[i & 1];
      const int64_t o_ld = last ? logits_ld : hidden;
      MMK_TRY(linear(layers[i], x, x_ld, o, o_ld, last ? (int)ACT_NONE : act));
      x = o;
      x_ld = o_ld;
    }
    return MMK_OK;
  }
  // the sampler's view of the head; rows, temperature, uniforms, destination and tau are the plan's
  void fill(SampleArgs& s) const {
    s.logits = logits; s.ld = logits_ld; s.n_classes = n_classes; s.has_temp_col = learn_temp; s.min_temp = min_temp;
  }
  // the n_out() columns of the last step's rows -> out (device memory)
  int copy_logits(float* out, int64_t out_ld, int64_t rows, hipStream_t st) const {
    // (a kernel of ours, not the runtime's 2D copy: the caller's rows may lie any 64-bit leading dimension apart; `rows` is the plan's
    //  max_batch x hop at the most - every caller has checked batch <= Bmax - and becomes the grid's x dimension)
    return launch_copy_rows(addr_static(logits), logits_ld, addr_static(out), out_ld, (int)rows, n_out(), nullptr, 0, st);
  }
};

// ---- the entry points every plan type has in the same words (Plan: cfg, tune, binder, committed, layout(Carver&)) ----------------------
template <typename Plan, typename Config>
int plan_create(const char* who, const Config* cfg, Plan** out, int (*derive)(Plan*)) {
  if (!cfg || !out) return fail(MMK_ERR_INVALID, "%s: null argument", who);
  Plan* p = new Plan();
  p->cfg = *cfg;
  p->tune.parse(cfg->tuning, sizeof(cfg->tuning));
  const int rc = derive(p);
  if (rc != MMK_OK) {
    delete p;
    return rc;
  }
  *out = p;
  return MMK_OK;
}

template <typename Plan>
int plan_bind(const char* who, Plan* p, const char* key, const float* dev_ptr, int64_t numel) {
  if (!p || !key || !dev_ptr) return fail(MMK_ERR_INVALID, "%s: null argument", who);
  p->binder.bind(key, dev_ptr, numel);
  p->committed = false;
  return MMK_OK;
}

// layout() only writes pointers: the sizing pass runs it on a copy
template <typename Plan>
size_t plan_workspace_bytes(const Plan* p) {
  if (!p) return 0;
  Plan tmp = *p;
  Carver c(nullptr);
  tmp.layout(c);
  return c.used();
}

// a commit's first half: the argument checks, then the plan laid out over the caller's workspace; *used: the bytes it takes
template <typename Plan>
int plan_place(const char* who, Plan* p, void* workspace, size_t workspace_bytes, size_t* used) {
  if (!p || !workspace) return fail(MMK_ERR_INVALID, "%s: null argument", who);
  if ((reinterpret_cast<uintptr_t>(workspace) & 255) != 0) return fail(MMK_ERR_WORKSPACE, "%s: workspace must be 256-byte aligned", who);
  Carver carve(workspace);
  p->layout(carve);
  *used = carve.used();
  if (*used > workspace_bytes) return fail(MMK_ERR_WORKSPACE, "%s: workspace of %zu bytes, %zu needed", who, workspace_bytes, *used);
  return MMK_OK;
}

// Cache of one instantiated hipGraph holding `steps` consecutive steps.
struct GraphCache {
  hipGraphExec_t exec = nullptr;
  hipGraph_t graph = nullptr;
  std::vector<int64_t> key;
  int steps = 0;
  void reset() {
    if (exec) (void)hipGraphExecDestroy(exec);
    if (graph) (void)hipGraphDestroy(graph);
    exec = nullptr;
    graph = nullptr;
    key.clear();
    steps = 0;
  }
};

}  // namespace mmk
