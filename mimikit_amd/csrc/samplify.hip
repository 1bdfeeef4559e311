// Samplifyer on the device (reference mimikit/extract/samplify.py): the quadratic interpolating spline of scipy's interp1d (coefficients
// and evaluation), the attack / peak search of attack_decay and the scoring, side test, refinement and zero-crossing snap of
// Samplifyer.fit - all from the per-frame spline coefficients (spline2.h); no T-long envelope or gradient is written by anything here
// but the evaluation kernel, which exists for the callers that want one.
#include "entry_util.h"
#include "spline2.h"
#include "../../include/mmk_samplify.h"

namespace mmk {

constexpr int kSpTile = MMK_SPLINE2_TILE;
constexpr int kSpHalo = MMK_SPLINE2_HALO;
constexpr int kPerTile = MMK_PERIODS_TILE;
constexpr int kGroup = MMK_SAMPLIFY_GROUP;
constexpr int kMaxLevels = MMK_SAMPLIFY_MAX_LEVELS;

// ---- coefficients ---------------------------------------------------------------------------------------------------------------------
// A workgroup owns kSpTile consecutive knots of one row and stages y and the collocation rows (sub, diag, super; made by spline2_basis at
// x = j from the knot vector) of its knots and kSpHalo more on either side in LDS.  Lane i then solves the tridiagonal system of the rows
// i - kSpHalo .. i + kSpHalo (cut at the row's ends) for c[i] alone: the Thomas recurrence from the window's left end up to row i - 1, the
// mirrored one from its right end down to row i + 1, and row i with both neighbours substituted.  Every lane's order of operations
// depends on i and n alone - not on the tile, the batch or the stride.
__global__ __launch_bounds__(kSpTile) void spline2_coef_kernel(const float* __restrict__ y, int64_t y_row_stride, int64_t n, int64_t n_tiles,
                                                              double* __restrict__ coef, int64_t coef_row_stride) {
  constexpr int W = kSpTile + 2 * kSpHalo;
  __shared__ double s_y[W], s_a[W], s_b[W], s_c[W];
  const int64_t row = blockIdx.x / n_tiles, tile = blockIdx.x - row * n_tiles;
  const float* yr = y + row * y_row_stride;
  const int64_t first = tile * kSpTile - kSpHalo;           // the knot of LDS slot 0
  for (int k = threadIdx.x; k < W; k += kSpTile) {
    const int64_t j = first + k;
    if (j < 0 || j >= n) continue;                          // (never read: a window is cut at the row's ends)
    const int64_t l = spline2_interval((double)j, n);
    double h[3];
    spline2_basis((double)j, l, n, h);
    const int64_t o = j - (l - 2);                          // h[o] is column j: 1 everywhere but in rows 0 (o = 0) and n - 1 (o = 2)
    s_a[k] = o >= 1 ? h[o - 1] : 0.0;
    s_b[k] = h[o];
    s_c[k] = o <= 1 ? h[o + 1] : 0.0;
    s_y[k] = (double)yr[j];
  }
  __syncthreads();
  const int64_t i = tile * kSpTile + threadIdx.x;
  if (i >= n) return;
  const int ki = threadIdx.x + kSpHalo;
  const int k0 = i - kSpHalo < 0 ? (int)(ki - i) : ki - kSpHalo;                    // slot of max(i - halo, 0)
  const int k1 = i + kSpHalo > n - 1 ? (int)(ki + (n - 1 - i)) : ki + kSpHalo;     // slot of min(i + halo, n - 1)
  double diag = s_b[ki], rhs = s_y[ki];
  if (k0 < ki) {
    double beta = s_b[k0], delta = s_y[k0];
    for (int k = k0 + 1; k < ki; ++k) {
      const double w = s_a[k] / beta;
      beta = s_b[k] - w * s_c[k - 1];
      delta = s_y[k] - w * delta;
    }
    const double w = s_a[ki] / beta;
    diag -= w * s_c[ki - 1];
    rhs -= w * delta;
  }
  if (k1 > ki) {
    double gamma = s_b[k1], eps = s_y[k1];
    for (int k = k1 - 1; k > ki; --k) {
      const double w = s_c[k] / gamma;
      gamma = s_b[k] - w * s_a[k + 1];
      eps = s_y[k] - w * eps;
    }
    const double w = s_c[ki] / gamma;
    diag -= w * s_a[ki + 1];
    rhs -= w * eps;
  }
  coef[row * coef_row_stride + i] = rhs / diag;
}

// ---- evaluation -----------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(MMK_SPLINE2_EVAL_TILE) void spline2_eval_kernel(const double* __restrict__ coef, int64_t coef_row_stride, int64_t n,
                                                                            float* __restrict__ out, int64_t out_row_stride, int64_t n_out,
                                                                            double step) {
  const double* c = coef + (int64_t)blockIdx.y * coef_row_stride;
  float* o = out + (int64_t)blockIdx.y * out_row_stride;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_out; i += (int64_t)gridDim.x * blockDim.x)
    o[i] = spline2_eval(c, n, i, n_out, step);
}

// ---- workgroup helpers ------------------------------------------------------------------------------------------------------------------
// inclusive scan of one int per lane over a workgroup of 256 (four waves); s_w: 4 ints of LDS; every lane must call
__device__ __forceinline__ int block_scan_incl(int v, int* s_w) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const int u = __shfl_up(v, d, 64);
    if (lane >= d) v += u;
  }
  __syncthreads();                                          // (s_w may still be read from a previous call)
  if (lane == 63) s_w[wave] = v;
  __syncthreads();
  int before = 0;
  for (int w = 0; w < wave; ++w) before += s_w[w];
  return v + before;
}

// ---- attacks and peaks -------------------------------------------------------------------------------------------------------------------
// A workgroup owns kPerTile consecutive samples: it evaluates g there and one sample to either side into LDS (0 outside the signal, which
// is neither an attack nor a peak), every lane flags its four consecutive samples, and a scan of the lanes' counts orders them.
// RAW 1: g is a float32 row of T samples given as it is (attack_decay on a curve of the caller's), RAW 0: the spline.
// FILL 0: the tile's two counts -> tile_off[2 b], tile_off[2 b + 1].  FILL 1: the indices, from the tile's offsets, into att / peaks.
template <int FILL, int RAW>
__global__ __launch_bounds__(256) void periods_kernel(const double* __restrict__ coef, int64_t n, const float* __restrict__ row, int64_t T, double step,
                                                     int64_t* __restrict__ tile_off,
                                                     int64_t n_att, int64_t n_peak, int64_t* __restrict__ att, int64_t* __restrict__ peaks) {
  __shared__ float s_g[kPerTile + 2];
  __shared__ int s_w[4];
  const int64_t t0 = (int64_t)blockIdx.x * kPerTile;
  for (int k = threadIdx.x; k < kPerTile + 2; k += 256) {
    const int64_t i = t0 - 1 + k;
    s_g[k] = (i >= 0 && i < T) ? (RAW ? row[i] : spline2_eval(coef, n, i, T, step)) : 0.f;
  }
  __syncthreads();
  int na = 0, np = 0;
  unsigned fa = 0, fp = 0;
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const int o = threadIdx.x * 4 + u;
    const float gm = s_g[o], g0 = s_g[o + 1], gp = s_g[o + 2];
    if (gm < 0.f && g0 > 0.f) { fa |= 1u << u; ++na; }
    if (g0 > 0.f && gp < 0.f) { fp |= 1u << u; ++np; }
  }
  const int incl = block_scan_incl(na | (np << 16), s_w);   // (at most kPerTile = 1024 of either: the halves do not carry)
  if (FILL == 0) {
    if (threadIdx.x == 255) {
      tile_off[2 * (int64_t)blockIdx.x] = incl & 0xffff;
      tile_off[2 * (int64_t)blockIdx.x + 1] = incl >> 16;
    }
  } else {
    int64_t pa = tile_off[2 * (int64_t)blockIdx.x] + ((incl & 0xffff) - na);
    int64_t pp = tile_off[2 * (int64_t)blockIdx.x + 1] + ((incl >> 16) - np);
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int64_t i = t0 + threadIdx.x * 4 + u;
      if (fa & (1u << u)) { if (pa >= 0 && pa < n_att) att[pa] = i; ++pa; }
      if (fp & (1u << u)) { if (pp >= 0 && pp < n_peak) peaks[pp] = i; ++pp; }
    }
  }
}

// the tiles' counts -> their exclusive offsets, in place, and the totals: one workgroup, 256 tiles per step with a carry
__global__ __launch_bounds__(256) void periods_scan_kernel(int64_t* __restrict__ tile_off, int64_t n_tiles, int64_t* __restrict__ counts) {
  __shared__ int s_w[4];
  int64_t carry_a = 0, carry_p = 0;
  for (int64_t base = 0; base < n_tiles; base += 256) {
    const int64_t b = base + threadIdx.x;
    const int ca = b < n_tiles ? (int)tile_off[2 * b] : 0, cp = b < n_tiles ? (int)tile_off[2 * b + 1] : 0;
    const int ia = block_scan_incl(ca, s_w);                // (256 tiles of at most 512 attacks: an int holds it)
    const int ip = block_scan_incl(cp, s_w);
    if (b < n_tiles) {
      tile_off[2 * b] = carry_a + (ia - ca);
      tile_off[2 * b + 1] = carry_p + (ip - cp);
    }
    __shared__ int s_tot[2];
    __syncthreads();
    if (threadIdx.x == 255) { s_tot[0] = ia; s_tot[1] = ip; }
    __syncthreads();
    carry_a += s_tot[0];
    carry_p += s_tot[1];
  }
  if (threadIdx.x == 0) { counts[0] = carry_a; counts[1] = carry_p; }
}

// dec of every attack: the first peak at or after it, by bisection of the rising list
__global__ __launch_bounds__(256) void periods_dec_kernel(const int64_t* __restrict__ att, int64_t n_att, const int64_t* __restrict__ peaks, int64_t n_peak,
                                                         int64_t T, int64_t* __restrict__ dec) {
  const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (k >= n_att) return;
  const int64_t a = att[k], b = k + 1 < n_att ? att[k + 1] : T - 1;
  int64_t lo = 0, hi = n_peak;                               // the first index with peaks[index] >= a
  while (lo < hi) {
    const int64_t mid = lo + (hi - lo) / 2;
    if (peaks[mid] < a) lo = mid + 1; else hi = mid;
  }
  int64_t d = T - 1;
  if (lo < n_peak) {
    const int64_t p = peaks[lo];
    if (p <= b - 2) d = p;
  }
  dec[k] = d;
}

// ---- scores -----------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void samplify_scores_kernel(const double* __restrict__ coef, int64_t n, int64_t T, double step, const int64_t* __restrict__ att,
                                                             const int64_t* __restrict__ dec, int64_t count, float sensitivity, float* __restrict__ scores,
                                                             float* __restrict__ env_att, float* __restrict__ env_dec, uint8_t* __restrict__ keep) {
  const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (k >= count) return;
  const int64_t a = att[k], d = dec[k];
  const bool ok = a >= 0 && a < T && d >= 0 && d < T;
  const float ea = ok ? spline2_eval(coef, n, a, T, step) : __builtin_nanf("");
  const float ed = ok ? spline2_eval(coef, n, d, T, step) : __builtin_nanf("");
  const float s = __fsub_rn(ed, ea);
  scores[k] = s;
  env_att[k] = ea;
  env_dec[k] = ed;
  keep[k] = (ok && s > sensitivity) ? 1 : 0;
}

// ---- side, refine, snap -------------------------------------------------------------------------------------------------------------------
struct SamplifyLevels {
  const double* e[kMaxLevels];
  const double* g[kMaxLevels];
  int64_t n[kMaxLevels];
  double step[kMaxLevels];
  int32_t levels;
};

__device__ __forceinline__ float block_max(float v, float* s_f) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) v = fmaxf(v, __shfl_xor(v, d, 64));
  __syncthreads();
  if ((threadIdx.x & 63) == 0) s_f[threadIdx.x >> 6] = v;
  __syncthreads();
  return fmaxf(fmaxf(s_f[0], s_f[1]), fmaxf(s_f[2], s_f[3]));
}

// the pair with the smaller value, the lower index among equal values (MIN), or the larger value likewise (MAX = -1: compare negated order)
template <typename V, int SIGN>
__device__ __forceinline__ void pick(V& v, int64_t& i, V ov, int64_t oi) {
  const bool better = SIGN > 0 ? (ov < v) : (ov > v);
  if (better || (ov == v && oi < i)) { v = ov; i = oi; }
}

template <typename V, int SIGN>
__device__ __forceinline__ int64_t block_arg(V v, int64_t i, V* s_v, int64_t* s_i) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    const V ov = __shfl_xor(v, d, 64);
    const int64_t oi = __shfl_xor((long long)i, d, 64);
    pick<V, SIGN>(v, i, ov, oi);
  }
  __syncthreads();
  if ((threadIdx.x & 63) == 0) { s_v[threadIdx.x >> 6] = v; s_i[threadIdx.x >> 6] = i; }
  __syncthreads();
  v = s_v[0]; i = s_i[0];
#pragma unroll
  for (int w = 1; w < 4; ++w) pick<V, SIGN>(v, i, s_v[w], s_i[w]);
  return i;
}

__device__ __forceinline__ bool crossing(const float* __restrict__ y, int64_t i) {
  return i == 0 || ((__float_as_uint(y[i]) ^ __float_as_uint(y[i - 1])) >> 31) != 0;
}

__global__ __launch_bounds__(kGroup) void samplify_cuts_kernel(const float* __restrict__ y, int64_t T, SamplifyLevels lv, const int64_t* __restrict__ coarse_cuts,
                                                              const int64_t* __restrict__ coarse_peaks, int64_t* __restrict__ sides,
                                                              float* __restrict__ lr_scores, int64_t* __restrict__ cuts) {
  __shared__ float s_f[4];
  __shared__ double s_d[4];
  __shared__ int64_t s_i[4];
  __shared__ int64_t s_hit[4], s_at[4];
  const int64_t k = blockIdx.x;
  const int64_t c0 = coarse_cuts[k], d0 = coarse_peaks[k];
  if (!(c0 >= 0 && c0 <= d0 && d0 <= T - 1)) {              // (the same for every lane)
    if (threadIdx.x == 0) {
      sides[k] = -1;
      cuts[k] = -1;
      if (lr_scores) lr_scores[2 * k] = lr_scores[2 * k + 1] = __builtin_nanf("");
    }
    return;
  }
  // side
  const int last = lv.levels - 1;
  const int64_t w = d0 - c0 < MMK_SAMPLIFY_MAX_WINDOW ? d0 - c0 : MMK_SAMPLIFY_MAX_WINDOW;
  const int64_t l0 = c0 - w < 0 ? 0 : c0 - w, r1 = c0 + w > T ? T : c0 + w;
  float left = -__builtin_inff(), right = -__builtin_inff();
  for (int64_t i = l0 + threadIdx.x; i < r1; i += kGroup) {
    const float v = __fsub_rn(spline2_eval(lv.e[0], lv.n[0], i, T, lv.step[0]), spline2_eval(lv.e[last], lv.n[last], i, T, lv.step[last]));
    if (i < c0) left = fmaxf(left, v); else right = fmaxf(right, v);
  }
  left = block_max(left, s_f);
  right = block_max(right, s_f);
  const int side = left >= right ? 0 : 1;
  // refine
  int64_t c = c0, d = side == 0 ? c0 : d0;
  for (int l = 1; l < lv.levels; ++l) {
    if (c == d) break;                                       // (c and d are the same in every lane)
    double best = __builtin_inf();
    float top = -__builtin_inff();
    int64_t bi = INT64_MAX, ti = INT64_MAX;
    for (int64_t i = c + threadIdx.x; i < d; i += kGroup) {
      const float e = spline2_eval(lv.e[l], lv.n[l], i, T, lv.step[l]), g = spline2_eval(lv.g[l], lv.n[l], i, T, lv.step[l]);
      const double obj = __dadd_rn(__dmul_rn(0.9, (double)e), __dmul_rn(0.1, __dsub_rn(1.0, (double)g)));
      if (obj < best || bi == INT64_MAX) { best = obj; bi = i; }
      if (e > top || ti == INT64_MAX) { top = e; ti = i; }
    }
    int64_t s = block_arg<double, 1>(best, bi, s_d, s_i) - c;
    const int64_t m = block_arg<float, -1>(top, ti, s_f, s_i) - c;
    s = s < d - 1 ? s : 0;
    const int64_t cs = c + s, cm = c + m;
    c = cs;
    d = cm > cs ? cm : cs;
  }
  // snap
  int64_t cut = c;
  for (int64_t base = 0;; base += kGroup) {
    const int64_t r = base + threadIdx.x, before = c - r, after = c + 1 + r;
    const bool hb = before >= 0 && crossing(y, before), ha = after < T && crossing(y, after);
    const unsigned long long mask = __ballot(hb || ha);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    __syncthreads();
    if (mask == 0) {
      if (lane == 0) s_hit[wave] = 0;
    } else if (lane == __ffsll((long long)mask) - 1) {
      s_hit[wave] = 1;
      s_at[wave] = hb ? before : after;
    }
    __syncthreads();
    bool found = false;
#pragma unroll
    for (int wv = 0; wv < 4; ++wv)
      if (!found && s_hit[wv]) { found = true; cut = s_at[wv]; }
    if (found || base + kGroup > c) break;                   // (before = 0 is a crossing: the walk ends within c steps)
  }
  if (threadIdx.x == 0) {
    sides[k] = side;
    cuts[k] = cut;
    if (lr_scores) { lr_scores[2 * k] = left; lr_scores[2 * k + 1] = right; }
  }
}

// ---- argument checks ------------------------------------------------------------------------------------------------------------------------
static int spline_ok(const char* what, const void* coef, int64_t n) {
  if (!coef || misaligned(coef, 8)) return fail(MMK_ERR_INVALID, "%s: the coefficients must be a float64 device pointer, 8-byte aligned", what);
  if (n < 3) return fail(MMK_ERR_INVALID, "%s: a quadratic spline needs n >= 3 knots, got %lld", what, (long long)n);
  return MMK_OK;
}

static double linspace_step(int64_t n, int64_t n_out) { return n_out > 1 ? (double)(n - 1) / (double)(n_out - 1) : 0.0; }      // np.linspace: delta / div

static int64_t period_tiles(int64_t n_samples) { return (n_samples + kPerTile - 1) / kPerTile; }

}  // namespace mmk

extern "C" int mmk_spline2_coef_f64(const float* y, int64_t y_row_stride, int32_t batch, int64_t n, double* coef, int64_t coef_row_stride,
                                    mmk_stream_t stream) {
  using namespace mmk;
  if (!y || !coef || batch <= 0 || (batch > 1 && (y_row_stride < 0 || coef_row_stride < n)))
    return fail(MMK_ERR_INVALID, "spline2_coef: bad arguments (batch=%d, n=%lld, row strides %lld / %lld)", batch, (long long)n, (long long)y_row_stride,
                (long long)coef_row_stride);
  if (misaligned(y, 4) || misaligned(coef, 8) || (batch > 1 && misaligned(coef + coef_row_stride, 8)))
    return fail(MMK_ERR_INVALID, "spline2_coef: y must be 4-byte and coef 8-byte aligned");
  if (n < 3) return fail(MMK_ERR_INVALID, "spline2_coef: a quadratic spline needs n >= 3 knots, got %lld", (long long)n);
  if (batch > 65535) return fail(MMK_ERR_UNSUPPORTED, "spline2_coef: %d rows are more than one launch takes (65535)", batch);
  const int64_t n_tiles = (n + kSpTile - 1) / kSpTile;
  if (n_tiles * batch > 0x7fffffffLL)
    return fail(MMK_ERR_UNSUPPORTED, "spline2_coef: %lld tiles of %d knots are more than one launch takes", (long long)(n_tiles * batch), kSpTile);
  return launch(spline2_coef_kernel, dim3((unsigned)(n_tiles * batch)), dim3(kSpTile), 0, (hipStream_t)stream, y, y_row_stride, n, n_tiles, coef,
                coef_row_stride);
}

extern "C" int mmk_spline2_eval_f32(const double* coef, int64_t coef_row_stride, int32_t batch, int64_t n, float* out, int64_t out_row_stride,
                                    int64_t n_out, mmk_stream_t stream) {
  using namespace mmk;
  if (!coef || !out || batch <= 0 || (batch > 1 && (coef_row_stride < 0 || out_row_stride < n_out)))
    return fail(MMK_ERR_INVALID, "spline2_eval: bad arguments (batch=%d, n=%lld, n_out=%lld, row strides %lld / %lld)", batch, (long long)n,
                (long long)n_out, (long long)coef_row_stride, (long long)out_row_stride);
  if (misaligned(out, 4)) return fail(MMK_ERR_INVALID, "spline2_eval: out must be 4-byte aligned");
  MMK_TRY(spline_ok("spline2_eval", coef, n));
  if (n_out < 1) return fail(MMK_ERR_INVALID, "spline2_eval: needs n_out >= 1 points, got %lld", (long long)n_out);
  if (batch > 65535) return fail(MMK_ERR_UNSUPPORTED, "spline2_eval: %d rows are more than one launch takes (65535)", batch);
  int64_t blocks = (n_out + MMK_SPLINE2_EVAL_TILE - 1) / MMK_SPLINE2_EVAL_TILE;
  blocks = blocks > 8192 ? 8192 : blocks;
  return launch(spline2_eval_kernel, dim3((unsigned)blocks, (unsigned)batch), dim3(MMK_SPLINE2_EVAL_TILE), 0, (hipStream_t)stream, coef,
                coef_row_stride, n, out, out_row_stride, n_out, linspace_step(n, n_out));
}

extern "C" size_t mmk_periods_workspace_bytes(int64_t n_samples) {
  return n_samples < 1 ? 0 : (size_t)mmk::period_tiles(n_samples) * 2 * sizeof(int64_t);
}

static int periods_ok(const char* what, const double* coef, int64_t n, const float* row, int64_t n_samples, const void* work, size_t work_bytes) {
  using namespace mmk;
  if ((coef != nullptr) == (row != nullptr)) return fail(MMK_ERR_INVALID, "%s: exactly one of coef (a spline) and row (its samples) must be given", what);
  if (coef) MMK_TRY(spline_ok(what, coef, n));
  if (row && misaligned(row, 4)) return fail(MMK_ERR_INVALID, "%s: row must be a float32 device pointer, 4-byte aligned", what);
  if (n_samples < 1) return fail(MMK_ERR_INVALID, "%s: n_samples = %lld < 1", what, (long long)n_samples);
  if (period_tiles(n_samples) > 0x7fffffffLL)
    return fail(MMK_ERR_UNSUPPORTED, "%s: %lld tiles of %d samples are more than one launch takes", what, (long long)period_tiles(n_samples), kPerTile);
  if (!work || misaligned(work, 8) || work_bytes < mmk_periods_workspace_bytes(n_samples))
    return fail(MMK_ERR_WORKSPACE, "%s: %zu bytes of 8-byte aligned workspace are needed, got %zu", what, mmk_periods_workspace_bytes(n_samples), work_bytes);
  return MMK_OK;
}

extern "C" int mmk_periods_count_i64(const double* coef, int64_t n, const float* row, int64_t n_samples, int64_t* counts, void* work, size_t work_bytes,
                                     mmk_stream_t stream) {
  using namespace mmk;
  MMK_TRY(periods_ok("periods_count", coef, n, row, n_samples, work, work_bytes));
  if (!counts || misaligned(counts, 8)) return fail(MMK_ERR_INVALID, "periods_count: counts must be an int64[2] device pointer");
  const int64_t n_tiles = period_tiles(n_samples);
  hipStream_t st = (hipStream_t)stream;
  const double step = coef ? linspace_step(n, n_samples) : 0.0;
  if (coef)
    MMK_TRY(launch(periods_kernel<0, 0>, dim3((unsigned)n_tiles), dim3(256), 0, st, coef, n, row, n_samples, step, (int64_t*)work, (int64_t)0,
                   (int64_t)0, (int64_t*)nullptr, (int64_t*)nullptr));
  else
    MMK_TRY(launch(periods_kernel<0, 1>, dim3((unsigned)n_tiles), dim3(256), 0, st, coef, n, row, n_samples, step, (int64_t*)work, (int64_t)0,
                   (int64_t)0, (int64_t*)nullptr, (int64_t*)nullptr));
  return launch(periods_scan_kernel, dim3(1), dim3(256), 0, st, (int64_t*)work, n_tiles, counts);
}

extern "C" int mmk_periods_fill_i64(const double* coef, int64_t n, const float* row, int64_t n_samples, const void* work, size_t work_bytes, int64_t n_att,
                                    int64_t n_peak, int64_t* att, int64_t* dec, int64_t* peaks, mmk_stream_t stream) {
  using namespace mmk;
  MMK_TRY(periods_ok("periods_fill", coef, n, row, n_samples, work, work_bytes));
  if (n_att < 0 || n_peak < 0 || 2 * n_att > n_samples + 1 || 2 * n_peak > n_samples + 1)
    return fail(MMK_ERR_INVALID, "periods_fill: n_att = %lld / n_peak = %lld of %lld samples (two of a kind are at least two samples apart)",
                (long long)n_att, (long long)n_peak, (long long)n_samples);
  if ((n_att > 0 && (!att || !dec)) || (n_peak > 0 && !peaks) || misaligned(att, 8) || misaligned(dec, 8) || misaligned(peaks, 8))
    return fail(MMK_ERR_INVALID, "periods_fill: att, dec and peaks must be int64 device pointers");
  if (n_att == 0 && n_peak == 0) return MMK_OK;
  hipStream_t st = (hipStream_t)stream;
  const double step = coef ? linspace_step(n, n_samples) : 0.0;
  const dim3 grid((unsigned)period_tiles(n_samples));
  if (coef) MMK_TRY(launch(periods_kernel<1, 0>, grid, dim3(256), 0, st, coef, n, row, n_samples, step, (int64_t*)work, n_att, n_peak, att, peaks));
  else MMK_TRY(launch(periods_kernel<1, 1>, grid, dim3(256), 0, st, coef, n, row, n_samples, step, (int64_t*)work, n_att, n_peak, att, peaks));
  if (n_att > 0)
    MMK_TRY(launch(periods_dec_kernel, dim3((unsigned)((n_att + 255) / 256)), dim3(256), 0, st, (const int64_t*)att, n_att, (const int64_t*)peaks, n_peak,
                   n_samples, dec));
  return MMK_OK;
}

extern "C" int mmk_samplify_scores_f32(const double* env_coef, int64_t n, int64_t n_samples, const int64_t* att, const int64_t* dec, int64_t count,
                                       float sensitivity, float* scores, float* env_att, float* env_dec, uint8_t* keep, mmk_stream_t stream) {
  using namespace mmk;
  MMK_TRY(spline_ok("samplify_scores", env_coef, n));
  if (n_samples < 1 || count < 0) return fail(MMK_ERR_INVALID, "samplify_scores: n_samples = %lld, count = %lld", (long long)n_samples, (long long)count);
  if (count == 0) return MMK_OK;
  if (!att || !dec || !scores || !env_att || !env_dec || !keep || misaligned(att, 8) || misaligned(dec, 8) || misaligned(scores, 4) ||
      misaligned(env_att, 4) || misaligned(env_dec, 4))
    return fail(MMK_ERR_INVALID, "samplify_scores: att / dec must be int64, scores / env_att / env_dec float32 and keep uint8 device pointers");
  if ((count + 255) / 256 > 0x7fffffffLL) return fail(MMK_ERR_UNSUPPORTED, "samplify_scores: count = %lld", (long long)count);
  return launch(samplify_scores_kernel, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, (hipStream_t)stream, env_coef, n, n_samples,
                linspace_step(n, n_samples), att, dec, count, sensitivity, scores, env_att, env_dec, keep);
}

extern "C" int mmk_samplify_cuts_i64(const float* y, int64_t n_samples, const double* const* env_coef, const double* const* grad_coef,
                                     const int64_t* n_knots, int32_t levels, const int64_t* coarse_cuts, const int64_t* coarse_peaks, int64_t count,
                                     int64_t* sides, float* lr_scores, int64_t* cuts, mmk_stream_t stream) {
  using namespace mmk;
  if (levels < 1 || levels > kMaxLevels)
    return fail(levels < 1 ? MMK_ERR_INVALID : MMK_ERR_UNSUPPORTED, "samplify_cuts: levels = %d, 1 .. %d (MMK_SAMPLIFY_MAX_LEVELS) are taken", levels, kMaxLevels);
  if (!y || misaligned(y, 4) || n_samples < 1 || count < 0 || !env_coef || !grad_coef || !n_knots)
    return fail(MMK_ERR_INVALID, "samplify_cuts: bad arguments (n_samples = %lld, count = %lld)", (long long)n_samples, (long long)count);
  SamplifyLevels lv;
  lv.levels = levels;
  for (int l = 0; l < kMaxLevels; ++l) {
    const int s = l < levels ? l : 0;                        // (unused slots repeat level 0: no lane reads them)
    MMK_TRY(spline_ok("samplify_cuts (env)", env_coef[s], n_knots[s]));
    MMK_TRY(spline_ok("samplify_cuts (grad)", grad_coef[s], n_knots[s]));
    lv.e[l] = env_coef[s];
    lv.g[l] = grad_coef[s];
    lv.n[l] = n_knots[s];
    lv.step[l] = linspace_step(n_knots[s], n_samples);
  }
  if (count == 0) return MMK_OK;
  if (!coarse_cuts || !coarse_peaks || !sides || !cuts || misaligned(coarse_cuts, 8) || misaligned(coarse_peaks, 8) || misaligned(sides, 8) ||
      misaligned(cuts, 8) || misaligned(lr_scores, 4))
    return fail(MMK_ERR_INVALID, "samplify_cuts: coarse_cuts / coarse_peaks / sides / cuts must be int64 device pointers, lr_scores float32 or NULL");
  if (count > 0x7fffffffLL) return fail(MMK_ERR_UNSUPPORTED, "samplify_cuts: count = %lld cuts are more than one launch takes", (long long)count);
  return launch(samplify_cuts_kernel, dim3((unsigned)count), dim3(kGroup), 0, (hipStream_t)stream, y, n_samples, lv, coarse_cuts, coarse_peaks, sides,
                lr_scores, cuts);
}
