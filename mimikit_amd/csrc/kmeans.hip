// K-means on the device (mimikit/extract/clusters.py:233-262 KMeans; include/mmk_kmeans.h): the nearest of a few centres for every frame,
// the float64 sums of every label's frames, and one step of k-means++ seeding.  Every kernel works on x' = fl32(x - offset), subtracted
// while loading; the centred corpus is never written.
//
//   kmeans_assign_kernel<KT>  key[r, j] = <x'_r, c_j> + shift[j] for k <= KT = 32, 64, 128, 256 centres.  The opposite shape of
//                         nn_search.h: there many corpus frames are walked in 128-wide tiles per span with a merge launch behind, here
//                         the "corpus" is a handful of centres that fit ONE tile.  A workgroup of four waves owns 128 rows, a wave 32 of
//                         them against all KT centres: KT / 32 products with A = centres and B = rows, the row on the lane and 16 centres
//                         in the registers - a row's candidates are met inside the lane in rising centre order, and "strictly greater"
//                         keeps the first.  The two half-waves hold the same rows against other centres and are joined by one shuffle
//                         (greater key, then lower index).  Rows and centres are staged and multiplied by the pieces of frame_walk.h:
//                         ONE order of the sum wherever they sit, and the search's order.  kNarrow, for d <= 16: a load covers 16 bins,
//                         not 32 (no lane loads a clamped duplicate), and the two groups of 8 bins that hold data are multiplied, not
//                         four; what is left out are products with zero.  The centres
//                         are re-staged per chunk by every workgroup (K D floats from L2 against 128 D floats of rows from HBM: 1/8 more
//                         LDS traffic at K = 16) rather than kept resident, which would cap K D at the LDS and give one workgroup per CU.
//                         (A workgroup that walks several row blocks with the next block's loads in flight was tried and was no faster.)
//                         The instances for up to 128 centres interleave their independent products and keep two waves per SIMD; the
//                         256-centre instance holds 128 accumulator registers, runs product by product and has one wave per SIMD.
//                         The label is read, compared and overwritten by the lane that owns the row; the rows that changed are counted
//                         per wave (ballot) and added with one integer atomic.
//   kmeans_sums_kernel    one WAVE per (slab of rows, chunk of P <= 64 columns): k x P float64 accumulators in LDS, the wave's 64 lanes are
//                         64 / P consecutive rows by P columns (coalesced), four row groups in flight.  Rows that are loaded together may
//                         share a label, so they are added one row at a time with a barrier between them - in rising row order, which
//                         is the slab's one order.  kmeans_sums_combine adds the slabs' partials in rising slab order.
//   row_d2 (device function)  |x'_r - o|^2: a wave per row, lane l takes bins l, l + 64, ... (the float64 difference of two floats is exact,
//                         its square is added by fma), then a butterfly of shuffles - every lane ends with the same sum.
//   kmeans_d2_kernel      row_d2 against the row's centre; a workgroup owns a slab, wave w its rows w, w + 4, ...; the four waves' sums are
//                         added in wave order, the slabs' by kmeans_reduce_kernel (thread i takes slabs i, i + 256, ..., then a tree).
//   kmeans_pp_*           the seeding step in three launches: the t pots per slab (row_d2 against every candidate row), the pick (the pots
//                         in the fixed order, the first smallest wins), and closest <- min(closest, |x' - x'_chosen|^2) by the same
//                         function, so the pot IS the sum of what is written.
// No floating-point atomics, no workgroup waits for another.  NaN and inf in the inputs are not handled.
#include "nn_search.h"

#include "../../include/mmk_kmeans.h"

namespace mmk {

constexpr int kKmRows = 128;              // rows of an assign workgroup, 32 per wave
constexpr int kKmSlabs = MMK_KMEANS_MAX_SLABS;
constexpr int kKmTrials = MMK_KMEANS_PP_MAX_TRIALS;
constexpr int64_t kKmSumsBudget = 64ll << 20;      // bytes of slab partials the sums may take
constexpr int kKmSumsLds = 60000;         // bytes of LDS one wave of the sums kernel may take (below the 64 KB a plain launch gets)

// the wave's 32 rows against all centres: the lane's candidates in rising centre order, the other half-wave's best by one shuffle, the label
// compared and overwritten by the lane that owns the row
template <int KT>
__device__ __forceinline__ void assign_epilogue(fw_f32x16 (&acc)[KT / 32], const float* shs, int32_t K, int64_t rbase, int64_t n, int wave, int lane,
                                                int32_t* __restrict__ labels, float* __restrict__ key, unsigned long long* __restrict__ changed) {
  constexpr int NP = KT / 32;
  const int fr = lane & 31, fh = lane >> 5;
  float best = __int_as_float(0xff800000);
  int bj = kNnEmpty;
#pragma unroll
  for (int p = 0; p < NP; ++p)
#pragma unroll
    for (int q = 0; q < 16; ++q) {
      const int j = fw_acc_row(p * 32, q, fh);
      const float c = __fadd_rn(acc[p][q], shs[j]);
      if (j < K && c > best) {
        best = c;
        bj = j;
      }
    }
  const float ok = __shfl_xor(best, 32);
  const int oj = __shfl_xor(bj, 32);
  if (nn_better(ok, oj, best, bj)) {
    best = ok;
    bj = oj;
  }
  const int64_t r = rbase + wave * 32 + fr;
  bool differs = false;
  if (fh == 0 && r < n) {
    differs = labels[r] != bj;
    labels[r] = bj;
    if (key) key[r] = best;
  }
  const unsigned long long moved = __ballot(differs);
  if (changed && lane == 0 && moved) atomicAdd(changed, (unsigned long long)__popcll(moved));
}

template <int KT, bool kNarrow>
__global__ __launch_bounds__(256, KT <= 128 ? 2 : 1) void kmeans_assign_kernel(const float* __restrict__ x, int64_t x_row_stride, const float* __restrict__ offset,
                                                             int64_t n, int32_t D, const float* __restrict__ centres, int64_t c_row_stride,
                                                             const float* __restrict__ shift, int32_t K,
                                                             int32_t* __restrict__ labels, float* __restrict__ key,
                                                             unsigned long long* __restrict__ changed) {
  constexpr int NP = KT / 32;                       // products of a wave
  constexpr int LC = kNarrow ? 16 : 32;             // bins a load covers: lanes on consecutive bins
  constexpr int RS = 256 / LC;                      // rows between a thread's loads
  constexpr int CL = KT / RS, XL = kKmRows / RS;    // centre and row dwords a thread loads per chunk
  __shared__ __attribute__((aligned(16))) float cs[KT * kFwPitch];
  __shared__ __attribute__((aligned(16))) float xs[kKmRows * kFwPitch];
  __shared__ float shs[KT];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int col = tid & (LC - 1), row0 = tid / LC;  // loads: bin `col` of rows row0, row0 + RS, ...
  const int fr = lane & 31, fh = lane >> 5;         // MFMA fragments: row / centre fr, bin half fh

  if (tid < KT) shs[tid] = tid < K ? shift[tid] : 0.f;
  fw_f32x16 acc[NP];
#pragma unroll
  for (int p = 0; p < NP; ++p)
#pragma unroll
    for (int q = 0; q < 16; ++q) acc[p][q] = 0.f;

  const int64_t rbase = (int64_t)blockIdx.x * kKmRows;
  float rg[CL + XL];
  auto gload = [&](int k0) {
    const float mu = offset ? offset[fw_bin(k0 + col, D)] : 0.f;
    fw_load<CL, RS, 0>(rg, centres, c_row_stride, 0, K, row0, col, k0, D);
    fw_load<XL, RS, CL>(rg, x, x_row_stride, rbase, n, row0, col, k0, D, [mu](float v) { return __fsub_rn(v, mu); });
  };
  gload(0);
  for (int k0 = 0; k0 < D; k0 += kFwKC) {
    const bool kin = k0 + col < D;
#pragma unroll
    for (int i = 0; i < CL; ++i) cs[(i * RS + row0) * kFwPitch + col] = (kin && i * RS + row0 < K) ? rg[i] : 0.f;
#pragma unroll
    for (int i = 0; i < XL; ++i) xs[(i * RS + row0) * kFwPitch + col] = (kin && rbase + i * RS + row0 < n) ? rg[CL + i] : 0.f;
    __syncthreads();
    if (k0 + kFwKC < D) gload(k0 + kFwKC);
#pragma unroll
    for (int g = 0; g < LC; g += 8) {
      const fw_f32x4 bv = fw_frag(xs, wave * 32 + fr, g, fh);
      if constexpr (KT <= 128) {                    // independent products interleaved
        fw_f32x4 av[NP];
#pragma unroll
        for (int p = 0; p < NP; ++p) av[p] = fw_frag(cs, p * 32 + fr, g, fh);
#pragma unroll
        for (int e = 0; e < 4; ++e)
#pragma unroll
          for (int p = 0; p < NP; ++p) fw_mfma(acc[p], av[p], bv, e);
      } else {                                      // product by product: four centre registers live, not 4 NP; the sum's order is the same
#pragma unroll
        for (int p = 0; p < NP; ++p) fw_mma(acc[p], fw_frag(cs, p * 32 + fr, g, fh), bv);
      }
    }
    __syncthreads();
  }
  assign_epilogue<KT>(acc, shs, K, rbase, n, wave, lane, labels, key, changed);
}

// ---- float64 sums of every label's rows ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void kmeans_sums_kernel(const float* __restrict__ x, int64_t x_row_stride, const float* __restrict__ offset, int64_t n,
                                                         int32_t D, const int32_t* __restrict__ labels, int32_t K, int32_t plog,
                                                         int64_t rows_per_slab, int32_t chunks, double* __restrict__ ws_sums,
                                                         long long* __restrict__ ws_counts) {
  extern __shared__ double km_lds[];                // K x P sums, then K counts
  const int P = 1 << plog, SUB = 64 >> plog;
  long long* cnt = reinterpret_cast<long long*>(km_lds + (size_t)K * P);
  const int lane = threadIdx.x, sub = lane >> plog, cl = lane & (P - 1);
  const int64_t slab = blockIdx.x / chunks;
  const int chunk = blockIdx.x % chunks;
  const int colv = chunk * P + cl;
  const bool colok = colv < D;
  const int cc = colok ? colv : D - 1;
  const bool counts_here = chunk == 0 && cl == 0;
  for (int i = lane; i < K * P; i += 64) km_lds[i] = 0.0;
  for (int i = lane; i < K; i += 64) cnt[i] = 0;
  __syncthreads();
  const float mu = offset ? offset[cc] : 0.f;
  const int64_t begin = slab * rows_per_slab;
  const int64_t end = begin + rows_per_slab < n ? begin + rows_per_slab : n;
  for (int64_t r0 = begin; r0 < end; r0 += 4 * SUB) {
    float v[4];
    int l[4];
    bool ok[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int64_t r = r0 + u * SUB + sub;
      const int64_t rr = r < end ? r : end - 1;
      v[u] = x[rr * x_row_stride + cc];
      l[u] = labels[rr];
      ok[u] = r < end && (unsigned)l[u] < (unsigned)K;
    }
#pragma unroll
    for (int u = 0; u < 4; ++u)
      for (int s = 0; s < SUB; ++s) {              // one row at a time: rows of one load may share a label, and the order is the row order
        if (sub == s && ok[u]) {
          if (colok) km_lds[l[u] * P + cl] += (double)__fsub_rn(v[u], mu);
          if (counts_here) cnt[l[u]] += 1;
        }
        __syncthreads();
      }
  }
  for (int i = lane; i < K * P; i += 64) {
    const int j = i >> plog, c = chunk * P + (i & (P - 1));
    if (c < D) ws_sums[(slab * K + j) * D + c] = km_lds[i];
  }
  if (chunk == 0)
    for (int i = lane; i < K; i += 64) ws_counts[slab * K + i] = cnt[i];
}

__global__ __launch_bounds__(256) void kmeans_sums_combine(const double* __restrict__ ws_sums, const long long* __restrict__ ws_counts, int64_t kd,
                                                           int32_t K, int32_t slabs, double* __restrict__ sums, int64_t* __restrict__ counts) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < kd) {
    double a = 0.0;
    for (int s = 0; s < slabs; ++s) a += ws_sums[s * kd + i];
    sums[i] = a;
  } else if (i < kd + K) {
    const int64_t j = i - kd;
    long long a = 0;
    for (int s = 0; s < slabs; ++s) a += ws_counts[(int64_t)s * K + j];
    counts[j] = a;
  }
}

// ---- squared distances in float64 -----------------------------------------------------------------------------------------------------
// |x'_r - o|^2 over D bins by one wave; kCentred: o is a row of x (the offset is subtracted from it as well), else a centre
template <bool kCentred>
__device__ __forceinline__ double row_d2(const float* __restrict__ xr, const float* __restrict__ o, const float* __restrict__ offset, int D, int lane) {
  double a = 0.0;
  for (int c = lane; c < D; c += 64) {
    const float mu = offset ? offset[c] : 0.f;
    const float xv = __fsub_rn(xr[c], mu);
    const float ov = kCentred ? __fsub_rn(o[c], mu) : o[c];
    const double df = (double)xv - (double)ov;
    a = fma(df, df, a);
  }
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) a += __shfl_xor(a, off);
  return a;
}

static inline int dist_slabs(int64_t n) { return (int)((n + 3) / 4 < kKmSlabs ? (n + 3) / 4 : kKmSlabs); }

__global__ __launch_bounds__(256) void kmeans_d2_kernel(const float* __restrict__ x, int64_t x_row_stride, const float* __restrict__ offset, int64_t n,
                                                        int32_t D, const int32_t* __restrict__ labels, int32_t K, const float* __restrict__ centres,
                                                        int64_t c_row_stride, int64_t rows_per_slab, double* __restrict__ row_out,
                                                        double* __restrict__ ws_part) {
  __shared__ double part[4];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t begin = (int64_t)blockIdx.x * rows_per_slab;
  const int64_t end = begin + rows_per_slab < n ? begin + rows_per_slab : n;
  double acc = 0.0;
  for (int64_t r = begin + wave; r < end; r += 4) {
    const int l = labels[r];
    double dd = 0.0;
    if ((unsigned)l < (unsigned)K) dd = row_d2<false>(x + r * x_row_stride, centres + (int64_t)l * c_row_stride, offset, D, lane);
    if (row_out && lane == 0) row_out[r] = dd;
    acc += dd;
  }
  if (lane == 0) part[wave] = acc;
  __syncthreads();
  if (threadIdx.x == 0) ws_part[blockIdx.x] = ((part[0] + part[1]) + part[2]) + part[3];
}

// out[i] = the sum of in[s * width + i] over s < slabs for i < width <= 8: thread t takes s = t, t + 256, ..., then a tree
__device__ __forceinline__ double reduce_slabs(const double* __restrict__ in, int width, int i, int slabs, double* red) {
  const int tid = threadIdx.x;
  double a = 0.0;
  for (int s = tid; s < slabs; s += 256) a += in[(int64_t)s * width + i];
  red[tid] = a;
  __syncthreads();
  for (int off = 128; off >= 1; off >>= 1) {
    if (tid < off) red[tid] += red[tid + off];
    __syncthreads();
  }
  const double total = red[0];
  __syncthreads();
  return total;
}

__global__ __launch_bounds__(256) void kmeans_reduce_kernel(const double* __restrict__ ws_part, int32_t slabs, double* __restrict__ out) {
  __shared__ double red[256];
  const double total = reduce_slabs(ws_part, 1, 0, slabs, red);
  if (threadIdx.x == 0) *out = total;
}

// ---- k-means++ seeding step ---------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ int64_t clamp_row(int64_t c, int64_t n) { return c < 0 || c >= n ? n - 1 : c; }

__global__ __launch_bounds__(256) void kmeans_pp_pots_kernel(const float* __restrict__ x, int64_t x_row_stride, const float* __restrict__ offset,
                                                             int64_t n, int32_t D, const int64_t* __restrict__ cand, int32_t T,
                                                             const double* __restrict__ closest, int64_t rows_per_slab,
                                                             double* __restrict__ ws_pots) {
  __shared__ double part[4][kKmTrials];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t begin = (int64_t)blockIdx.x * rows_per_slab;
  const int64_t end = begin + rows_per_slab < n ? begin + rows_per_slab : n;
  const float* crow[kKmTrials];
  double acc[kKmTrials];
#pragma unroll
  for (int i = 0; i < kKmTrials; ++i) {
    crow[i] = x + clamp_row(cand[i < T ? i : 0], n) * x_row_stride;
    acc[i] = 0.0;
  }
  for (int64_t r = begin + wave; r < end; r += 4) {
    const double cl = closest[r];
#pragma unroll
    for (int i = 0; i < kKmTrials; ++i)
      if (i < T) {
        const double dd = row_d2<true>(x + r * x_row_stride, crow[i], offset, D, lane);
        acc[i] += dd < cl ? dd : cl;
      }
  }
  if (lane == 0) {
#pragma unroll
    for (int i = 0; i < kKmTrials; ++i) part[wave][i] = acc[i];
  }
  __syncthreads();
  if (threadIdx.x < kKmTrials) {
    const int i = threadIdx.x;
    ws_pots[(int64_t)blockIdx.x * kKmTrials + i] = ((part[0][i] + part[1][i]) + part[2][i]) + part[3][i];
  }
}

__global__ __launch_bounds__(256) void kmeans_pp_pick_kernel(const double* __restrict__ ws_pots, int32_t slabs, const int64_t* __restrict__ cand, int32_t T,
                                                             int64_t n, double* __restrict__ pot, int64_t* __restrict__ chosen,
                                                             int64_t* __restrict__ ws_row) {
  __shared__ double red[256];
  double best = 0.0;
  int bi = 0;
  for (int i = 0; i < T; ++i) {
    const double p = reduce_slabs(ws_pots, kKmTrials, i, slabs, red);
    if (i == 0 || p < best) {
      best = p;
      bi = i;
    }
  }
  if (threadIdx.x == 0) {
    *pot = best;
    *chosen = cand[bi];
    *ws_row = clamp_row(cand[bi], n);
  }
}

__global__ __launch_bounds__(256) void kmeans_pp_apply_kernel(const float* __restrict__ x, int64_t x_row_stride, const float* __restrict__ offset,
                                                              int64_t n, int32_t D, const int64_t* __restrict__ ws_row, int64_t rows_per_slab,
                                                              double* __restrict__ closest) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t begin = (int64_t)blockIdx.x * rows_per_slab;
  const int64_t end = begin + rows_per_slab < n ? begin + rows_per_slab : n;
  const float* crow = x + clamp_row(*ws_row, n) * x_row_stride;
  for (int64_t r = begin + wave; r < end; r += 4) {
    const double dd = row_d2<true>(x + r * x_row_stride, crow, offset, D, lane);
    if (lane == 0 && dd < closest[r]) closest[r] = dd;
  }
}

// the sums' partition: as many slabs as the budget of partials allows, at most kKmSlabs, at least 64 rows each
static inline int sums_slabs(int64_t n, int32_t d, int32_t k) {
  const int64_t per = (int64_t)k * d * 8;
  int64_t cap = kKmSumsBudget / per;
  cap = cap < 1 ? 1 : cap > kKmSlabs ? kKmSlabs : cap;
  const int64_t need = (n + 63) / 64;
  return (int)(need < cap ? need : cap);
}
// columns of a chunk: the power of two that covers d, at most 64, halved until k x P float64 and k counts fit the wave's LDS (0: they never do)
static inline int sums_plog(int32_t d, int32_t k) {
  int plog = 0;
  while (plog < 6 && (1 << plog) < d) ++plog;
  while (plog > 0 && (int64_t)k * (8 * (1 << plog) + 8) > kKmSumsLds) --plog;
  return (int64_t)k * (8 * (1 << plog) + 8) > kKmSumsLds ? -1 : plog;
}

}  // namespace mmk

extern "C" int mmk_kmeans_assign_f32(const float* x, int64_t x_row_stride, const float* offset, int64_t n, int32_t d, const float* centres,
                                     int64_t c_row_stride, const float* shift, int32_t k, int32_t* labels, float* key, int64_t* changed,
                                     mmk_stream_t stream) {
  using namespace mmk;
  if (n < 1 || d < 1 || k < 1) return fail(MMK_ERR_INVALID, "kmeans_assign: n = %lld, d = %d, k = %d (all at least 1)", (long long)n, d, k);
  if (k > MMK_KMEANS_MAX_K)
    return fail(MMK_ERR_UNSUPPORTED, "kmeans_assign: k = %d centres, more than the %d (MMK_KMEANS_MAX_K) of the widest centre tile", k, MMK_KMEANS_MAX_K);
  if (!x || !centres || !shift || !labels || x_row_stride < 0 || c_row_stride < 0)
    return fail(MMK_ERR_INVALID, "kmeans_assign: bad arguments (null pointer or negative stride %lld / %lld)", (long long)x_row_stride, (long long)c_row_stride);
  if (misaligned(x, 4) || misaligned(offset, 4) || misaligned(centres, 4) || misaligned(shift, 4) || misaligned(labels, 4) || misaligned(key, 4))
    return fail(MMK_ERR_INVALID, "kmeans_assign: x, offset, centres, shift, labels and key must be 4-byte aligned");
  if (misaligned(changed, 8)) return fail(MMK_ERR_INVALID, "kmeans_assign: changed must be 8-byte aligned");
  const int64_t n_blocks = (n + kKmRows - 1) / kKmRows;
  if (n_blocks > 0x7fffffffLL) return fail(MMK_ERR_UNSUPPORTED, "kmeans_assign: %lld rows are more than one launch takes", (long long)n);
  const dim3 grid((unsigned)n_blocks), block(256);
  unsigned long long* ch = reinterpret_cast<unsigned long long*>(changed);
  hipStream_t st = (hipStream_t)stream;
#define MMK_KM_ASSIGN(KT, NARROW) \
  launch(kmeans_assign_kernel<KT, NARROW>, grid, block, 0, st, x, x_row_stride, offset, n, d, centres, c_row_stride, shift, k, labels, key, ch)
  if (d <= 16) {
    if (k <= 32) return MMK_KM_ASSIGN(32, true);
    if (k <= 64) return MMK_KM_ASSIGN(64, true);
    if (k <= 128) return MMK_KM_ASSIGN(128, true);
    return MMK_KM_ASSIGN(256, true);
  }
  if (k <= 32) return MMK_KM_ASSIGN(32, false);
  if (k <= 64) return MMK_KM_ASSIGN(64, false);
  if (k <= 128) return MMK_KM_ASSIGN(128, false);
  return MMK_KM_ASSIGN(256, false);
#undef MMK_KM_ASSIGN
}

extern "C" size_t mmk_kmeans_label_sums_workspace_bytes(int64_t n, int32_t d, int32_t k) {
  using namespace mmk;
  if (n < 1 || d < 1 || k < 1) return 0;
  const size_t slabs = (size_t)sums_slabs(n, d, k);
  return slabs * (size_t)k * ((size_t)d + 1) * 8 + (size_t)kKmSlabs * 8;
}

extern "C" int mmk_kmeans_label_sums_f64(const float* x, int64_t x_row_stride, const float* offset, int64_t n, int32_t d, const int32_t* labels,
                                         int32_t k, double* sums, int64_t* counts, const float* centres, int64_t c_row_stride, double* row_d2,
                                         double* inertia, void* workspace, size_t workspace_bytes, mmk_stream_t stream) {
  using namespace mmk;
  if (n < 1 || d < 1 || k < 1) return fail(MMK_ERR_INVALID, "kmeans_label_sums: n = %lld, d = %d, k = %d (all at least 1)", (long long)n, d, k);
  if (!x || !labels || !sums || !counts || x_row_stride < 0 || c_row_stride < 0)
    return fail(MMK_ERR_INVALID, "kmeans_label_sums: bad arguments (null pointer or negative stride %lld / %lld)", (long long)x_row_stride,
                (long long)c_row_stride);
  if (!centres && (row_d2 || inertia)) return fail(MMK_ERR_INVALID, "kmeans_label_sums: row_d2 and inertia need the centres");
  if (misaligned(x, 4) || misaligned(offset, 4) || misaligned(labels, 4) || misaligned(centres, 4))
    return fail(MMK_ERR_INVALID, "kmeans_label_sums: x, offset, labels and centres must be 4-byte aligned");
  if (misaligned(sums, 8) || misaligned(counts, 8) || misaligned(row_d2, 8) || misaligned(inertia, 8))
    return fail(MMK_ERR_INVALID, "kmeans_label_sums: sums, counts, row_d2 and inertia must be 8-byte aligned");
  const int plog = sums_plog(d, k);
  if (plog < 0) return fail(MMK_ERR_UNSUPPORTED, "kmeans_label_sums: k = %d labels: their counts alone do not fit a wave's %d bytes of LDS", k, kKmSumsLds);
  const size_t need = mmk_kmeans_label_sums_workspace_bytes(n, d, k);
  if (!workspace || misaligned(workspace, 8) || workspace_bytes < need)
    return fail(MMK_ERR_WORKSPACE, "kmeans_label_sums: the workspace has %zu bytes, %zu are needed, 8-byte aligned", workspace_bytes, need);
  const int slabs = sums_slabs(n, d, k);
  const int64_t rows_per_slab = (n + slabs - 1) / slabs;
  const int64_t chunks = ((int64_t)d + (1 << plog) - 1) >> plog;
  if (chunks * slabs > 0x7fffffffLL || (int64_t)k * d > (int64_t)0x7fffffff * 128)
    return fail(MMK_ERR_UNSUPPORTED, "kmeans_label_sums: d = %d by k = %d is more than one launch takes", d, k);
  hipStream_t st = (hipStream_t)stream;
  const int64_t kd = (int64_t)k * d;
  double* ws_sums = static_cast<double*>(workspace);
  long long* ws_counts = reinterpret_cast<long long*>(ws_sums + (size_t)slabs * kd);
  double* ws_part = reinterpret_cast<double*>(ws_counts + (size_t)slabs * k);
  const size_t lds = (size_t)k * (8 * ((size_t)1 << plog) + 8);
  MMK_TRY(launch(kmeans_sums_kernel, dim3((unsigned)(chunks * slabs)), dim3(64), lds, st, x, x_row_stride, offset, n, d, labels, k, plog, rows_per_slab,
                 (int32_t)chunks, ws_sums, ws_counts));
  MMK_TRY(launch(kmeans_sums_combine, dim3((unsigned)((kd + k + 255) / 256)), dim3(256), 0, st, ws_sums, ws_counts, kd, k, slabs, sums, counts));
  if (centres && (row_d2 || inertia)) {
    const int ds = dist_slabs(n);
    const int64_t rps = (n + ds - 1) / ds;
    MMK_TRY(launch(kmeans_d2_kernel, dim3(ds), dim3(256), 0, st, x, x_row_stride, offset, n, d, labels, k, centres, c_row_stride, rps, row_d2, ws_part));
    if (inertia) MMK_TRY(launch(kmeans_reduce_kernel, dim3(1), dim3(256), 0, st, ws_part, ds, inertia));
  }
  return MMK_OK;
}

extern "C" size_t mmk_kmeans_pp_step_workspace_bytes(void) { return ((size_t)MMK_KMEANS_MAX_SLABS * MMK_KMEANS_PP_MAX_TRIALS + 1) * 8; }

extern "C" int mmk_kmeans_pp_step_f64(const float* x, int64_t x_row_stride, const float* offset, int64_t n, int32_t d, const int64_t* cand, int32_t t,
                                      double* closest, double* pot, int64_t* chosen, void* workspace, size_t workspace_bytes, mmk_stream_t stream) {
  using namespace mmk;
  if (n < 1 || d < 1 || t < 1) return fail(MMK_ERR_INVALID, "kmeans_pp_step: n = %lld, d = %d, t = %d (all at least 1)", (long long)n, d, t);
  if (t > MMK_KMEANS_PP_MAX_TRIALS)
    return fail(MMK_ERR_UNSUPPORTED, "kmeans_pp_step: t = %d candidates, more than %d (MMK_KMEANS_PP_MAX_TRIALS)", t, MMK_KMEANS_PP_MAX_TRIALS);
  if (!x || !cand || !closest || !pot || !chosen || x_row_stride < 0)
    return fail(MMK_ERR_INVALID, "kmeans_pp_step: bad arguments (null pointer or negative stride %lld)", (long long)x_row_stride);
  if (misaligned(x, 4) || misaligned(offset, 4)) return fail(MMK_ERR_INVALID, "kmeans_pp_step: x and offset must be 4-byte aligned");
  if (misaligned(cand, 8) || misaligned(closest, 8) || misaligned(pot, 8) || misaligned(chosen, 8))
    return fail(MMK_ERR_INVALID, "kmeans_pp_step: cand, closest, pot and chosen must be 8-byte aligned");
  if (!workspace || misaligned(workspace, 8) || workspace_bytes < mmk_kmeans_pp_step_workspace_bytes())
    return fail(MMK_ERR_WORKSPACE, "kmeans_pp_step: the workspace has %zu bytes, %zu are needed, 8-byte aligned", workspace_bytes,
                mmk_kmeans_pp_step_workspace_bytes());
  hipStream_t st = (hipStream_t)stream;
  const int slabs = dist_slabs(n);
  const int64_t rps = (n + slabs - 1) / slabs;
  double* ws_pots = static_cast<double*>(workspace);
  int64_t* ws_row = reinterpret_cast<int64_t*>(ws_pots + (size_t)MMK_KMEANS_MAX_SLABS * MMK_KMEANS_PP_MAX_TRIALS);
  MMK_TRY(launch(kmeans_pp_pots_kernel, dim3(slabs), dim3(256), 0, st, x, x_row_stride, offset, n, d, cand, t, closest, rps, ws_pots));
  MMK_TRY(launch(kmeans_pp_pick_kernel, dim3(1), dim3(256), 0, st, ws_pots, slabs, cand, t, n, pot, chosen, ws_row));
  return launch(kmeans_pp_apply_kernel, dim3(slabs), dim3(256), 0, st, x, x_row_stride, offset, n, d, ws_row, rps, closest);
}
