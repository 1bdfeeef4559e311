// Non-negative matrix factorisation of corpus frames (mimikit/features/functionals.py:1141-1170 NMF = sklearn.decomposition.NMF with its
// defaults: the NNDSVDA start, the cyclic coordinate-descent solver, Frobenius loss, no regularisation).  Everything is fp64 inside; the
// frames are fp32 and converted while they are loaded.  No atomics, every sum in one fixed order: two calls give the same bits.
//
//   start        G = X^T X by mmk_pca_cov_f64 (mean 0, scale 1; it divides by n - 1, the eigenvalues are multiplied back), the k leading
//                eigenpairs by mmk_pca_eig_f64, u_j = X v_j / S_j by the row kernel below, the norms of the signed parts by per-run
//                partial sums added in rising run order, then sklearn's choice of part, scaling, cut at 1e-6 and fill with mean(X).
//   row side     (the W half-sweep) one lane per row of X, kNfRows rows per workgroup.  The rows' tile of X goes through LDS (loaded
//                along the rows, read along the columns), a tile of H^T beside it is read as broadcasts; the lane's row of X H^T, its
//                row of W and the k sequential coordinate updates stay in registers, H H^T (32 KB at k = 64) is read from LDS as
//                broadcasts.  X H^T is never written.  The lanes' violations are added per workgroup (wave tree, waves in rising
//                order) and the workgroups' sums by a second launch.
//   column side  (the H half-sweep) X^T W is a sum over the rows: a workgroup owns 64 columns and one run of rows, a lane one column
//                and a quarter of the k components; W goes through LDS, X is read in place (coalesced along the columns).  The runs'
//                partial (d, k) blocks are added in rising run order by the sweep kernel, one lane per row of H^T.
//   Gram         H H^T and W^T W: per-run partial (k, k) blocks, added in rising run order.
//   convergence  a device flag takes the iteration that met sklearn's stop rule; every kernel of a later iteration returns at once.
//
// The MFMA units are not used: the products are fp64 FMA chains fed by LDS broadcast reads.  Measured, an iteration at
// k = 16 is 11 times its floor of two streaming reads of X - the products on v_mfma_f64_16x16x4_f64 are the next step.
#include "entry_util.h"
#include "wave_ops.h"

#include <math.h>

#include "../../include/mmk_nmf.h"

namespace mmk {

constexpr int kNfRows = 128;          // rows of a workgroup on the row side: one lane per row
constexpr int kNfCols = 32;           // columns of X per LDS tile on the row side
constexpr int kNfXtCols = 64;         // columns of a workgroup on the column side
constexpr int kNfXtRows = 32;         // rows of W per LDS tile on the column side
constexpr int kNfMinRun = 256;        // fewest rows of a run
constexpr int kNfTargetGroups = 1024; // workgroups asked for across column blocks and runs
constexpr int kNfGramRuns = 256;      // most runs of a Gram sum
constexpr int kNfGramRows = 64;       // rows per LDS tile of the Gram kernel
constexpr int kNfStatChunks = 1024;   // most row chunks of the mean / min reduction
static_assert(MMK_NMF_MAX_COMPONENTS == 64, "the kernels are instantiated for 4, 8, 16, 32 and 64 padded components");

struct NfPlan {
  int kp;                      // k padded to 4, 8, 16, 32 or 64
  int runs;                    // of X^T W
  int64_t rows_per_run;
  int gruns_n, gruns_d;        // of W^T W and H H^T
  int64_t grows_n, grows_d;
  int64_t nbw, nbh;            // workgroups of the two sweeps
  int chunks;                  // of the mean / min reduction
  int64_t rows_per_chunk;
};

static void nf_gram_plan(int64_t m, int& runs, int64_t& rows) {
  int64_t r = (m + kNfMinRun - 1) / kNfMinRun;
  if (r > kNfGramRuns) r = kNfGramRuns;
  rows = round_up((m + r - 1) / r, kNfGramRows);
  runs = (int)((m + rows - 1) / rows);
}

static NfPlan nf_plan(int64_t n, int32_t d, int32_t k) {
  NfPlan p;
  p.kp = 4;
  while (p.kp < k) p.kp *= 2;
  const int colblocks = (d + kNfXtCols - 1) / kNfXtCols;
  int64_t want = (kNfTargetGroups + colblocks - 1) / colblocks;
  const int64_t most = (n + kNfMinRun - 1) / kNfMinRun;
  if (want > most) want = most;
  if (want < 1) want = 1;
  p.rows_per_run = round_up((n + want - 1) / want, kNfXtRows);
  p.runs = (int)((n + p.rows_per_run - 1) / p.rows_per_run);
  nf_gram_plan(n, p.gruns_n, p.grows_n);
  nf_gram_plan(d, p.gruns_d, p.grows_d);
  p.nbw = (n + kNfRows - 1) / kNfRows;
  p.nbh = (d + kNfRows - 1) / kNfRows;
  int64_t c = (n + 63) / 64;
  p.chunks = (int)(c < kNfStatChunks ? c : kNfStatChunks);
  p.rows_per_chunk = (n + p.chunks - 1) / p.chunks;
  return p;
}

// ---------------------------------------------------------------------------------------------------------------- the coordinate sweep
// b: the row of X B, a: the row of A (both in registers, zero beyond k), gs: B^T B in LDS, KP x KP, zero beyond k.  Returns the row's violation
template <int KP>
__device__ __forceinline__ double nf_sweep(const double (&b)[KP], double (&a)[KP], const double* gs, int k) {
  double viol = 0.0;
#pragma unroll
  for (int t = 0; t < KP; ++t) {
    if (t < k) {
      double g = -b[t];
#pragma unroll
      for (int r = 0; r < KP; ++r) g = fma(gs[t * KP + r], a[r], g);
      const double pg = a[t] == 0.0 ? fmin(0.0, g) : g;
      viol += fabs(pg);
      const double h = gs[t * KP + t];
      if (h != 0.0) a[t] = fmax(a[t] - g / h, 0.0);
    }
  }
  return viol;
}

template <int KP>
__device__ __forceinline__ void nf_load_gram(const double* __restrict__ gram, int k, double* gs) {
  for (int idx = threadIdx.x; idx < KP * KP; idx += blockDim.x) {
    const int t = idx / KP, r = idx % KP;
    gs[idx] = (t < k && r < k) ? gram[t * k + r] : 0.0;
  }
}

// ---------------------------------------------------------------------------------------------------------------- row side
// MODE 0: the W half-sweep (aux = H H^T (k, k); a = W, in place; vpart[workgroup] = its violation)
// MODE 1: a[i][t] = (X B)[i][t] / aux[t]   (the start's u_j = X v_j / S_j)
template <int KP, int MODE>
__global__ __launch_bounds__(kNfRows) void nmf_rows_kernel(const float* __restrict__ x, int64_t x_row_stride, int64_t n, int32_t d, int32_t k,
                                                           const double* __restrict__ bt, const double* __restrict__ aux, double* __restrict__ a,
                                                           double* __restrict__ vpart, const int32_t* __restrict__ done) {
  // the tiles of the product and, after it, H H^T share one buffer: 33 KB at k = 64
  constexpr int kTiles = kNfCols * KP + (kNfRows * (kNfCols + 1) + 1) / 2;
  __shared__ double smem[(MODE == 0 && KP * KP > kTiles) ? KP * KP : kTiles];
  __shared__ double red[kNfRows / 64];
  double* bs = smem;
  float* xt = reinterpret_cast<float*>(smem + kNfCols * KP);
  double* gs = smem;
  if (done && *done) return;
  const int tid = threadIdx.x;
  const int64_t rbase = (int64_t)blockIdx.x * kNfRows;
  const int64_t row = rbase + tid;
  const bool live = row < n;
  double acc[KP];
#pragma unroll
  for (int t = 0; t < KP; ++t) acc[t] = 0.0;
  const int lc = tid & (kNfCols - 1), lr = tid / kNfCols;      // the tile is loaded along the rows of x: 32 lanes on 32 columns
  for (int j0 = 0; j0 < d; j0 += kNfCols) {
    const bool cin = j0 + lc < d;
#pragma unroll 8
    for (int q = 0; q < kNfRows / (kNfRows / kNfCols); ++q) {
      const int rr = q * (kNfRows / kNfCols) + lr;
      const int64_t r = rbase + rr;
      xt[rr * (kNfCols + 1) + lc] = (cin && r < n) ? x[r * x_row_stride + j0 + lc] : 0.0f;
    }
    for (int idx = tid; idx < kNfCols * KP; idx += kNfRows) {
      const int jj = idx / KP, t = idx % KP;
      bs[idx] = (j0 + jj < d && t < k) ? bt[(int64_t)(j0 + jj) * k + t] : 0.0;
    }
    __syncthreads();
#pragma unroll 4
    for (int jj = 0; jj < kNfCols; ++jj) {
      const double xv = (double)xt[tid * (kNfCols + 1) + jj];
#pragma unroll
      for (int t = 0; t < KP; ++t) acc[t] = fma(xv, bs[jj * KP + t], acc[t]);
    }
    __syncthreads();
  }
  if (MODE == 1) {
    if (live) {
#pragma unroll
      for (int t = 0; t < KP; ++t)
        if (t < k) a[row * k + t] = acc[t] / aux[t];
    }
    return;
  }
  nf_load_gram<KP>(aux, k, gs);                               // (the loop's last barrier lies behind every read of the tiles)
  double w[KP];
#pragma unroll
  for (int t = 0; t < KP; ++t) w[t] = (live && t < k) ? a[row * k + t] : 0.0;
  __syncthreads();
  double viol = nf_sweep<KP>(acc, w, gs, k);
  if (live) {
#pragma unroll
    for (int t = 0; t < KP; ++t)
      if (t < k) a[row * k + t] = w[t];
  }
  viol = block_sum(live ? viol : 0.0, red);
  if (tid == 0) vpart[blockIdx.x] = viol;
}

// ---------------------------------------------------------------------------------------------------------------- column side
// partial[run][col][t] = sum over the run's rows r, rising, of x[r][col] w[r][t]
template <int KP>
__global__ __launch_bounds__(256) void nmf_xtw_kernel(const float* __restrict__ x, int64_t x_row_stride, int64_t n, int32_t d, int32_t k,
                                                      const double* __restrict__ w, int64_t rows_per_run, double* __restrict__ partial,
                                                      const int32_t* __restrict__ done) {
  constexpr int KPT = KP / 4;
  __shared__ double ws[kNfXtRows * KP];
  if (done && *done) return;
  const int tid = threadIdx.x, lane = tid & 63, kg = tid >> 6;
  const int col = blockIdx.x * kNfXtCols + lane;
  const bool cin = col < d;
  const int run = blockIdx.y;
  const int64_t rbeg = (int64_t)run * rows_per_run;
  const int64_t rend = rbeg + rows_per_run < n ? rbeg + rows_per_run : n;
  double acc[KPT];
#pragma unroll
  for (int q = 0; q < KPT; ++q) acc[q] = 0.0;
  for (int64_t rb = rbeg; rb < rend; rb += kNfXtRows) {
    for (int idx = tid; idx < kNfXtRows * KP; idx += 256) {
      const int rr = idx / KP, t = idx % KP;
      ws[idx] = (rb + rr < rend && t < k) ? w[(rb + rr) * k + t] : 0.0;
    }
    __syncthreads();
#pragma unroll 8
    for (int rr = 0; rr < kNfXtRows; ++rr) {
      const double xv = (cin && rb + rr < rend) ? (double)x[(rb + rr) * x_row_stride + col] : 0.0;
#pragma unroll
      for (int q = 0; q < KPT; ++q) acc[q] = fma(xv, ws[rr * KP + kg * KPT + q], acc[q]);
    }
    __syncthreads();
  }
  if (cin) {
#pragma unroll
    for (int q = 0; q < KPT; ++q) {
      const int t = kg * KPT + q;
      if (t < k) partial[((int64_t)run * d + col) * k + t] = acc[q];
    }
  }
}

// the H half-sweep: one lane per row j of H^T, whose row of X^T W is the runs' partial rows added in rising run order
template <int KP>
__global__ __launch_bounds__(kNfRows) void nmf_cols_kernel(const double* __restrict__ partial, int32_t runs, int32_t d, int32_t k,
                                                           const double* __restrict__ gram, double* __restrict__ ht, double* __restrict__ vpart,
                                                           const int32_t* __restrict__ done) {
  __shared__ double gs[KP * KP];
  __shared__ double red[kNfRows / 64];
  if (done && *done) return;
  const int tid = threadIdx.x;
  const int j = blockIdx.x * kNfRows + tid;
  const bool live = j < d;
  nf_load_gram<KP>(gram, k, gs);
  double acc[KP], h[KP];
#pragma unroll
  for (int t = 0; t < KP; ++t) {
    acc[t] = 0.0;
    h[t] = (live && t < k) ? ht[(int64_t)j * k + t] : 0.0;
  }
  if (live) {
    for (int r = 0; r < runs; ++r) {
      const double* p = partial + ((int64_t)r * d + j) * k;
#pragma unroll
      for (int t = 0; t < KP; ++t)
        if (t < k) acc[t] += p[t];
    }
  }
  __syncthreads();
  double viol = nf_sweep<KP>(acc, h, gs, k);
  if (live) {
#pragma unroll
    for (int t = 0; t < KP; ++t)
      if (t < k) ht[(int64_t)j * k + t] = h[t];
  }
  viol = block_sum(live ? viol : 0.0, red);
  if (tid == 0) vpart[blockIdx.x] = viol;
}

// ---------------------------------------------------------------------------------------------------------------- Gram
// partial[run][t][r] = sum over the run's rows i, rising, of a[i][t] a[i][r];  a (m, k) contiguous
__global__ __launch_bounds__(256) void nmf_gram_kernel(const double* __restrict__ a, int64_t m, int32_t k, int64_t rows_per_run,
                                                       double* __restrict__ partial, const int32_t* __restrict__ done) {
  __shared__ double as[kNfGramRows * MMK_NMF_MAX_COMPONENTS];
  if (done && *done) return;
  const int tid = threadIdx.x, kk = k * k;
  const int64_t rbeg = (int64_t)blockIdx.x * rows_per_run;
  const int64_t rend = rbeg + rows_per_run < m ? rbeg + rows_per_run : m;
  constexpr int E = MMK_NMF_MAX_COMPONENTS * MMK_NMF_MAX_COMPONENTS / 256;
  double acc[E];
  int ta[E], ra[E];
#pragma unroll
  for (int q = 0; q < E; ++q) {
    const int e = tid + q * 256;
    acc[q] = 0.0;
    ta[q] = e < kk ? e / k : 0;
    ra[q] = e < kk ? e % k : 0;
  }
  for (int64_t rb = rbeg; rb < rend; rb += kNfGramRows) {
    const int rows = (int)(rend - rb < kNfGramRows ? rend - rb : kNfGramRows);
    for (int idx = tid; idx < rows * k; idx += 256) as[idx] = a[rb * k + idx];
    __syncthreads();
    for (int rr = 0; rr < rows; ++rr) {
#pragma unroll
      for (int q = 0; q < E; ++q)
        if (tid + q * 256 < kk) acc[q] = fma(as[rr * k + ta[q]], as[rr * k + ra[q]], acc[q]);
    }
    __syncthreads();
  }
#pragma unroll
  for (int q = 0; q < E; ++q)
    if (tid + q * 256 < kk) partial[(int64_t)blockIdx.x * kk + tid + q * 256] = acc[q];
}

__global__ __launch_bounds__(256) void nmf_gram_reduce_kernel(const double* __restrict__ partial, int32_t runs, int32_t kk, double* __restrict__ gram,
                                                              const int32_t* __restrict__ done) {
  if (done && *done) return;
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= kk) return;
  double acc = 0.0;
  for (int r = 0; r < runs; ++r) acc += partial[(int64_t)r * kk + e];
  gram[e] = acc;
}

// ---------------------------------------------------------------------------------------------------------------- violation and the flag
// one wave: lane l adds the entries l, l + 64, ... in rising order, then the wave tree.  stat: [0] the first iteration's violation, [1] the
// last one's;  *done = the iteration that met the stop rule.  Without a flag (done == nullptr): stat[0] = the sum.
__global__ __launch_bounds__(64) void nmf_check_kernel(const double* __restrict__ vpart, int64_t count, int32_t iter, double tol, double* __restrict__ stat,
                                                       int32_t* __restrict__ done) {
  if (done && *done) return;
  double v = 0.0;
  for (int64_t i = threadIdx.x; i < count; i += 64) v += vpart[i];
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off);
  if (threadIdx.x != 0) return;
  if (!done) {
    stat[0] = v;
    return;
  }
  if (iter == 1) stat[0] = v;
  stat[1] = v;
  const double first = stat[0];
  if (first == 0.0 || v / first <= tol) *done = iter;
}

// ---------------------------------------------------------------------------------------------------------------- the start's pieces
// per chunk of rows: the sum (fp64) and the smallest entry
__global__ __launch_bounds__(256) void nmf_stat_kernel(const float* __restrict__ x, int64_t x_row_stride, int64_t n, int32_t d, int64_t rows_per_chunk,
                                                       double* __restrict__ psum, double* __restrict__ pmin) {
  __shared__ double red[4];
  __shared__ double mn[256];
  const int tid = threadIdx.x;
  const int64_t rbeg = (int64_t)blockIdx.x * rows_per_chunk;
  const int64_t rend = rbeg + rows_per_chunk < n ? rbeg + rows_per_chunk : n;
  double acc = 0.0, lo = INFINITY;
  for (int64_t r = rbeg; r < rend; ++r)
    for (int c = tid; c < d; c += 256) {
      const double v = (double)x[r * x_row_stride + c];
      acc += v;
      lo = v < lo ? v : lo;
    }
  mn[tid] = lo;
  acc = block_sum(acc, red);
  for (int off = 128; off >= 1; off >>= 1) {
    if (tid < off) mn[tid] = mn[tid + off] < mn[tid] ? mn[tid + off] : mn[tid];
    __syncthreads();
  }
  if (tid == 0) {
    psum[blockIdx.x] = acc;
    pmin[blockIdx.x] = mn[0];
  }
}

// stat[0] = mean(x), stat[1] = min(x)
__global__ __launch_bounds__(64) void nmf_stat_fin_kernel(const double* __restrict__ psum, const double* __restrict__ pmin, int32_t chunks, double count,
                                                          double* __restrict__ stat) {
  double v = 0.0, lo = INFINITY;
  for (int i = threadIdx.x; i < chunks; i += 64) {
    v += psum[i];
    lo = pmin[i] < lo ? pmin[i] : lo;
  }
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    v += __shfl_xor(v, off);
    const double o = __shfl_xor(lo, off);
    lo = o < lo ? o : lo;
  }
  if (threadIdx.x == 0) {
    stat[0] = v / count;
    stat[1] = lo;
  }
}

__global__ __launch_bounds__(256) void nmf_fill_kernel(double* __restrict__ p, int32_t count, double v) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < count) p[i] = v;
}

// vt (d, k) = v^T;  s[t] = sqrt(variance[t] (n - 1)): the covariance kernel divided the Gram matrix by n - 1
__global__ __launch_bounds__(256) void nmf_vt_kernel(const double* __restrict__ v, const double* __restrict__ variance, int32_t d, int32_t k, double nm1,
                                                     double* __restrict__ vt, double* __restrict__ s) {
  const int idx = blockIdx.x * 256 + threadIdx.x;
  if (idx < k) s[idx] = sqrt(variance[idx] * nm1);
  if (idx >= d * k) return;
  const int j = idx / k, t = idx % k;
  vt[idx] = v[(int64_t)t * d + j];
}

// partial[run][0][t] = sum over the run's rows, rising per thread and then the workgroup's tree, of max(a[i][t], 0)^2;  [run][1][t]: of min(a[i][t], 0)^2
__global__ __launch_bounds__(256) void nmf_partnorm_kernel(const double* __restrict__ a, int64_t m, int32_t k, int64_t rows_per_run,
                                                           double* __restrict__ partial) {
  __shared__ double red[4];
  const int tid = threadIdx.x;
  const int64_t rbeg = (int64_t)blockIdx.x * rows_per_run;
  const int64_t rend = rbeg + rows_per_run < m ? rbeg + rows_per_run : m;
  for (int t = 0; t < k; ++t) {
    double sp = 0.0, sn = 0.0;
    for (int64_t r = rbeg + tid; r < rend; r += 256) {
      const double v = a[r * k + t];
      const double p = v > 0.0 ? v : 0.0, q = v < 0.0 ? v : 0.0;
      sp = fma(p, p, sp);
      sn = fma(q, q, sn);
    }
    sp = block_sum(sp, red);
    sn = block_sum(sn, red);
    if (tid == 0) {
      partial[((int64_t)blockIdx.x * 2 + 0) * k + t] = sp;
      partial[((int64_t)blockIdx.x * 2 + 1) * k + t] = sn;
    }
  }
}

// sklearn's choice per column t >= 1: coef[t] = (the u part's norm, the v part's norm, lbd = sqrt(S_t m)), part[t] = 1 for the positive parts
__global__ __launch_bounds__(64) void nmf_choose_kernel(const double* __restrict__ pu, int32_t runs_u, const double* __restrict__ pv, int32_t runs_v,
                                                        const double* __restrict__ s, int32_t k, double* __restrict__ coef, int32_t* __restrict__ part) {
  const int t = threadIdx.x;
  if (t >= k) return;
  if (t == 0) {
    coef[0] = coef[1] = 1.0;
    coef[2] = sqrt(s[0]);
    part[0] = 2;
    return;
  }
  double up = 0.0, un = 0.0, vp = 0.0, vn = 0.0;
  for (int r = 0; r < runs_u; ++r) {
    up += pu[((int64_t)r * 2 + 0) * k + t];
    un += pu[((int64_t)r * 2 + 1) * k + t];
  }
  for (int r = 0; r < runs_v; ++r) {
    vp += pv[((int64_t)r * 2 + 0) * k + t];
    vn += pv[((int64_t)r * 2 + 1) * k + t];
  }
  const double xp = sqrt(up), xn = sqrt(un), yp = sqrt(vp), yn = sqrt(vn);
  const double mp = xp * yp, mn = xn * yn;
  const bool pos = mp > mn;                                  // strictly, as sklearn
  coef[3 * t + 0] = pos ? xp : xn;
  coef[3 * t + 1] = pos ? yp : yn;
  coef[3 * t + 2] = sqrt(s[t] * (pos ? mp : mn));
  part[t] = pos ? 1 : 0;
}

// a (m, k) in place: the chosen part, normalised and scaled; entries < 1e-6 become 0, zeros become avg.  which: 0 = the u side, 1 = the v side
__global__ __launch_bounds__(256) void nmf_init_kernel(double* __restrict__ a, int64_t m, int32_t k, int32_t which, const double* __restrict__ coef,
                                                       const int32_t* __restrict__ part, const double* __restrict__ stat) {
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= m * k) return;
  const int t = (int)(idx % k);
  const double v = a[idx], lbd = coef[3 * t + 2];
  double out;
  if (t == 0) {
    out = lbd * fabs(v);
  } else {
    const double p = part[t] ? (v > 0.0 ? v : 0.0) : fabs(v < 0.0 ? v : 0.0);
    out = lbd * (p / coef[3 * t + which]);
  }
  if (out < MMK_NMF_EPS) out = 0.0;
  if (out == 0.0) out = stat[0];
  a[idx] = out;
}

#define NF_DISPATCH(kp, ...)                                      \
  switch (kp) {                                                   \
    case 4: { constexpr int KP = 4; __VA_ARGS__; } break;         \
    case 8: { constexpr int KP = 8; __VA_ARGS__; } break;         \
    case 16: { constexpr int KP = 16; __VA_ARGS__; } break;       \
    case 32: { constexpr int KP = 32; __VA_ARGS__; } break;       \
    default: { constexpr int KP = 64; __VA_ARGS__; } break;       \
  }

// the workspace of a half-sweep, in doubles: gram (k k), gram partials, X^T W partials, the workgroups' violations
struct NfHalfWs {
  double *gram, *gpart, *xpart, *vpart;
  size_t doubles;
};
static NfHalfWs nf_half_ws(void* workspace, const NfPlan& p, int32_t d, int32_t k) {
  NfHalfWs w;
  const size_t kk = (size_t)k * k;
  const size_t gruns = (size_t)(p.gruns_n > p.gruns_d ? p.gruns_n : p.gruns_d);
  w.gram = static_cast<double*>(workspace);
  w.gpart = w.gram + kk;
  w.xpart = w.gpart + gruns * kk;
  w.vpart = w.xpart + (size_t)p.runs * d * k;
  w.doubles = kk + gruns * kk + (size_t)p.runs * d * k + (size_t)(p.nbw + p.nbh);
  return w;
}

static int nf_gram(const double* a, int64_t m, int32_t k, int runs, int64_t rows, const NfHalfWs& ws, const int32_t* done, hipStream_t st) {
  MMK_TRY(launch(nmf_gram_kernel, dim3((unsigned)runs), dim3(256), 0, st, a, m, k, rows, ws.gpart, done));
  return launch(nmf_gram_reduce_kernel, dim3((unsigned)((k * k + 255) / 256)), dim3(256), 0, st, ws.gpart, runs, k * k, ws.gram, done);
}

// the W half: H H^T, then the row kernel; the workgroups' violations go to ws.vpart[0 .. nbw)
static int nf_w_half(const float* x, int64_t xs, int64_t n, int32_t d, int32_t k, const double* ht, double* w, const NfPlan& p, const NfHalfWs& ws,
                     const int32_t* done, hipStream_t st) {
  MMK_TRY(nf_gram(ht, d, k, p.gruns_d, p.grows_d, ws, done, st));
  NF_DISPATCH(p.kp, return launch(nmf_rows_kernel<KP, 0>, dim3((unsigned)p.nbw), dim3(kNfRows), 0, st, x, xs, n, d, k, ht,
                                  (const double*)ws.gram, w, ws.vpart, done));
}

// the H half: W^T W, the runs' X^T W, then the sweep over the rows of H^T; violations to ws.vpart[nbw .. nbw + nbh)
static int nf_h_half(const float* x, int64_t xs, int64_t n, int32_t d, int32_t k, const double* w, double* ht, const NfPlan& p, const NfHalfWs& ws,
                     const int32_t* done, hipStream_t st) {
  MMK_TRY(nf_gram(w, n, k, p.gruns_n, p.grows_n, ws, done, st));
  const dim3 grid((unsigned)((d + kNfXtCols - 1) / kNfXtCols), (unsigned)p.runs);
  NF_DISPATCH(p.kp, MMK_TRY(launch(nmf_xtw_kernel<KP>, grid, dim3(256), 0, st, x, xs, n, d, k, w, p.rows_per_run, ws.xpart, done)));
  NF_DISPATCH(p.kp, return launch(nmf_cols_kernel<KP>, dim3((unsigned)p.nbh), dim3(kNfRows), 0, st, (const double*)ws.xpart, p.runs, d, k,
                                  (const double*)ws.gram, ht, ws.vpart + p.nbw, done));
}

static int nf_stats(const float* x, int64_t xs, int64_t n, int32_t d, const NfPlan& p, double* psum, double* stat, hipStream_t st) {
  MMK_TRY(launch(nmf_stat_kernel, dim3((unsigned)p.chunks), dim3(256), 0, st, x, xs, n, d, p.rows_per_chunk, psum, psum + p.chunks));
  return launch(nmf_stat_fin_kernel, dim3(1), dim3(64), 0, st, (const double*)psum, (const double*)(psum + p.chunks), p.chunks,
                (double)n * (double)d, stat);
}

// start: n_components <= min(n, d), the condition of sklearn's NNDSVDA start; the sweeps take any 1 <= n_components <= the limit (a transform
// of fewer rows than components is one)
static int nf_check_shape(const char* who, int64_t n, int32_t d, int32_t k, bool start = false) {
  if (n < 1 || d < 1) return fail(MMK_ERR_INVALID, "%s: n = %lld rows, d = %d columns (both at least 1)", who, (long long)n, d);
  if (d > MMK_NMF_MAX_D) return fail(MMK_ERR_UNSUPPORTED, "%s: d = %d columns, the limit is %d (MMK_NMF_MAX_D)", who, d, MMK_NMF_MAX_D);
  if (k > MMK_NMF_MAX_COMPONENTS)
    return fail(MMK_ERR_UNSUPPORTED, "%s: n_components = %d, the limit is %d (MMK_NMF_MAX_COMPONENTS: a row of W lives in one lane's registers)", who, k,
                MMK_NMF_MAX_COMPONENTS);
  if (k < 1) return fail(MMK_ERR_INVALID, "%s: n_components = %d must be at least 1", who, k);
  if (start && (k > d || k > n))
    return fail(MMK_ERR_INVALID, "%s: n_components = %d must lie in [1, min(n, d) = %lld]", who, k, (long long)(n < d ? n : d));
  if ((n + kNfRows - 1) / kNfRows > 0x7fffffffLL) return fail(MMK_ERR_UNSUPPORTED, "%s: %lld rows are more than one launch takes", who, (long long)n);
  return MMK_OK;
}

static bool nf_shape_ok(int64_t n, int32_t d, int32_t k, bool start = false) {
  return n >= 1 && d >= 1 && d <= MMK_NMF_MAX_D && k >= 1 && k <= MMK_NMF_MAX_COMPONENTS && (!start || (k <= d && k <= n)) &&
         (n + kNfRows - 1) / kNfRows <= 0x7fffffffLL;
}

// the start's workspace, in doubles
struct NfStartWs {
  double *zeros, *ones, *c, *variance, *psum, *stat, *ppart, *coef;
  void *cov_ws, *eig_ws;
  size_t cov_bytes, eig_bytes, doubles;
};
static NfStartWs nf_start_ws(void* workspace, const NfPlan& p, int64_t n, int32_t d, int32_t k) {
  NfStartWs w;
  w.cov_bytes = mmk_pca_cov_workspace_bytes(n, d);
  w.eig_bytes = mmk_pca_eig_workspace_bytes(d, k);
  double* at = static_cast<double*>(workspace);
  w.zeros = at;
  at += d;
  w.ones = at;
  at += d;
  w.c = at;
  at += (size_t)d * d;
  w.variance = at;
  at += k;
  w.psum = at;
  at += 2 * (size_t)p.chunks;
  w.stat = at;
  at += 2;
  w.ppart = at;
  at += 2 * (size_t)k * (size_t)(p.gruns_n + p.gruns_d);
  w.coef = at;
  at += 3 * (size_t)k;
  w.cov_ws = at;
  at += w.cov_bytes / sizeof(double);
  w.eig_ws = at;
  at += w.eig_bytes / sizeof(double);
  w.doubles = (size_t)(at - static_cast<double*>(workspace));
  return w;
}

}  // namespace mmk

// ---------------------------------------------------------------------------------------------------------------- entry points
extern "C" size_t mmk_nmf_start_workspace_bytes(int64_t n, int32_t d, int32_t k) {
  using namespace mmk;
  if (!nf_shape_ok(n, d, k, true) || n < 2) return 0;
  return nf_start_ws(nullptr, nf_plan(n, d, k), n, d, k).doubles * sizeof(double);
}

extern "C" int mmk_nmf_start_f64(const float* x, int64_t x_row_stride, int64_t n, int32_t d, int32_t k, double* w, double* ht, double* s, double* v,
                                 int32_t* part, void* workspace, size_t workspace_bytes, mmk_stream_t stream) {
  using namespace mmk;
  MMK_TRY(nf_check_shape("nmf_start", n, d, k, true));
  if (n < 2) return fail(MMK_ERR_INVALID, "nmf_start: n = %lld rows, at least 2 are needed (the Gram matrix comes from the covariance kernel)", (long long)n);
  if (!x || !w || !ht || !s || !v || !part || !workspace || x_row_stride < 0)
    return fail(MMK_ERR_INVALID, "nmf_start: bad arguments (null pointer or negative stride %lld)", (long long)x_row_stride);
  if (misaligned(x, 4) || misaligned(part, 4) || misaligned(w, 8) || misaligned(ht, 8) || misaligned(s, 8) || misaligned(v, 8) ||
      misaligned(workspace, 8))
    return fail(MMK_ERR_INVALID, "nmf_start: x and part must be 4-byte aligned, w, ht, s, v and the workspace 8-byte aligned");
  MMK_TRY(workspace_check("nmf_start", workspace, 8, workspace_bytes, mmk_nmf_start_workspace_bytes(n, d, k)));
  hipStream_t st = (hipStream_t)stream;
  const NfPlan p = nf_plan(n, d, k);
  const NfStartWs ws = nf_start_ws(workspace, p, n, d, k);
  MMK_TRY(nf_stats(x, x_row_stride, n, d, p, ws.psum, ws.stat, st));
  MMK_TRY(launch(nmf_fill_kernel, dim3((unsigned)((d + 255) / 256)), dim3(256), 0, st, ws.zeros, d, 0.0));
  MMK_TRY(launch(nmf_fill_kernel, dim3((unsigned)((d + 255) / 256)), dim3(256), 0, st, ws.ones, d, 1.0));
  MMK_TRY(mmk_pca_cov_f64(x, x_row_stride, n, d, ws.zeros, ws.ones, ws.c, ws.cov_ws, ws.cov_bytes, stream));
  int32_t eig_iter = 0;
  MMK_TRY(mmk_pca_eig_f64(ws.c, d, k, 0, v, ws.variance, &eig_iter, ws.eig_ws, ws.eig_bytes, stream));
  double host[MMK_NMF_MAX_COMPONENTS + 2];
  MMK_HIP(hipMemcpyAsync(host, ws.variance, (size_t)k * sizeof(double), hipMemcpyDeviceToHost, st));
  MMK_HIP(hipMemcpyAsync(host + k, ws.stat, 2 * sizeof(double), hipMemcpyDeviceToHost, st));
  MMK_HIP(hipStreamSynchronize(st));
  if (host[k + 1] < 0.0) return fail(MMK_ERR_INVALID, "nmf_start: negative values in the frames (the smallest is %g)", host[k + 1]);
  const double nm1 = (double)(n - 1);
  const double lam0 = host[0] * nm1, lamk = host[k - 1] * nm1;
  const double thr = MMK_NMF_RANK_MARGIN * ((double)(n + 2) * 1.1102230246251565e-16 + MMK_PCA_TOL * sqrt((double)d)) * lam0;
  if (!(lamk > thr))
    return fail(MMK_ERR_INVALID,
                "nmf_start: n_components = %d exceeds the numerical rank of the frames: eigenvalue %d of X^T X is %.3e, not above %.3e "
                "(= %.0f ((n + 2) 2^-53 + %.0e sqrt(d)) times the largest, %.3e); the reference's start is arbitrary there",
                k, k - 1, lamk, thr, MMK_NMF_RANK_MARGIN, MMK_PCA_TOL, lam0);
  MMK_TRY(launch(nmf_vt_kernel, dim3((unsigned)((d * k + 255) / 256)), dim3(256), 0, st, (const double*)v, (const double*)ws.variance, d, k, nm1, ht, s));
  NF_DISPATCH(p.kp, MMK_TRY(launch(nmf_rows_kernel<KP, 1>, dim3((unsigned)p.nbw), dim3(kNfRows), 0, st, x, x_row_stride, n, d, k,
                                   (const double*)ht, (const double*)s, w, (double*)nullptr, (const int32_t*)nullptr)));
  double* pu = ws.ppart;
  double* pv = ws.ppart + 2 * (size_t)k * p.gruns_n;
  MMK_TRY(launch(nmf_partnorm_kernel, dim3((unsigned)p.gruns_n), dim3(256), 0, st, (const double*)w, n, k, p.grows_n, pu));
  MMK_TRY(launch(nmf_partnorm_kernel, dim3((unsigned)p.gruns_d), dim3(256), 0, st, (const double*)ht, (int64_t)d, k, p.grows_d, pv));
  MMK_TRY(launch(nmf_choose_kernel, dim3(1), dim3(64), 0, st, (const double*)pu, p.gruns_n, (const double*)pv, p.gruns_d, (const double*)s, k, ws.coef,
                 part));
  MMK_TRY(launch(nmf_init_kernel, dim3((unsigned)((n * k + 255) / 256)), dim3(256), 0, st, w, n, k, 0, (const double*)ws.coef, (const int32_t*)part,
                 (const double*)ws.stat));
  return launch(nmf_init_kernel, dim3((unsigned)(((int64_t)d * k + 255) / 256)), dim3(256), 0, st, ht, (int64_t)d, k, 1, (const double*)ws.coef,
                (const int32_t*)part, (const double*)ws.stat);
}

extern "C" size_t mmk_nmf_half_workspace_bytes(int64_t n, int32_t d, int32_t k) {
  using namespace mmk;
  if (!nf_shape_ok(n, d, k)) return 0;
  return nf_half_ws(nullptr, nf_plan(n, d, k), d, k).doubles * sizeof(double);
}

static int nf_half_args(const char* who, const float* x, int64_t x_row_stride, int64_t n, int32_t d, int32_t k, const void* a, const void* b,
                        const void* violation, const void* workspace, size_t workspace_bytes, size_t need) {
  using namespace mmk;
  MMK_TRY(nf_check_shape(who, n, d, k));
  if (!x || !a || !b || !violation || !workspace || x_row_stride < 0)
    return fail(MMK_ERR_INVALID, "%s: bad arguments (null pointer or negative stride %lld)", who, (long long)x_row_stride);
  if (misaligned(x, 4) || misaligned(a, 8) || misaligned(b, 8) || misaligned(violation, 8) || misaligned(workspace, 8))
    return fail(MMK_ERR_INVALID, "%s: x must be 4-byte aligned, w, ht, violation and the workspace 8-byte aligned", who);
  return workspace_check(who, workspace, 8, workspace_bytes, need);
}

extern "C" int mmk_nmf_w_half_f64(const float* x, int64_t x_row_stride, int64_t n, int32_t d, int32_t k, const double* ht, double* w, double* violation,
                                  void* workspace, size_t workspace_bytes, mmk_stream_t stream) {
  using namespace mmk;
  MMK_TRY(nf_half_args("nmf_w_half", x, x_row_stride, n, d, k, ht, w, violation, workspace, workspace_bytes, mmk_nmf_half_workspace_bytes(n, d, k)));
  hipStream_t st = (hipStream_t)stream;
  const NfPlan p = nf_plan(n, d, k);
  const NfHalfWs ws = nf_half_ws(workspace, p, d, k);
  MMK_TRY(nf_w_half(x, x_row_stride, n, d, k, ht, w, p, ws, nullptr, st));
  return launch(nmf_check_kernel, dim3(1), dim3(64), 0, st, (const double*)ws.vpart, p.nbw, 0, 0.0, violation, (int32_t*)nullptr);
}

extern "C" int mmk_nmf_h_half_f64(const float* x, int64_t x_row_stride, int64_t n, int32_t d, int32_t k, const double* w, double* ht, double* violation,
                                  void* workspace, size_t workspace_bytes, mmk_stream_t stream) {
  using namespace mmk;
  MMK_TRY(nf_half_args("nmf_h_half", x, x_row_stride, n, d, k, w, ht, violation, workspace, workspace_bytes, mmk_nmf_half_workspace_bytes(n, d, k)));
  hipStream_t st = (hipStream_t)stream;
  const NfPlan p = nf_plan(n, d, k);
  const NfHalfWs ws = nf_half_ws(workspace, p, d, k);
  MMK_TRY(nf_h_half(x, x_row_stride, n, d, k, w, ht, p, ws, nullptr, st));
  return launch(nmf_check_kernel, dim3(1), dim3(64), 0, st, (const double*)(ws.vpart + p.nbw), p.nbh, 0, 0.0, violation, (int32_t*)nullptr);
}

extern "C" size_t mmk_nmf_solve_workspace_bytes(int64_t n, int32_t d, int32_t k) {
  using namespace mmk;
  if (!nf_shape_ok(n, d, k)) return 0;
  const NfPlan p = nf_plan(n, d, k);
  return (nf_half_ws(nullptr, p, d, k).doubles + 2 * (size_t)p.chunks + 6) * sizeof(double);
}

extern "C" int mmk_nmf_solve_f64(const float* x, int64_t x_row_stride, int64_t n, int32_t d, int32_t k, double* w, double* ht, int32_t update_h, double tol,
                                 int32_t max_iter, int32_t poll, int32_t check_nonneg, int32_t* n_iter, void* workspace, size_t workspace_bytes,
                                 mmk_stream_t stream) {
  using namespace mmk;
  MMK_TRY(nf_half_args("nmf_solve", x, x_row_stride, n, d, k, w, ht, workspace, workspace, workspace_bytes, mmk_nmf_solve_workspace_bytes(n, d, k)));
  if (!n_iter) return fail(MMK_ERR_INVALID, "nmf_solve: bad arguments (n_iter is null)");
  if (max_iter < 1 || poll < 0 || !(tol >= 0.0))
    return fail(MMK_ERR_INVALID, "nmf_solve: max_iter = %d (at least 1), poll = %d (0: %d), tol = %g (0 or above)", max_iter, poll, MMK_NMF_POLL, tol);
  hipStream_t st = (hipStream_t)stream;
  const NfPlan p = nf_plan(n, d, k);
  const NfHalfWs ws = nf_half_ws(workspace, p, d, k);
  double* psum = static_cast<double*>(workspace) + ws.doubles;
  double* stat = psum + 2 * (size_t)p.chunks;            // the first violation, the last, the flag, then mean and min of x
  int32_t* done = reinterpret_cast<int32_t*>(stat + 2);
  const int every = poll > 0 ? poll : MMK_NMF_POLL;
  struct {
    double first, last;
    int32_t done, pad;
    double mean, min;
  } host = {0.0, 0.0, 0, 0, 0.0, 0.0};
  static_assert(sizeof(host) == 5 * sizeof(double), "the flag block is five doubles");
  MMK_HIP(hipMemsetAsync(stat, 0, 5 * sizeof(double), st));
  if (check_nonneg) MMK_TRY(nf_stats(x, x_row_stride, n, d, p, psum, stat + 3, st));
  int it = 0;
  while (it < max_iter && !host.done) {
    ++it;
    MMK_TRY(nf_w_half(x, x_row_stride, n, d, k, ht, w, p, ws, done, st));
    if (update_h) MMK_TRY(nf_h_half(x, x_row_stride, n, d, k, w, ht, p, ws, done, st));
    MMK_TRY(launch(nmf_check_kernel, dim3(1), dim3(64), 0, st, (const double*)ws.vpart, update_h ? p.nbw + p.nbh : p.nbw, it, tol, stat, done));
    if (it % every == 0 || it == max_iter) {
      MMK_HIP(hipMemcpyAsync(&host, stat, sizeof(host), hipMemcpyDeviceToHost, st));
      MMK_HIP(hipStreamSynchronize(st));
      if (check_nonneg && host.min < 0.0) return fail(MMK_ERR_INVALID, "nmf_solve: negative values in the frames (the smallest is %g)", host.min);
      if (host.last != host.last) break;                 // NaN: no later iteration mends it
    }
  }
  *n_iter = host.done ? host.done : max_iter;
  return MMK_OK;
}
