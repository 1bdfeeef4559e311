// Principal components of corpus frames (mimikit/features/functionals.py:1114-1138 PCA = sklearn's StandardScaler, then sklearn's PCA).  Everything is
// fp64 inside; the frames and the scores are fp32.  Four entry points, no atomics, every sum in one fixed order: two calls give the same bits.
//
//   column statistics     three passes over the rows, each a launch of per-chunk partial sums (a chunk is a fixed run of rows: the partials
//                         of 64 columns by one workgroup) and a launch that adds the chunks' partials in rising order:
//                         mu = sum x / N;  var = sum (x - mu)^2 / N, scale = 1 where var <= N eps var + (N mu eps)^2 (sklearn's
//                         _is_constant_feature) and sqrt(var) elsewhere;  m = sum ((x - mu) / scale) / N, the mean that sklearn's PCA
//                         subtracts again, folded into the mean that leaves: mean = mu + m scale.
//   covariance            C = Z^T Z / (N - 1), Z = (x - mean) / scale formed while a tile is loaded and never written.  A workgroup owns one
//                         64 x 64 block of the lower block triangle and one run of rows; its four waves hold 2 x 2 products of
//                         v_mfma_f64_16x16x4_f64 each (C/D: col = lane & 15, row = (lane >> 4) + 4 reg).  The runs' partial blocks go to the
//                         workspace and a second launch adds them in rising run order, divides once and writes C[i][j] and C[j][i] from the
//                         one value computed for j <= i.
//   top-k eigenpairs      block subspace iteration with a Rayleigh-Ritz step on a block of b = min(D, k + 16) columns:
//                             Q' = orth(Y)   Householder QR in one workgroup - reflectors, not a Cholesky of Y^T Y: Q' is orthonormal whatever
//                                            the rank of Y (a zero column leaves its reflector the identity)
//                             Z = C Q'       v_mfma_f64_16x16x4_f64, C read through its mirror so that both operands are coalesced
//                             H = Q'^T Z     W, theta = eig(H): cyclic Jacobi in one workgroup, H in LDS, round-robin pairs (b / 2
//                                            rotations at a time), eigenvalues sorted falling
//                             Q = Q' W, Y = Z W (= C Q up to rounding), res_k = |Y_k - theta_k Q_k|_2
//                         until max_k res_k <= kPcTol |C|_inf over the first k columns.  The start block is a counter-based hash.  A device
//                         flag holds the iteration that converged; every kernel of a later iteration returns at once when it is set, and the
//                         host reads the flag every kPcPoll iterations - the result does not depend on when the host looks.
//                         At the end each vector's sign makes its entry of largest magnitude (the first of equals) positive.
//   projection            scores = ((y - mean) / scale) components^T, per (row, component) one fp64 fma chain over rising column, rounded to
//                         fp32 once.
//
// The QR, H, Jacobi, rotation, residual and finish kernels of the eigen step live in subspace_eig.h, which factor_analysis.hip shares; the
// product C Q', |C|_inf and the stop test are this file's.
#include "subspace_eig.h"

namespace mmk {

constexpr int kPcExtra = 16;            // guard columns of the block beyond n_components
static_assert(kPcExtra == kPcGuard, "pc_block and the Jacobi kernel's LDS (subspace_eig.h) are sized by kPcGuard");
constexpr int kStChunks = 1024;         // most row chunks of the column statistics
constexpr int kStMinRows = 256;
constexpr int kCvTile = 64;
constexpr int kCvRows = 16;             // rows per LDS chunk
constexpr int kCvPitch = 68;
constexpr int kCvMinRows = 256;         // fewest rows of a run
constexpr int kCvTargetGroups = 1024;   // workgroups asked for across blocks and runs
constexpr int kPjRows = 16;
constexpr int kPjCols = 64;

// ---------------------------------------------------------------------------------------------------------------- column statistics
static int st_chunks(int64_t n) {
  const int64_t c = (n + kStMinRows - 1) / kStMinRows;
  return (int)(c < kStChunks ? c : kStChunks);
}

// MODE 0: x;  1: (x - a)^2;  2: (x - a) / s
template <int MODE>
__global__ __launch_bounds__(256) void pca_colsum_kernel(const float* __restrict__ x, int64_t x_row_stride, int64_t n, int32_t d,
                                                         const double* __restrict__ a, const double* __restrict__ s, int64_t rows_per_chunk,
                                                         double* __restrict__ partial) {
  __shared__ double red[4][64];
  const int col = blockIdx.x * 64 + (threadIdx.x & 63), rl = threadIdx.x >> 6;
  const int64_t rbeg = (int64_t)blockIdx.y * rows_per_chunk;
  const int64_t rend = rbeg + rows_per_chunk < n ? rbeg + rows_per_chunk : n;
  double acc = 0.0;
  if (col < d) {
    const double av = MODE > 0 ? a[col] : 0.0, sv = MODE == 2 ? s[col] : 1.0;
    for (int64_t r = rbeg + rl; r < rend; r += 4) {
      const double v = (double)x[r * x_row_stride + col];
      if (MODE == 0) acc += v;
      if (MODE == 1) acc = fma(v - av, v - av, acc);
      if (MODE == 2) acc += (v - av) / sv;
    }
  }
  red[rl][threadIdx.x & 63] = acc;
  __syncthreads();
  if (rl == 0 && col < d) partial[(int64_t)blockIdx.y * d + col] = ((red[0][threadIdx.x] + red[1][threadIdx.x]) + red[2][threadIdx.x]) + red[3][threadIdx.x];
}

template <int MODE>
__global__ __launch_bounds__(256) void pca_colfin_kernel(const double* __restrict__ partial, int32_t chunks, int64_t n, int32_t d,
                                                         double* __restrict__ mu, double* __restrict__ scale, double* __restrict__ mean) {
  const int col = blockIdx.x * 256 + threadIdx.x;
  if (col >= d) return;
  double acc = 0.0;
  for (int c = 0; c < chunks; ++c) acc += partial[(int64_t)c * d + col];
  const double nn = (double)n;
  if (MODE == 0) mu[col] = acc / nn;
  if (MODE == 1) {
    const double var = acc / nn, eps = 2.220446049250313e-16, m = mu[col];
    const double t = nn * m * eps;
    scale[col] = var <= nn * eps * var + t * t ? 1.0 : sqrt(var);
  }
  if (MODE == 2) mean[col] = fma(acc / nn, scale[col], mu[col]);
}

// ---------------------------------------------------------------------------------------------------------------- covariance
__device__ __forceinline__ void cv_pair(int pair, int& bi, int& bj) {
  int i = (int)((sqrt(8.0 * (double)pair + 1.0) - 1.0) * 0.5);
  while ((i + 1) * (i + 2) / 2 <= pair) ++i;
  while (i * (i + 1) / 2 > pair) --i;
  bi = i;
  bj = pair - i * (i + 1) / 2;
}

struct CvPlan {
  int nb, pairs, runs;
  int64_t rows_per_run;
};
static CvPlan cv_plan(int64_t n, int32_t d) {
  CvPlan p;
  p.nb = (d + kCvTile - 1) / kCvTile;
  p.pairs = p.nb * (p.nb + 1) / 2;
  int64_t want = (kCvTargetGroups + p.pairs - 1) / p.pairs;
  const int64_t most = (n + kCvMinRows - 1) / kCvMinRows;
  if (want > most) want = most;
  if (want < 1) want = 1;
  p.rows_per_run = round_up((n + want - 1) / want, kCvRows);
  p.runs = (int)((n + p.rows_per_run - 1) / p.rows_per_run);
  return p;
}

__global__ __launch_bounds__(256) void pca_cov_kernel(const float* __restrict__ x, int64_t x_row_stride, int64_t n, int32_t d,
                                                      const double* __restrict__ mean, const double* __restrict__ scale, int64_t rows_per_run,
                                                      int32_t n_pairs, double* __restrict__ partial) {
  __shared__ double zi[kCvRows * kCvPitch];
  __shared__ double zj[kCvRows * kCvPitch];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave & 1, wn = wave >> 1;
  const int pair = blockIdx.x % n_pairs, run = blockIdx.x / n_pairs;
  int bi, bj;
  cv_pair(pair, bi, bj);
  const int col = tid & 63, r0 = tid >> 6;
  const int ci = bi * kCvTile + col, cj = bj * kCvTile + col;
  const bool ini = ci < d, inj = cj < d;
  const int cic = ini ? ci : d - 1, cjc = inj ? cj : d - 1;
  const double mi = mean[cic], si = scale[cic], mj = mean[cjc], sj = scale[cjc];
  const int64_t rbeg = (int64_t)run * rows_per_run;
  const int64_t rend = rbeg + rows_per_run < n ? rbeg + rows_per_run : n;

  pc_f64x4 acc[2][2];
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < 2; ++b)
#pragma unroll
      for (int q = 0; q < 4; ++q) acc[a][b][q] = 0.0;

  float gi[4], gj[4];
  auto gload = [&](int64_t rb) {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int64_t r = rb + q * 4 + r0;
      const int64_t rc = r < n ? r : n - 1;
      gi[q] = x[rc * x_row_stride + cic];
      gj[q] = x[rc * x_row_stride + cjc];
    }
  };
  if (rbeg < rend) gload(rbeg);
  for (int64_t rb = rbeg; rb < rend; rb += kCvRows) {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const bool ok = rb + q * 4 + r0 < rend;
      zi[(q * 4 + r0) * kCvPitch + col] = (ok && ini) ? ((double)gi[q] - mi) / si : 0.0;
      zj[(q * 4 + r0) * kCvPitch + col] = (ok && inj) ? ((double)gj[q] - mj) / sj : 0.0;
    }
    __syncthreads();
    if (rb + kCvRows < rend) gload(rb + kCvRows);
#pragma unroll
    for (int kk = 0; kk < kCvRows; kk += 4) {
      double av[2], bv[2];
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        av[t] = zi[(kk + (lane >> 4)) * kCvPitch + wm * 32 + t * 16 + (lane & 15)];
        bv[t] = zj[(kk + (lane >> 4)) * kCvPitch + wn * 32 + t * 16 + (lane & 15)];
      }
#pragma unroll
      for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b) acc[a][b] = __builtin_amdgcn_mfma_f64_16x16x4f64(av[a], bv[b], acc[a][b], 0, 0, 0);
    }
    __syncthreads();
  }
  double* out = partial + ((int64_t)run * n_pairs + pair) * (kCvTile * kCvTile);
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < 2; ++b)
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int row = wm * 32 + a * 16 + (lane >> 4) + 4 * q;      // the f64 map: NOT 4 (lane >> 4) + q
        const int cc = wn * 32 + b * 16 + (lane & 15);
        out[row * kCvTile + cc] = acc[a][b][q];
      }
}

__global__ __launch_bounds__(256) void pca_cov_reduce_kernel(const double* __restrict__ partial, int32_t n_pairs, int32_t runs, int32_t d,
                                                             double denom, double* __restrict__ c) {
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int pair = (int)(idx / (kCvTile * kCvTile)), e = (int)(idx % (kCvTile * kCvTile));
  if (pair >= n_pairs) return;
  int bi, bj;
  cv_pair(pair, bi, bj);
  const int i = bi * kCvTile + e / kCvTile, j = bj * kCvTile + e % kCvTile;
  if (i >= d || j >= d || j > i) return;
  double acc = 0.0;
  for (int r = 0; r < runs; ++r) acc += partial[((int64_t)r * n_pairs + pair) * (kCvTile * kCvTile) + e];
  const double v = acc / denom;
  c[(int64_t)i * d + j] = v;
  c[(int64_t)j * d + i] = v;
}

// ---------------------------------------------------------------------------------------------------------------- eigenpairs
// |C|_inf: one workgroup per row, then one thread takes the largest
__global__ __launch_bounds__(256) void pca_rowsum_kernel(const double* __restrict__ c, int32_t d, double* __restrict__ rowsum) {
  __shared__ double red[4];
  double acc = 0.0;
  for (int j = threadIdx.x; j < d; j += 256) acc += fabs(c[(int64_t)blockIdx.x * d + j]);
  acc = block_sum(acc, red);
  if (threadIdx.x == 0) rowsum[blockIdx.x] = acc;
}
__global__ __launch_bounds__(64) void pca_cnorm_kernel(const double* __restrict__ rowsum, int32_t d, double* __restrict__ stat) {
  if (threadIdx.x != 0) return;
  double m = 0.0;
  for (int i = 0; i < d; ++i) m = rowsum[i] > m ? rowsum[i] : m;
  stat[0] = m;
}

// z (d, b) = C qp: a workgroup owns a 16 x 16 tile of z, its four waves a quarter of the sum each, added in rising wave order
__global__ __launch_bounds__(256) void pca_cq_kernel(const double* __restrict__ c, int32_t d, int32_t b, const double* __restrict__ qp,
                                                     double* __restrict__ z, const int32_t* __restrict__ done) {
  __shared__ double red[4][256];
  if (*done) return;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int r0 = blockIdx.x * 16, c0 = blockIdx.y * 16;
  const int kq = ((d + 3) / 4 + 3) & ~3;
  const int kbeg = wave * kq, kend = (wave + 1) * kq < d ? (wave + 1) * kq : d;
  const int row = r0 + (lane & 15), colq = c0 + (lane & 15);
  const int rowc = row < d ? row : d - 1, colc = colq < b ? colq : b - 1;
  pc_f64x4 acc = {0.0, 0.0, 0.0, 0.0};
  for (int k0 = kbeg; k0 < kend; k0 += 4) {
    const int k = k0 + (lane >> 4);
    const int kc = k < d ? k : d - 1;
    const double av = c[(int64_t)kc * d + rowc];     // = C[row][k]: C is mirrored exactly
    const double bv = qp[(int64_t)kc * b + colc];
    const bool kin = k < kend;
    acc = __builtin_amdgcn_mfma_f64_16x16x4f64((kin && row < d) ? av : 0.0, (kin && colq < b) ? bv : 0.0, acc, 0, 0, 0);
  }
#pragma unroll
  for (int q = 0; q < 4; ++q) red[wave][q * 64 + lane] = acc[q];
  __syncthreads();
  if (wave == 0) {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int orow = r0 + (lane >> 4) + 4 * q, ocol = c0 + (lane & 15);
      const double v = ((red[0][q * 64 + lane] + red[1][q * 64 + lane]) + red[2][q * 64 + lane]) + red[3][q * 64 + lane];
      if (orow < d && ocol < b) z[(int64_t)orow * b + ocol] = v;
    }
  }
}

// stat[0] = |C|_inf, stat[1] = the largest residual of the last iteration that ran; *done = that iteration once it meets the stop rule
__global__ __launch_bounds__(64) void pca_check_kernel(int32_t ncomp, int32_t iter, const double* __restrict__ resid, double* __restrict__ stat,
                                                       int32_t* __restrict__ done) {
  if (threadIdx.x != 0 || *done) return;
  double m = 0.0;
  for (int k = 0; k < ncomp; ++k) m = (resid[k] > m || resid[k] != resid[k]) ? resid[k] : m;
  stat[1] = m;
  if (m <= kPcTol * stat[0]) *done = iter;
}

// ---------------------------------------------------------------------------------------------------------------- projection
__global__ __launch_bounds__(256) void pca_project_kernel(const float* __restrict__ y, int64_t y_row_stride, int64_t m, int32_t d,
                                                          const double* __restrict__ mean, const double* __restrict__ scale,
                                                          const double* __restrict__ components, int32_t ncomp, float* __restrict__ out,
                                                          int64_t out_row_stride) {
  __shared__ double zs[kPjRows * (kPjCols + 1)];
  __shared__ double cs[MMK_PCA_MAX_COMPONENTS * (kPjCols + 1)];
  const int tid = threadIdx.x;
  const int col = tid & 63, r4 = tid >> 6;
  const int row = tid & 15, kg = tid >> 4;
  const int64_t rbase = (int64_t)blockIdx.x * kPjRows;
  double acc[4] = {0.0, 0.0, 0.0, 0.0};
  for (int j0 = 0; j0 < d; j0 += kPjCols) {
    const int j = j0 + col;
    const bool jin = j < d;
    const double mj = jin ? mean[j] : 0.0, sj = jin ? scale[j] : 1.0;
#pragma unroll
    for (int q = 0; q < kPjRows / 4; ++q) {
      const int64_t r = rbase + q * 4 + r4;
      zs[(q * 4 + r4) * (kPjCols + 1) + col] = (jin && r < m) ? ((double)y[r * y_row_stride + j] - mj) / sj : 0.0;
    }
    for (int kk = r4; kk < ncomp; kk += 4) cs[kk * (kPjCols + 1) + col] = jin ? components[(int64_t)kk * d + j] : 0.0;
    __syncthreads();
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int k = kg + 16 * q;
      if (k < ncomp) {
        double a = acc[q];
        for (int jj = 0; jj < kPjCols; ++jj) a = fma(zs[row * (kPjCols + 1) + jj], cs[k * (kPjCols + 1) + jj], a);
        acc[q] = a;
      }
    }
    __syncthreads();
  }
  const int64_t r = rbase + row;
  if (r < m) {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int k = kg + 16 * q;
      if (k < ncomp) out[r * out_row_stride + k] = (float)acc[q];
    }
  }
}

}  // namespace mmk

// ---------------------------------------------------------------------------------------------------------------- entry points
extern "C" size_t mmk_pca_colstats_workspace_bytes(int64_t n, int32_t d) {
  using namespace mmk;
  if (n < 1 || d < 1 || d > MMK_PCA_MAX_D) return 0;
  return ((size_t)st_chunks(n) + 1) * (size_t)d * sizeof(double);
}

extern "C" int mmk_pca_colstats_f64(const float* x, int64_t x_row_stride, int64_t n, int32_t d, double* mean, double* scale, void* workspace,
                                    size_t workspace_bytes, mmk_stream_t stream) {
  using namespace mmk;
  if (n < 1 || d < 1) return fail(MMK_ERR_INVALID, "pca_colstats: n = %lld rows, d = %d columns (both at least 1)", (long long)n, d);
  if (d > MMK_PCA_MAX_D) return fail(MMK_ERR_UNSUPPORTED, "pca_colstats: d = %d columns, the limit is %d (MMK_PCA_MAX_D)", d, MMK_PCA_MAX_D);
  if (!x || !mean || !scale || !workspace || x_row_stride < 0)
    return fail(MMK_ERR_INVALID, "pca_colstats: bad arguments (null pointer or negative stride %lld)", (long long)x_row_stride);
  if (misaligned(x, 4) || misaligned(mean, 8) || misaligned(scale, 8) || misaligned(workspace, 8))
    return fail(MMK_ERR_INVALID, "pca_colstats: x must be 4-byte aligned, mean, scale and the workspace 8-byte aligned");
  MMK_TRY(workspace_check("pca_colstats", workspace, 8, workspace_bytes, mmk_pca_colstats_workspace_bytes(n, d)));
  hipStream_t st = (hipStream_t)stream;
  const int chunks = st_chunks(n);
  const int64_t rows_per_chunk = (n + chunks - 1) / chunks;
  double* mu = static_cast<double*>(workspace);
  double* partial = mu + d;
  const dim3 grid((unsigned)((d + 63) / 64), (unsigned)chunks), fin((unsigned)((d + 255) / 256)), wg(256);
  MMK_TRY(launch(pca_colsum_kernel<0>, grid, wg, 0, st, x, x_row_stride, n, d, (const double*)nullptr, (const double*)nullptr, rows_per_chunk, partial));
  MMK_TRY(launch(pca_colfin_kernel<0>, fin, wg, 0, st, partial, chunks, n, d, mu, scale, mean));
  MMK_TRY(launch(pca_colsum_kernel<1>, grid, wg, 0, st, x, x_row_stride, n, d, mu, (const double*)nullptr, rows_per_chunk, partial));
  MMK_TRY(launch(pca_colfin_kernel<1>, fin, wg, 0, st, partial, chunks, n, d, mu, scale, mean));
  MMK_TRY(launch(pca_colsum_kernel<2>, grid, wg, 0, st, x, x_row_stride, n, d, mu, scale, rows_per_chunk, partial));
  return launch(pca_colfin_kernel<2>, fin, wg, 0, st, partial, chunks, n, d, mu, scale, mean);
}

extern "C" size_t mmk_pca_cov_workspace_bytes(int64_t n, int32_t d) {
  using namespace mmk;
  if (n < 2 || d < 1 || d > MMK_PCA_MAX_D) return 0;
  const CvPlan p = cv_plan(n, d);
  return (size_t)p.runs * (size_t)p.pairs * kCvTile * kCvTile * sizeof(double);
}

extern "C" int mmk_pca_cov_f64(const float* x, int64_t x_row_stride, int64_t n, int32_t d, const double* mean, const double* scale, double* c,
                               void* workspace, size_t workspace_bytes, mmk_stream_t stream) {
  using namespace mmk;
  if (n < 2 || d < 1) return fail(MMK_ERR_INVALID, "pca_cov: n = %lld rows (at least 2), d = %d columns (at least 1)", (long long)n, d);
  if (d > MMK_PCA_MAX_D) return fail(MMK_ERR_UNSUPPORTED, "pca_cov: d = %d columns, the limit is %d (MMK_PCA_MAX_D)", d, MMK_PCA_MAX_D);
  if (!x || !mean || !scale || !c || !workspace || x_row_stride < 0)
    return fail(MMK_ERR_INVALID, "pca_cov: bad arguments (null pointer or negative stride %lld)", (long long)x_row_stride);
  if (misaligned(x, 4) || misaligned(mean, 8) || misaligned(scale, 8) || misaligned(c, 8) || misaligned(workspace, 8))
    return fail(MMK_ERR_INVALID, "pca_cov: x must be 4-byte aligned, mean, scale, c and the workspace 8-byte aligned");
  MMK_TRY(workspace_check("pca_cov", workspace, 8, workspace_bytes, mmk_pca_cov_workspace_bytes(n, d)));
  hipStream_t st = (hipStream_t)stream;
  const CvPlan p = cv_plan(n, d);
  double* partial = static_cast<double*>(workspace);
  MMK_TRY(launch(pca_cov_kernel, dim3((unsigned)(p.pairs * p.runs)), dim3(256), 0, st, x, x_row_stride, n, d, mean, scale, p.rows_per_run, p.pairs,
                 partial));
  return launch(pca_cov_reduce_kernel, dim3((unsigned)(p.pairs * (kCvTile * kCvTile / 256))), dim3(256), 0, st, partial, p.pairs, p.runs, d,
                (double)(n - 1), c);
}

extern "C" size_t mmk_pca_eig_workspace_bytes(int32_t d, int32_t n_components) {
  using namespace mmk;
  if (d < 1 || d > MMK_PCA_MAX_D || n_components < 1 || n_components > MMK_PCA_MAX_COMPONENTS || n_components > d) return 0;
  const size_t b = (size_t)pc_block(d, n_components);
  return (4 * (size_t)d * b + 3 * b * b + b + (size_t)d + (size_t)n_components + 4) * sizeof(double);
}

extern "C" int mmk_pca_eig_f64(const double* c, int32_t d, int32_t n_components, int32_t max_iter, double* components, double* variance,
                               int32_t* n_iter, void* workspace, size_t workspace_bytes, mmk_stream_t stream) {
  using namespace mmk;
  if (d < 1 || n_components < 1 || n_components > d)
    return fail(MMK_ERR_INVALID, "pca_eig: n_components = %d must lie in [1, d = %d]", n_components, d);
  if (d > MMK_PCA_MAX_D) return fail(MMK_ERR_UNSUPPORTED, "pca_eig: d = %d columns, the limit is %d (MMK_PCA_MAX_D)", d, MMK_PCA_MAX_D);
  if (n_components > MMK_PCA_MAX_COMPONENTS)
    return fail(MMK_ERR_UNSUPPORTED, "pca_eig: n_components = %d, the limit is %d (MMK_PCA_MAX_COMPONENTS: the Jacobi step's block fits LDS)",
                n_components, MMK_PCA_MAX_COMPONENTS);
  if (max_iter < 0) return fail(MMK_ERR_INVALID, "pca_eig: max_iter = %d < 0 (0: MMK_PCA_MAX_ITER)", max_iter);
  if (!c || !components || !variance || !n_iter || !workspace) return fail(MMK_ERR_INVALID, "pca_eig: bad arguments (null pointer)");
  if (misaligned(c, 8) || misaligned(components, 8) || misaligned(variance, 8) || misaligned(workspace, 8))
    return fail(MMK_ERR_INVALID, "pca_eig: c, components, variance and the workspace must be 8-byte aligned");
  MMK_TRY(workspace_check("pca_eig", workspace, 8, workspace_bytes, mmk_pca_eig_workspace_bytes(d, n_components)));
  hipStream_t st = (hipStream_t)stream;
  const int b = pc_block(d, n_components);
  const int cap = max_iter > 0 ? max_iter : MMK_PCA_MAX_ITER;
  const int64_t db = (int64_t)d * b;
  double* y = static_cast<double*>(workspace);
  double* qp = y + db;
  double* z = qp + db;
  double* q = z + db;
  double* h = q + db;
  double* w = h + b * b;
  double* w2 = w + b * b;
  double* theta = w2 + b * b;
  double* rowsum = theta + b;
  double* resid = rowsum + d;
  double* stat = resid + n_components;                   // |C|_inf, the last residual, then the flag
  int32_t* done = reinterpret_cast<int32_t*>(stat + 2);
  const dim3 wg(256), wide(kPcWide), per_elem((unsigned)((db + 255) / 256));
  MMK_HIP(hipMemsetAsync(stat, 0, 4 * sizeof(double), st));
  MMK_TRY(launch(pca_start_kernel, per_elem, wg, 0, st, d, b, y));
  MMK_TRY(launch(pca_rowsum_kernel, dim3((unsigned)d), wg, 0, st, c, d, rowsum));
  MMK_TRY(launch(pca_cnorm_kernel, dim3(1), dim3(64), 0, st, rowsum, d, stat));
  struct {
    double cnorm, resid;
    int32_t done, pad;
  } host = {0.0, 0.0, 0, 0};
  int it = 0;
  while (it < cap && !host.done) {
    ++it;
    MMK_TRY(launch(pca_qr_kernel, dim3(1), wide, 0, st, d, b, y, qp, done));
    MMK_TRY(launch(pca_cq_kernel, dim3((unsigned)((d + 15) / 16), (unsigned)((b + 15) / 16)), wg, 0, st, c, d, b, qp, z, done));
    MMK_TRY(launch(pca_h_kernel, dim3((unsigned)b), wide, 0, st, d, b, qp, z, h, done));
    MMK_TRY(launch(pca_jacobi_kernel, dim3(1), wide, 0, st, b, h, w, w2, theta, done));
    MMK_TRY(launch(pca_rotate_kernel, per_elem, wg, 0, st, d, b, qp, z, w2, q, y, done));
    MMK_TRY(launch(pca_resid_kernel, dim3((unsigned)n_components), wg, 0, st, d, b, q, y, theta, resid, done));
    MMK_TRY(launch(pca_check_kernel, dim3(1), dim3(64), 0, st, n_components, it, resid, stat, done));
    if (it % kPcPoll == 0 || it == cap) {
      MMK_HIP(hipMemcpyAsync(&host, stat, sizeof(host), hipMemcpyDeviceToHost, st));
      MMK_HIP(hipStreamSynchronize(st));
      if (host.resid != host.resid) break;              // NaN: no later iteration mends it
    }
  }
  if (!host.done)
    return fail(MMK_ERR_CONVERGENCE,
                "pca_eig: %d iterations of the subspace iteration left a residual of %.3e, the stop rule asks for %.3e (= %.0e |C|_inf) "
                "over the first %d of %d columns",
                it, host.resid, kPcTol * host.cnorm, kPcTol, n_components, b);
  *n_iter = host.done;
  return launch(pca_finish_kernel, dim3((unsigned)n_components), wg, 0, st, d, b, q, theta, components, variance);
}

extern "C" int mmk_pca_project_f32(const float* y, int64_t y_row_stride, int64_t m, int32_t d, const double* mean, const double* scale,
                                   const double* components, int32_t n_components, float* out, int64_t out_row_stride, mmk_stream_t stream) {
  using namespace mmk;
  if (m < 1 || d < 1 || n_components < 1)
    return fail(MMK_ERR_INVALID, "pca_project: m = %lld rows, d = %d columns, n_components = %d (all at least 1)", (long long)m, d, n_components);
  if (d > MMK_PCA_MAX_D) return fail(MMK_ERR_UNSUPPORTED, "pca_project: d = %d columns, the limit is %d (MMK_PCA_MAX_D)", d, MMK_PCA_MAX_D);
  if (n_components > MMK_PCA_MAX_COMPONENTS)
    return fail(MMK_ERR_UNSUPPORTED, "pca_project: n_components = %d, the limit is %d (MMK_PCA_MAX_COMPONENTS)", n_components,
                MMK_PCA_MAX_COMPONENTS);
  if ((m + kPjRows - 1) / kPjRows > 0x7fffffffLL)
    return fail(MMK_ERR_UNSUPPORTED, "pca_project: %lld rows are more than one launch takes", (long long)m);
  if (!y || !mean || !scale || !components || !out || y_row_stride < 0 || out_row_stride < n_components)
    return fail(MMK_ERR_INVALID, "pca_project: bad arguments (null pointer, negative stride %lld or an output stride %lld below n_components)",
                (long long)y_row_stride, (long long)out_row_stride);
  if (misaligned(y, 4) || misaligned(out, 4) || misaligned(mean, 8) || misaligned(scale, 8) || misaligned(components, 8))
    return fail(MMK_ERR_INVALID, "pca_project: y and out must be 4-byte aligned, mean, scale and components 8-byte aligned");
  return launch(pca_project_kernel, dim3((unsigned)((m + kPjRows - 1) / kPjRows)), dim3(256), 0, (hipStream_t)stream, y, y_row_stride, m, d, mean,
                scale, components, n_components, out, out_row_stride);
}
