// Factor analysis of corpus frames (mimikit/features/functionals.py:1173-1203 FactorAnalysis = sklearn's FactorAnalysis, EM on the noise
// variances psi) in Gram form: include/mmk_factor_analysis.h states the algorithm.  Everything is fp64; the frames enter through
// C = Xc^T Xc / n alone (pca.hip's covariance kernel), so the EM steps never touch them.  No atomics, every sum in one fixed order.
//
//   the EM entry     one launch sequence per INNER iteration of the block subspace iteration on G = S C S, S = diag(1 / (sqrt(psi) + 1e-12)):
//                        qr, fa_scq, h, jacobi, rotate, resid (subspace_eig.h, shared with pca.hip)   and   fa_advance
//                    fa_scq is pca_cq_kernel with the two scalings: Q's rows by 1/sp while they are loaded, Z's rows in the epilogue; its
//                    first column of workgroups also sums |G|'s rows from the C values it loads anyway.  fa_advance is the state machine:
//                    it takes |G|_inf and the largest residual; below the stop rule it forms ll, tests the EM stop, updates psi (the next
//                    inner iteration then works on the new G, from the block this one left) and counts the step; at the stop it writes W
//                    with its signs and sets FaState.stop, which is the `done` word of every kernel.
//   the transform    M = I + Wpsi W^T (k x k, SPD) in LDS, Cholesky, the factor's inverse into the upper triangle, M^-1 to the workspace;
//                    a second launch forms A = M^-1 Wpsi.
#include "subspace_eig.h"

#include "../../include/mmk_factor_analysis.h"

namespace mmk {

constexpr double kFaSmall = MMK_FA_SMALL;
constexpr int kFaPitch = MMK_FA_MAX_COMPONENTS + 1;

struct FaState {
  double gnorm, resid, old_ll, pad0;  // |G|_inf and the largest residual of the last inner iteration that ran; ll of the last EM step
  int32_t stop;                       // 0: running;  > 0: the EM steps taken at the stop;  < 0: -(EM step + 1) whose eigen step failed
  int32_t em;                         // EM steps completed
  int32_t inner;                      // inner iterations of the current EM step
  int32_t total;                      // inner iterations in all
  int32_t step0;                      // inner iterations of EM step 0
  int32_t hit_tol;                    // 1: ll - old < tol stopped the loop
  int32_t pad1[2];
};
static_assert(sizeof(FaState) == 64, "the state is copied to the host as eight doubles");

__global__ __launch_bounds__(256) void fa_init_kernel(int32_t d, double* __restrict__ psi, double* __restrict__ spinv, FaState* __restrict__ st) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < d) {
    psi[i] = 1.0;
    spinv[i] = 1.0 / (1.0 + kFaSmall);
  }
  if (i == 0) {
    FaState s = {};
    s.old_ll = -INFINITY;
    *st = s;
  }
}

// z (d, b) = S C S qp, rowsum[i] = sum_j |G[i][j]| (workgroups of column 0): a workgroup owns a 16 x 16 tile of z, its four waves a quarter
// of the sum each, added in rising wave order.  C/D of v_mfma_f64_16x16x4_f64: col = lane & 15, row = (lane >> 4) + 4 reg.
__global__ __launch_bounds__(256) void fa_scq_kernel(const double* __restrict__ c, int32_t d, int32_t b, const double* __restrict__ qp,
                                                     const double* __restrict__ spinv, double* __restrict__ z, double* __restrict__ rowsum,
                                                     const int32_t* __restrict__ done) {
  __shared__ double red[4][256];
  __shared__ double rs[4][64];
  if (*done) return;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int r0 = blockIdx.x * 16, c0 = blockIdx.y * 16;
  const int kq = ((d + 3) / 4 + 3) & ~3;
  const int kbeg = wave * kq, kend = (wave + 1) * kq < d ? (wave + 1) * kq : d;
  const int row = r0 + (lane & 15), colq = c0 + (lane & 15);
  const int rowc = row < d ? row : d - 1, colc = colq < b ? colq : b - 1;
  pc_f64x4 acc = {0.0, 0.0, 0.0, 0.0};
  double rsum = 0.0;
  for (int k0 = kbeg; k0 < kend; k0 += 4) {
    const int k = k0 + (lane >> 4);
    const int kc = k < d ? k : d - 1;
    const double sk = spinv[kc];
    const double av = c[(int64_t)kc * d + rowc];     // = C[row][k]: C is mirrored exactly
    const double bv = qp[(int64_t)kc * b + colc] * sk;
    const bool kin = k < kend;
    const double a = (kin && row < d) ? av : 0.0;
    rsum = fma(fabs(a), sk, rsum);
    acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a, (kin && colq < b) ? bv : 0.0, acc, 0, 0, 0);
  }
#pragma unroll
  for (int q = 0; q < 4; ++q) red[wave][q * 64 + lane] = acc[q];
  rs[wave][lane] = rsum;
  __syncthreads();
  if (wave == 0) {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int orow = r0 + (lane >> 4) + 4 * q, ocol = c0 + (lane & 15);
      const double v = ((red[0][q * 64 + lane] + red[1][q * 64 + lane]) + red[2][q * 64 + lane]) + red[3][q * 64 + lane];
      if (orow < d && ocol < b) z[(int64_t)orow * b + ocol] = v * spinv[orow];
    }
    if (blockIdx.y == 0 && lane < 16 && row < d) {
      double s = 0.0;
      for (int w = 0; w < 4; ++w)
        for (int g = 0; g < 4; ++g) s += rs[w][g * 16 + lane];
      rowsum[row] = s * spinv[row];
    }
  }
}

__device__ __forceinline__ double fa_block_max(double v, double* red) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) v = fmax(v, __shfl_xor(v, off));
  const int nw = blockDim.x >> 6;
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  double m = red[0];
  for (int w = 1; w < nw; ++w) m = fmax(m, red[w]);
  return m;
}

// the state machine (file comment).  One workgroup of kPcWide threads; psi is the caller's noise_variance.
__global__ __launch_bounds__(kPcWide) void fa_advance_kernel(const double* __restrict__ c, int32_t d, int32_t b, int32_t ncomp, double nn, double tol,
                                                             int32_t max_em, int32_t cap, const double* __restrict__ q,
                                                             const double* __restrict__ theta, const double* __restrict__ resid,
                                                             const double* __restrict__ rowsum, double* __restrict__ psi,
                                                             double* __restrict__ spinv, double* __restrict__ components,
                                                             double* __restrict__ loglike, FaState* __restrict__ st) {
  __shared__ double red[kPcWide / 64];
  __shared__ double fac[MMK_PCA_MAX_COMPONENTS];
  if (st->stop) return;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  double g = 0.0;
  for (int i = tid; i < d; i += kPcWide) g = fmax(g, rowsum[i]);
  g = fa_block_max(g, red);
  double m = 0.0;
  for (int k = 0; k < ncomp; ++k) m = (resid[k] > m || resid[k] != resid[k]) ? resid[k] : m;
  const int inner = st->inner + 1, em = st->em, total = st->total + 1;
  const double old = st->old_ll;
  __syncthreads();                                   // every thread has read the state
  const bool bad = m != m;
  if (bad || !(m <= kPcTol * g)) {
    if (tid == 0) {
      st->gnorm = g;
      st->resid = m;
      st->inner = inner;
      st->total = total;
      if (bad || inner >= cap) st->stop = -(em + 1);
    }
    return;
  }
  // ---- the eigen step has converged: EM step `em`
  if (tid < ncomp) fac[tid] = sqrt(fmax(theta[tid] - 1.0, 0.0));
  const double slt = block_sum(tid < ncomp ? log(theta[tid]) : 0.0, red);
  const double sth = block_sum(tid < ncomp ? theta[tid] : 0.0, red);
  double tr = 0.0, slp = 0.0;
  for (int i = tid; i < d; i += kPcWide) {
    const double si = spinv[i];
    tr += c[(int64_t)i * d + i] * si * si;
    slp += log(psi[i]);
  }
  tr = block_sum(tr, red);
  slp = block_sum(slp, red);
  const double ll = -0.5 * nn * ((double)d * 1.8378770664093453 + (double)ncomp + slt + (tr - sth) + slp);      // log(2 pi)
  const bool hit = ll - old < tol, last = em + 1 >= max_em;
  if (hit || last) {
    // W, row by row: a wave finds the row's entry of largest magnitude (the first of equals) and writes the row with that entry positive
    for (int j = wave; j < ncomp; j += kPcWide / 64) {
      const double f = fac[j];
      double best = -1.0;
      int at = 0x7fffffff;
      for (int i = lane; i < d; i += 64) {
        const double a = fabs((f * q[(int64_t)i * b + j]) * (sqrt(psi[i]) + kFaSmall));
        if (a > best) {
          best = a;
          at = i;
        }
      }
#pragma unroll
      for (int off = 32; off >= 1; off >>= 1) {
        const double ob = __shfl_xor(best, off);
        const int oi = __shfl_xor(at, off);
        if (ob > best || (ob == best && oi < at)) {
          best = ob;
          at = oi;
        }
      }
      if (at >= d) at = 0;                           // (a row of NaN: no entry compared larger)
      const double sign = f * q[(int64_t)at * b + j] < 0.0 ? -1.0 : 1.0;
      for (int i = lane; i < d; i += 64) components[(int64_t)j * d + i] = sign * ((f * q[(int64_t)i * b + j]) * (sqrt(psi[i]) + kFaSmall));
    }
  }
  __syncthreads();                                   // W is written from the psi it belongs to
  if (!hit) {
    for (int i = tid; i < d; i += kPcWide) {
      const double sp = sqrt(psi[i]) + kFaSmall;
      double s = 0.0;
      for (int j = 0; j < ncomp; ++j) {
        const double w = (fac[j] * q[(int64_t)i * b + j]) * sp;
        s = fma(w, w, s);
      }
      const double p = fmax(c[(int64_t)i * d + i] - s, kFaSmall);
      psi[i] = p;
      spinv[i] = 1.0 / (sqrt(p) + kFaSmall);
    }
  }
  if (tid == 0) {
    loglike[em] = ll;
    st->gnorm = g;
    st->resid = m;
    st->old_ll = ll;
    st->em = em + 1;
    st->inner = 0;
    st->total = total;
    if (em == 0) st->step0 = inner;
    if (hit || last) {
      st->hit_tol = hit ? 1 : 0;
      st->stop = em + 1;
    }
  }
}

// minv (k, k) = (I + Wpsi W^T)^-1, one workgroup: M's lower triangle in LDS, Cholesky in place, column c of the factor's inverse by
// thread c into row c of the strict upper triangle (its diagonal in dinv), then M^-1 = L^-T L^-1 entry by entry
__global__ __launch_bounds__(kPcWide) void fa_minv_kernel(const double* __restrict__ w, const double* __restrict__ psi, int32_t d, int32_t k,
                                                          double* __restrict__ minv) {
  __shared__ double ms[MMK_FA_MAX_COMPONENTS * kFaPitch];
  __shared__ double dinv[MMK_FA_MAX_COMPONENTS];
  const int tid = threadIdx.x;
  for (int idx = tid; idx < k * k; idx += kPcWide) {
    const int a = idx / k, bb = idx % k;
    if (bb > a) continue;
    double s = 0.0;
    for (int i = 0; i < d; ++i) s = fma(w[(int64_t)a * d + i] / psi[i], w[(int64_t)bb * d + i], s);
    ms[a * kFaPitch + bb] = a == bb ? s + 1.0 : s;
  }
  for (int j = 0; j < k; ++j) {
    __syncthreads();
    if (tid == 0) ms[j * kFaPitch + j] = sqrt(ms[j * kFaPitch + j]);
    __syncthreads();
    const double djj = ms[j * kFaPitch + j];
    for (int r = j + 1 + tid; r < k; r += kPcWide) ms[r * kFaPitch + j] /= djj;
    __syncthreads();
    const int rest = k - j - 1;
    for (int idx = tid; idx < rest * rest; idx += kPcWide) {
      const int r = j + 1 + idx / rest, cc = j + 1 + idx % rest;
      if (cc <= r) ms[r * kFaPitch + cc] = fma(-ms[r * kFaPitch + j], ms[cc * kFaPitch + j], ms[r * kFaPitch + cc]);
    }
  }
  __syncthreads();
  if (tid < k) dinv[tid] = 1.0 / ms[tid * kFaPitch + tid];
  __syncthreads();
  if (tid < k) {
    const int cc = tid;
    for (int r = cc + 1; r < k; ++r) {
      double s = ms[r * kFaPitch + cc] * dinv[cc];
      for (int t = cc + 1; t < r; ++t) s = fma(ms[r * kFaPitch + t], ms[cc * kFaPitch + t], s);
      ms[cc * kFaPitch + r] = -s * dinv[r];
    }
  }
  __syncthreads();
  for (int idx = tid; idx < k * k; idx += kPcWide) {
    const int a = idx / k, bb = idx % k;
    const int lo = a > bb ? a : bb;
    double s = 0.0;
    for (int r = lo; r < k; ++r) {
      const double la = r == a ? dinv[a] : ms[a * kFaPitch + r];
      const double lb = r == bb ? dinv[bb] : ms[bb * kFaPitch + r];
      s = fma(la, lb, s);
    }
    minv[idx] = s;
  }
}

// a (k, d) = minv (w / psi)
__global__ __launch_bounds__(256) void fa_apply_kernel(const double* __restrict__ w, const double* __restrict__ psi, const double* __restrict__ minv,
                                                       int32_t d, int32_t k, double* __restrict__ a) {
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (int64_t)k * d) return;
  const int j = (int)(idx / d), i = (int)(idx % d);
  const double p = psi[i];
  double s = 0.0;
  for (int t = 0; t < k; ++t) s = fma(minv[j * k + t], w[(int64_t)t * d + i] / p, s);
  a[idx] = s;
}

static int fa_limits(const char* who, int32_t d, int32_t k) {
  if (d < 1 || k < 1 || k > d) return fail(MMK_ERR_INVALID, "%s: n_components = %d must lie in [1, d = %d]", who, k, d);
  if (d > MMK_FA_MAX_D) return fail(MMK_ERR_UNSUPPORTED, "%s: d = %d columns, the limit is %d (MMK_FA_MAX_D)", who, d, MMK_FA_MAX_D);
  if (k > MMK_FA_MAX_COMPONENTS)
    return fail(MMK_ERR_UNSUPPORTED, "%s: n_components = %d, the limit is %d (MMK_FA_MAX_COMPONENTS: the Jacobi block and the Cholesky fit LDS)", who, k,
                MMK_FA_MAX_COMPONENTS);
  return MMK_OK;
}

}  // namespace mmk

// ---------------------------------------------------------------------------------------------------------------- entry points
extern "C" size_t mmk_fa_fit_workspace_bytes(int32_t d, int32_t n_components) {
  using namespace mmk;
  if (d < 1 || d > MMK_FA_MAX_D || n_components < 1 || n_components > MMK_FA_MAX_COMPONENTS || n_components > d) return 0;
  const size_t b = (size_t)pc_block(d, n_components);
  return (4 * (size_t)d * b + 3 * b * b + b + 2 * (size_t)d + (size_t)n_components) * sizeof(double) + sizeof(FaState);
}

extern "C" int mmk_fa_fit_f64(const double* c, int32_t d, int32_t n_components, int64_t n, double tol, int32_t max_iter, double* components,
                              double* noise_variance, double* loglike, int32_t* n_iter, int32_t* converged, int32_t* inner_iters, void* workspace,
                              size_t workspace_bytes, mmk_stream_t stream) {
  using namespace mmk;
  MMK_TRY(fa_limits("fa_fit", d, n_components));
  if (n < 2) return fail(MMK_ERR_INVALID, "fa_fit: n = %lld frames, at least 2 are needed", (long long)n);
  if (max_iter < 1 || !(tol >= 0.0)) return fail(MMK_ERR_INVALID, "fa_fit: max_iter = %d must be at least 1 and tol = %g 0 or above", max_iter, tol);
  if (!c || !components || !noise_variance || !loglike || !n_iter || !converged || !inner_iters || !workspace)
    return fail(MMK_ERR_INVALID, "fa_fit: bad arguments (null pointer)");
  if (misaligned(c, 8) || misaligned(components, 8) || misaligned(noise_variance, 8) || misaligned(loglike, 8) || misaligned(workspace, 8))
    return fail(MMK_ERR_INVALID, "fa_fit: c, components, noise_variance, loglike and the workspace must be 8-byte aligned");
  MMK_TRY(workspace_check("fa_fit", workspace, 8, workspace_bytes, mmk_fa_fit_workspace_bytes(d, n_components)));
  hipStream_t st = (hipStream_t)stream;
  const int b = pc_block(d, n_components);
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
  double* spinv = rowsum + d;
  double* resid = spinv + d;
  FaState* state = reinterpret_cast<FaState*>(resid + n_components);
  const int32_t* done = &state->stop;
  const dim3 wg(256), wide(kPcWide), per_elem((unsigned)((db + 255) / 256));
  MMK_TRY(launch(fa_init_kernel, dim3((unsigned)((d + 255) / 256)), wg, 0, st, d, noise_variance, spinv, state));
  MMK_TRY(launch(pca_start_kernel, per_elem, wg, 0, st, d, b, y));
  FaState host = {};
  const int64_t most = (int64_t)max_iter * MMK_PCA_MAX_ITER;      // (the device stops sooner: every EM step ends or fails within the cap)
  int64_t it = 0;
  while (it < most && !host.stop) {
    ++it;
    MMK_TRY(launch(pca_qr_kernel, dim3(1), wide, 0, st, d, b, y, qp, done));
    MMK_TRY(launch(fa_scq_kernel, dim3((unsigned)((d + 15) / 16), (unsigned)((b + 15) / 16)), wg, 0, st, c, d, b, (const double*)qp, (const double*)spinv, z,
                   rowsum, done));
    MMK_TRY(launch(pca_h_kernel, dim3((unsigned)b), wide, 0, st, d, b, (const double*)qp, (const double*)z, h, done));
    MMK_TRY(launch(pca_jacobi_kernel, dim3(1), wide, 0, st, b, (const double*)h, w, w2, theta, done));
    MMK_TRY(launch(pca_rotate_kernel, per_elem, wg, 0, st, d, b, (const double*)qp, (const double*)z, (const double*)w2, q, y, done));
    MMK_TRY(launch(pca_resid_kernel, dim3((unsigned)n_components), wg, 0, st, d, b, (const double*)q, (const double*)y, (const double*)theta, resid, done));
    MMK_TRY(launch(fa_advance_kernel, dim3(1), wide, 0, st, c, d, b, n_components, (double)n, tol, max_iter, (int32_t)MMK_PCA_MAX_ITER, (const double*)q,
                   (const double*)theta, (const double*)resid, (const double*)rowsum, noise_variance, spinv, components, loglike, state));
    if (it % kPcPoll == 0 || it == most) {
      MMK_HIP(hipMemcpyAsync(&host, state, sizeof(host), hipMemcpyDeviceToHost, st));
      MMK_HIP(hipStreamSynchronize(st));
    }
  }
  if (host.stop <= 0)
    return fail(MMK_ERR_CONVERGENCE,
                "fa_fit: EM step %d: %d iterations of the subspace iteration left a residual of %.3e, the stop rule asks for %.3e (= %.0e |G|_inf) "
                "over the first %d of %d columns (n_components beyond the number of factors in the frames leaves no gap after theta_k)",
                host.stop < 0 ? -host.stop - 1 : host.em, host.inner, host.resid, kPcTol * host.gnorm, kPcTol, n_components, b);
  *n_iter = host.stop;
  *converged = host.hit_tol;
  inner_iters[0] = host.total;
  inner_iters[1] = host.step0;
  return MMK_OK;
}

extern "C" size_t mmk_fa_transform_matrix_workspace_bytes(int32_t d, int32_t n_components) {
  if (d < 1 || d > MMK_FA_MAX_D || n_components < 1 || n_components > MMK_FA_MAX_COMPONENTS || n_components > d) return 0;
  return (size_t)n_components * (size_t)n_components * sizeof(double);
}

extern "C" int mmk_fa_transform_matrix_f64(const double* components, const double* noise_variance, int32_t d, int32_t n_components, double* a,
                                           void* workspace, size_t workspace_bytes, mmk_stream_t stream) {
  using namespace mmk;
  MMK_TRY(fa_limits("fa_transform_matrix", d, n_components));
  if (!components || !noise_variance || !a || !workspace) return fail(MMK_ERR_INVALID, "fa_transform_matrix: bad arguments (null pointer)");
  if (misaligned(components, 8) || misaligned(noise_variance, 8) || misaligned(a, 8) || misaligned(workspace, 8))
    return fail(MMK_ERR_INVALID, "fa_transform_matrix: components, noise_variance, a and the workspace must be 8-byte aligned");
  MMK_TRY(workspace_check("fa_transform_matrix", workspace, 8, workspace_bytes, mmk_fa_transform_matrix_workspace_bytes(d, n_components)));
  hipStream_t st = (hipStream_t)stream;
  double* minv = static_cast<double*>(workspace);
  MMK_TRY(launch(fa_minv_kernel, dim3(1), dim3(kPcWide), 0, st, components, noise_variance, d, n_components, minv));
  return launch(fa_apply_kernel, dim3((unsigned)(((int64_t)n_components * d + 255) / 256)), dim3(256), 0, st, components, noise_variance,
                (const double*)minv, d, n_components, a);
}
