// The block subspace iteration's kernels that do not depend on how the matrix is applied: the start block, the Householder QR, H = Q'^T Z,
// the cyclic Jacobi of H, the rotation, the residuals and the signed copy-out.  pca.hip (Z = C Q', mmk_pca_eig_f64, which nmf.hip calls) and
// factor_analysis.hip (Z = S C S Q' with a diagonal S that changes from one EM step to the next) include this header and bring their own
// product, norm and stop kernels.  Every kernel of an iteration takes the caller's `done` word and returns at once when it is set; the
// kernels are `inline` so that each translation unit holds its own copy of the ones it launches.
#pragma once
#include "entry_util.h"
#include "wave_ops.h"

#include <math.h>

namespace mmk {

typedef double pc_f64x4 __attribute__((ext_vector_type(4)));

constexpr double kPcTol = MMK_PCA_TOL;  // the stop rule's tolerance, relative to the matrix' infinity norm
constexpr int kPcPoll = 8;              // the host reads the convergence flag every kPcPoll iterations
constexpr int kPcGuard = 16;            // guard columns of the block beyond n_components (pca.hip states it as kPcExtra)
constexpr int kPcMaxBlock = MMK_PCA_MAX_COMPONENTS + kPcGuard;
constexpr int kPcSweeps = 40;           // cap of the Jacobi sweeps (8 to 10 are typical)
constexpr int kPcWide = 1024;           // threads of the one-workgroup kernels
static_assert(kPcMaxBlock == 80, "the Jacobi kernel's LDS is sized for 80 columns");

inline int pc_block(int32_t d, int32_t ncomp) { return d < ncomp + kPcGuard ? d : ncomp + kPcGuard; }

inline __global__ __launch_bounds__(256) void pca_start_kernel(int32_t d, int32_t b, double* __restrict__ y) {
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (int64_t)d * b) return;
  uint32_t h = (uint32_t)idx * 0x9E3779B9u + 0x7F4A7C15u;
  h ^= h >> 16;
  h *= 0x85EBCA6Bu;
  h ^= h >> 13;
  h *= 0xC2B2AE35u;
  h ^= h >> 16;
  y[idx] = (double)(h >> 8) * (1.0 / 8388608.0) - 1.0;      // [-1, 1), exact
}

// Householder QR of y (d, b) row-major in place, then qp (d, b) = the first b columns of the product of the reflectors.  One workgroup of
// kPcWide threads: thread (g, j) = (tid / b, tid % b) walks the rows g, g + nrg, ... of column j.
inline __global__ __launch_bounds__(kPcWide) void pca_qr_kernel(int32_t d, int32_t b, double* __restrict__ y, double* __restrict__ qp,
                                                                const int32_t* __restrict__ done) {
  __shared__ double part[kPcWide];
  __shared__ double red[kPcWide / 64];
  __shared__ double betas[kPcMaxBlock];
  if (*done) return;
  const int tid = threadIdx.x;
  const int nrg = kPcWide / b;
  const int g = tid / b, j = tid % b;
  const bool live = g < nrg;
  for (int k = 0; k < b; ++k) {
    double ss = 0.0;
    for (int i = k + tid; i < d; i += kPcWide) {
      const double v = y[(int64_t)i * b + k];
      ss = fma(v, v, ss);
    }
    const double x0 = y[(int64_t)k * b + k];
    ss = block_sum(ss, red);
    const double nrm = sqrt(ss);
    double beta = 0.0, v0 = x0;
    if (nrm > 0.0) {
      const double alpha = x0 >= 0.0 ? -nrm : nrm;
      v0 = x0 - alpha;
      beta = -1.0 / (alpha * v0);
    }
    __syncthreads();                                 // every thread has read x0
    if (tid == 0) {
      y[(int64_t)k * b + k] = v0;
      betas[k] = beta;
    }
    __syncthreads();
    double p = 0.0;
    if (live && j > k)
      for (int i = k + g; i < d; i += nrg) p = fma(y[(int64_t)i * b + k], y[(int64_t)i * b + j], p);
    part[tid] = p;
    __syncthreads();
    if (live && j > k) {
      double s = 0.0;
      for (int gg = 0; gg < nrg; ++gg) s += part[gg * b + j];
      s *= beta;
      for (int i = k + g; i < d; i += nrg) y[(int64_t)i * b + j] = fma(-s, y[(int64_t)i * b + k], y[(int64_t)i * b + j]);
    }
    __syncthreads();
  }
  for (int64_t idx = tid; idx < (int64_t)d * b; idx += kPcWide) qp[idx] = (idx / b == idx % b) ? 1.0 : 0.0;
  __syncthreads();
  for (int k = b - 1; k >= 0; --k) {
    const double beta = betas[k];
    double p = 0.0;
    if (live && j >= k)
      for (int i = k + g; i < d; i += nrg) p = fma(y[(int64_t)i * b + k], qp[(int64_t)i * b + j], p);
    part[tid] = p;
    __syncthreads();
    if (live && j >= k) {
      double s = 0.0;
      for (int gg = 0; gg < nrg; ++gg) s += part[gg * b + j];
      s *= beta;
      for (int i = k + g; i < d; i += nrg) qp[(int64_t)i * b + j] = fma(-s, y[(int64_t)i * b + k], qp[(int64_t)i * b + j]);
    }
    __syncthreads();
  }
}

// h (b, b) = qp^T z: workgroup a computes row a
inline __global__ __launch_bounds__(kPcWide) void pca_h_kernel(int32_t d, int32_t b, const double* __restrict__ qp, const double* __restrict__ z,
                                                               double* __restrict__ h, const int32_t* __restrict__ done) {
  __shared__ double part[kPcWide];
  if (*done) return;
  const int tid = threadIdx.x, a = blockIdx.x;
  const int nrg = kPcWide / b;
  const int g = tid / b, j = tid % b;
  double p = 0.0;
  if (g < nrg)
    for (int i = g; i < d; i += nrg) p = fma(qp[(int64_t)i * b + a], z[(int64_t)i * b + j], p);
  part[tid] = p;
  __syncthreads();
  if (tid < b) {
    double s = 0.0;
    for (int gg = 0; gg < nrg; ++gg) s += part[gg * b + tid];
    h[a * b + tid] = s;
  }
}

// eigenvectors (columns of w2, sorted by falling eigenvalue theta) of the symmetrised h: cyclic Jacobi, b / 2 disjoint rotations at a time
inline __global__ __launch_bounds__(kPcWide) void pca_jacobi_kernel(int32_t b, const double* __restrict__ h, double* __restrict__ w,
                                                                    double* __restrict__ w2, double* __restrict__ theta,
                                                                    const int32_t* __restrict__ done) {
  constexpr int P = kPcMaxBlock + 1;
  __shared__ double hs[kPcMaxBlock * P];
  __shared__ double cs[kPcMaxBlock / 2], sn[kPcMaxBlock / 2];
  __shared__ int pp[kPcMaxBlock / 2], qq[kPcMaxBlock / 2], rank[kPcMaxBlock];
  __shared__ int rotated;
  if (*done) return;
  const int tid = threadIdx.x;
  for (int idx = tid; idx < b * b; idx += kPcWide) {
    const int a = idx / b, c = idx % b;
    hs[a * P + c] = 0.5 * (h[a * b + c] + h[c * b + a]);
    w[idx] = a == c ? 1.0 : 0.0;
  }
  const int m = (b + 1) & ~1, half = m / 2;
  __syncthreads();
  for (int sweep = 0; sweep < kPcSweeps; ++sweep) {
    if (tid == 0) rotated = 0;
    __syncthreads();
    for (int r = 0; r < m - 1; ++r) {
      if (tid < half) {
        int p = tid == 0 ? m - 1 : (r + tid) % (m - 1);
        int q = tid == 0 ? r : (r - tid + (m - 1)) % (m - 1);
        if (p > q) {
          const int t = p;
          p = q;
          q = t;
        }
        double c = 1.0, s = 0.0;
        if (q < b) {
          const double apq = hs[p * P + q], app = hs[p * P + p], aqq = hs[q * P + q];
          const double g = 100.0 * fabs(apq);
          if (apq != 0.0 && !(fabs(app) + g == fabs(app) && fabs(aqq) + g == fabs(aqq))) {
            const double th = (aqq - app) / (2.0 * apq);
            const double t = (th >= 0.0 ? 1.0 : -1.0) / (fabs(th) + sqrt(th * th + 1.0));
            c = 1.0 / sqrt(t * t + 1.0);
            s = t * c;
            rotated = 1;
          }
        }
        pp[tid] = p;
        qq[tid] = q;
        cs[tid] = c;
        sn[tid] = s;
      }
      __syncthreads();
      for (int idx = tid; idx < b * half; idx += kPcWide) {      // H <- H J, W <- W J
        const int i = idx / half, t = idx % half;
        const int p = pp[t], q = qq[t];
        const double c = cs[t], s = sn[t];
        if (q < b && s != 0.0) {
          const double hp = hs[i * P + p], hq = hs[i * P + q];
          hs[i * P + p] = c * hp - s * hq;
          hs[i * P + q] = s * hp + c * hq;
          const double wp = w[i * b + p], wq = w[i * b + q];
          w[i * b + p] = c * wp - s * wq;
          w[i * b + q] = s * wp + c * wq;
        }
      }
      __syncthreads();
      for (int idx = tid; idx < b * half; idx += kPcWide) {      // H <- J^T H
        const int jc = idx / half, t = idx % half;
        const int p = pp[t], q = qq[t];
        const double c = cs[t], s = sn[t];
        if (q < b && s != 0.0) {
          const double hp = hs[p * P + jc], hq = hs[q * P + jc];
          hs[p * P + jc] = c * hp - s * hq;
          hs[q * P + jc] = s * hp + c * hq;
        }
      }
      __syncthreads();
    }
    const int any = rotated;
    __syncthreads();
    if (!any) break;
  }
  if (tid < b) {
    const double mine = hs[tid * P + tid];
    int rk = 0;
    for (int i = 0; i < b; ++i) {
      const double o = hs[i * P + i];
      rk += (o > mine || (o == mine && i < tid)) ? 1 : 0;
    }
    rank[tid] = rk;
    theta[rk] = mine;
  }
  __syncthreads();
  for (int idx = tid; idx < b * b; idx += kPcWide) w2[(idx / b) * b + rank[idx % b]] = w[idx];
}

// q (d, b) = qp w2, y (d, b) = z w2
inline __global__ __launch_bounds__(256) void pca_rotate_kernel(int32_t d, int32_t b, const double* __restrict__ qp, const double* __restrict__ z,
                                                                const double* __restrict__ w2, double* __restrict__ q, double* __restrict__ y,
                                                                const int32_t* __restrict__ done) {
  if (*done) return;
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (int64_t)d * b) return;
  const int64_t i = idx / b;
  const int j = (int)(idx % b);
  double aq = 0.0, ay = 0.0;
  for (int k = 0; k < b; ++k) {
    const double wv = w2[k * b + j];
    aq = fma(qp[i * b + k], wv, aq);
    ay = fma(z[i * b + k], wv, ay);
  }
  q[idx] = aq;
  y[idx] = ay;
}

inline __global__ __launch_bounds__(256) void pca_resid_kernel(int32_t d, int32_t b, const double* __restrict__ q, const double* __restrict__ y,
                                                               const double* __restrict__ theta, double* __restrict__ resid,
                                                               const int32_t* __restrict__ done) {
  __shared__ double red[4];
  if (*done) return;
  const int k = blockIdx.x;
  const double th = theta[k];
  double acc = 0.0;
  for (int i = threadIdx.x; i < d; i += 256) {
    const double r = fma(-th, q[(int64_t)i * b + k], y[(int64_t)i * b + k]);
    acc = fma(r, r, acc);
  }
  acc = block_sum(acc, red);
  if (threadIdx.x == 0) resid[k] = sqrt(acc);
}

// components[k][0 .. d) = +-q[.][k], the sign that makes the entry of largest magnitude (the first of equals) positive
inline __global__ __launch_bounds__(256) void pca_finish_kernel(int32_t d, int32_t b, const double* __restrict__ q, const double* __restrict__ theta,
                                                                double* __restrict__ components, double* __restrict__ variance) {
  __shared__ double bv[256];
  __shared__ int bi[256];
  const int k = blockIdx.x, tid = threadIdx.x;
  double best = -1.0;
  int at = 0x7fffffff;
  for (int i = tid; i < d; i += 256) {
    const double a = fabs(q[(int64_t)i * b + k]);
    if (a > best) {
      best = a;
      at = i;
    }
  }
  bv[tid] = best;
  bi[tid] = at;
  __syncthreads();
  for (int off = 128; off >= 1; off >>= 1) {
    if (tid < off && (bv[tid + off] > bv[tid] || (bv[tid + off] == bv[tid] && bi[tid + off] < bi[tid]))) {
      bv[tid] = bv[tid + off];
      bi[tid] = bi[tid + off];
    }
    __syncthreads();
  }
  const double sign = q[(int64_t)bi[0] * b + k] < 0.0 ? -1.0 : 1.0;
  for (int i = tid; i < d; i += 256) components[(int64_t)k * d + i] = sign * q[(int64_t)i * b + k];
  if (tid == 0) variance[k] = theta[k] > 0.0 ? theta[k] : 0.0;
}

}  // namespace mmk
