// The time-domain half of the envelope-follower functionals (mimikit/features/functionals.py:794-1004): Interpolate and Derivative.
// (Envelop's frame energies are an epilogue of the STFT kernels: OUT 5 in istft.hip / spectral2048.hip.)  Both are single streaming
// passes: consecutive lanes on consecutive outputs, rows at any stride, 4-byte alignment.
#include "entry_util.h"

namespace mmk {

// ---- Interpolate --------------------------------------------------------------------------------------------------------------------
// ALIGN 1: the positions of np.linspace(0, n - 1, n_out) - double(i) * step with step = (n - 1) / (n_out - 1) made on the host in float64, the
//   last one forced to n - 1 (numpy does both) - so a position is the double scipy's interp1d sees; its weight (a difference of two doubles
//   less than one apart: exact) is rounded to fp32 once.  MODE 0: y_lo + w (y_hi - y_lo), MODE 1 ('previous'): y[floor(pos)].
// ALIGN 0: torch.nn.functional.interpolate(mode="linear", align_corners=False) as its CPU kernel computes it, all in fp32:
//   src = max(fma(scale, i + 0.5, -0.5), 0), scale = float(n) / float(n_out) - ONE rounding: torch's vectorised CPU build fuses the product and
//   the difference, and with two roundings the position of a long row is off by an ulp of ITS size, not of the weight's;
//   i0 = min(int(src), n - 1); i1 = i0 + (i0 < n - 1);
//   l1 = clamp(src - i0, 0, 1); y = (1 - l1) x[i0] + l1 x[i1]; and x[i] itself where n_out == n.
template <int ALIGN, int MODE>
__global__ __launch_bounds__(256) void interp1d_kernel(const float* __restrict__ x, int64_t x_row_stride, int64_t n, float* __restrict__ y,
                                                      int64_t y_row_stride, int64_t n_out, double step, float scale) {
  const float* xr = x + (int64_t)blockIdx.y * x_row_stride;
  float* yr = y + (int64_t)blockIdx.y * y_row_stride;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_out; i += (int64_t)gridDim.x * blockDim.x) {
    if (ALIGN == 1) {
      double pos = (double)i * step;
      if (i == n_out - 1 && n_out > 1) pos = (double)(n - 1);
      int64_t lo = (int64_t)pos;                             // pos >= 0: floor
      lo = lo > n - 1 ? n - 1 : lo;
      if (MODE == 1) {
        yr[i] = xr[lo];
      } else {
        const int64_t hi = lo < n - 1 ? lo + 1 : lo;
        const float w = (float)(pos - (double)lo);
        const float a = xr[lo], b = xr[hi];
        yr[i] = a + w * (b - a);
      }
    } else {
      if (n_out == n) {
        yr[i] = xr[i];
        continue;
      }
      float src = fmaf(scale, (float)i + 0.5f, -0.5f);
      src = src < 0.f ? 0.f : src;
      int64_t i0 = (int64_t)src;
      i0 = i0 > n - 1 ? n - 1 : i0;
      const int64_t i1 = i0 + (i0 < n - 1 ? 1 : 0);
      const float l1 = fminf(fmaxf(src - (float)i0, 0.f), 1.f);
      const float l0 = 1.f - l1;
      yr[i] = l0 * xr[i0] + l1 * xr[i1];
    }
  }
}

// ---- Derivative -----------------------------------------------------------------------------------------------------------------------
// derivative_torch (:960-974) as one pass.  A workgroup owns kDerivTile consecutive outputs of one row and stages them plus a halo of L on
// either side in LDS; the odd reflection about the row's ends, xp[-m] = x[0] + (x[0] - x[m]), xp[n-1+m] = x[n-1] + (x[n-1] - x[n-1-m])
// (the reference's order), is resolved as the halo is loaded (n > L: every index it asks for is inside the row).  Per output the lags are
// added in order 1 .. L, each term as the reference forms it: (float(1 / d) * ((xp[i+d] - x[i]) + (x[i] - xp[i-d]))) / 2, then / L - a true
// division, as torch's (x / 3 and x * float(1 / 3) differ in the last bit).
constexpr int kDerivTile = MMK_DERIV_TILE;
constexpr int kDerivMaxLag = MMK_DERIV_MAX_LAG;

__global__ __launch_bounds__(256) void derivative_kernel(const float* __restrict__ x, int64_t x_row_stride, int64_t n, int L, int64_t n_tiles,
                                                        float* __restrict__ y, int64_t y_row_stride) {
  __shared__ float s_x[kDerivTile + 2 * kDerivMaxLag];
  __shared__ float s_inv[kDerivMaxLag];
  const int64_t row = blockIdx.x / n_tiles, tile = blockIdx.x - row * n_tiles;
  const float* xr = x + row * x_row_stride;
  const int64_t t0 = tile * kDerivTile;
  const float x_first = xr[0], x_last = xr[n - 1];
  for (int j = threadIdx.x; j < kDerivTile + 2 * L; j += blockDim.x) {
    const int64_t p = t0 - L + j;                           // position in the padded row, -L .. n - 1 + L
    float v = 0.f;
    if (p < 0) v = x_first + (x_first - xr[-p]);            // -p <= L < n
    else if (p < n) v = xr[p];
    else if (p < n + L) v = x_last + (x_last - xr[2 * (n - 1) - p]);      // n - 1 - m, m = p - (n - 1) <= L
    s_x[j] = v;
  }
  for (int d = threadIdx.x; d < L; d += blockDim.x) s_inv[d] = (float)(1.0 / (double)(d + 1));
  __syncthreads();
  const float fL = (float)L;
  float* yr = y + row * y_row_stride;
#pragma unroll
  for (int u = 0; u < kDerivTile / 256; ++u) {
    const int o = threadIdx.x + 256 * u;
    const int64_t i = t0 + o;
    if (i >= n) break;
    const float* c = s_x + L + o;
    const float xi = c[0];
    float acc = 0.f;
    for (int d = 1; d <= L; ++d) {
      const float g = (s_inv[d - 1] * ((c[d] - xi) + (xi - c[-d]))) * 0.5f;
      acc += g / fL;
    }
    yr[i] = acc;
  }
}

static int rows_ok(const char* what, const void* x, int64_t x_row_stride, int32_t batch, int64_t n, const void* y, int64_t y_row_stride,
                   int64_t n_y) {
  MMK_TRY(rows_check(what, x, x_row_stride, batch, n, y, y_row_stride, n_y, false));
  if (batch > 65535) return fail(MMK_ERR_UNSUPPORTED, "%s: %d rows are more than one launch takes (65535)", what, batch);
  return MMK_OK;
}

}  // namespace mmk

extern "C" int mmk_interp1d_f32(const float* x, int64_t x_row_stride, int32_t batch, int64_t n, float* y, int64_t y_row_stride, int64_t n_out,
                                int32_t mode, int32_t align, mmk_stream_t stream) {
  using namespace mmk;
  MMK_TRY(rows_ok("interp1d", x, x_row_stride, batch, n, y, y_row_stride, n_out));
  if (n < 2 || n_out < 1) return fail(MMK_ERR_INVALID, "interp1d: needs n >= 2 knots and n_out >= 1 points, got %lld and %lld", (long long)n, (long long)n_out);
  if (mode < 0 || mode > 1 || align < 0 || align > 1 || (mode == 1 && align == 0))
    return fail(MMK_ERR_INVALID, "interp1d: mode %d / align %d (linear = 0 with either alignment, previous = 1 with align = 1)", mode, align);
  const double step = n_out > 1 ? (double)(n - 1) / (double)(n_out - 1) : 0.0;      // np.linspace: delta / div
  const float scale = (float)n / (float)n_out;
  int64_t blocks = (n_out + 255) / 256;
  blocks = blocks > 4096 ? 4096 : blocks;
  const dim3 grid((unsigned)blocks, (unsigned)batch), wg(256);
  hipStream_t st = (hipStream_t)stream;
  if (align == 0) return launch(interp1d_kernel<0, 0>, grid, wg, 0, st, x, x_row_stride, n, y, y_row_stride, n_out, step, scale);
  if (mode == 0) return launch(interp1d_kernel<1, 0>, grid, wg, 0, st, x, x_row_stride, n, y, y_row_stride, n_out, step, scale);
  return launch(interp1d_kernel<1, 1>, grid, wg, 0, st, x, x_row_stride, n, y, y_row_stride, n_out, step, scale);
}

extern "C" int mmk_derivative_f32(const float* x, int64_t x_row_stride, int32_t batch, int64_t n, int32_t max_lag, float* y,
                                  int64_t y_row_stride, mmk_stream_t stream) {
  using namespace mmk;
  MMK_TRY(rows_ok("derivative", x, x_row_stride, batch, n, y, y_row_stride, n));
  if (max_lag < 1) return fail(MMK_ERR_INVALID, "derivative: max_lag must be at least 1, got %d", max_lag);
  if (max_lag > kDerivMaxLag) return fail(MMK_ERR_UNSUPPORTED, "derivative: max_lag = %d, the limit is %d", max_lag, kDerivMaxLag);
  if (n <= max_lag) return fail(MMK_ERR_INVALID, "derivative: the odd reflection of max_lag = %d needs more than %d samples, got %lld", max_lag, max_lag, (long long)n);
  const int64_t n_tiles = (n + kDerivTile - 1) / kDerivTile;
  if (n_tiles * batch > 0x7fffffffLL)
    return fail(MMK_ERR_UNSUPPORTED, "derivative: %lld tiles of %d samples are more than one launch takes", (long long)(n_tiles * batch), kDerivTile);
  return launch(derivative_kernel, dim3((unsigned)(n_tiles * batch)), dim3(256), 0, (hipStream_t)stream, x, x_row_stride, n, (int)max_lag, n_tiles, y,
                y_row_stride);
}
