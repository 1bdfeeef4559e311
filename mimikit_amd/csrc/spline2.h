// The quadratic interpolating spline of scipy.interpolate.interp1d(np.arange(n), y, kind="quadratic") = make_interp_spline(k = 2) with its
// not-a-knot ends, as ONE set of __device__ functions: the coefficient solve's collocation rows, the eval kernel and the two selection
// kernels of samplify.hip all go through spline2_basis, and every value of the spline through spline2_eval - the same instructions in
// the same order wherever a value is needed (no contraction: the pragma below; the one fused step is written out).
//
// Knots (scipy's _not_a_knot for an even degree: the midpoints of the sites without the first and the last):
//     t = [0, 0, 0, 1.5, 2.5, ..., n - 2.5, n - 1, n - 1, n - 1]         (n + 3 of them; n = 3: no interior knot, one parabola)
// B_j, j = 0 .. n - 1, is the degree-2 B-spline on t[j .. j + 3];  s(x) = sum_j c[j] B_j(x), and on t[l] <= x < t[l + 1] only B_{l-2}, B_{l-1}, B_l
// are not zero.  They come from de Boor's recurrence exactly as scipy's _deBoor_D runs it (divisions included), in float64.
#pragma once
#include <stdint.h>

namespace mmk {

// t[j] of the knot vector above, 0 <= j <= n + 2
__device__ __forceinline__ double spline2_knot(int64_t j, int64_t n) {
  return j <= 2 ? 0.0 : (j >= n ? (double)(n - 1) : (double)j - 1.5);
}

// the knot interval of x in [0, n - 1]: the largest l in [2, n - 1] with t[l] <= x  (x = j + f, 0 <= f < 1 exactly: l = j + 1, or j + 2 from f = 0.5 on)
__device__ __forceinline__ int64_t spline2_interval(double x, int64_t n) {
  const int64_t j = (int64_t)x;
  int64_t l = j + (x - (double)j >= 0.5 ? 2 : 1);
  l = l < 2 ? 2 : l;
  return l > n - 1 ? n - 1 : l;
}

// h[0 .. 2] = B_{l-2}(x), B_{l-1}(x), B_l(x)
__device__ __forceinline__ void spline2_basis(double x, int64_t l, int64_t n, double h[3]) {
#pragma clang fp contract(off)
  const double tm1 = spline2_knot(l - 1, n), t0 = spline2_knot(l, n), t1 = spline2_knot(l + 1, n), t2 = spline2_knot(l + 2, n);
  // j = 1: the two linear B-splines on [t0, t1)
  double w = 1.0 / (t1 - t0);                       // (t1 > t0: l is a non-empty interval)
  const double a0 = w * (t1 - x), a1 = w * (x - t0);
  // j = 2
  double h0 = 0.0, h1 = 0.0, h2 = 0.0;
  if (t1 != tm1) {
    w = a0 / (t1 - tm1);
    h0 = h0 + w * (t1 - x);
    h1 = w * (x - tm1);
  }
  if (t2 != t0) {
    w = a1 / (t2 - t0);
    h1 = h1 + w * (t2 - x);
    h2 = w * (x - t0);
  }
  h[0] = h0; h[1] = h1; h[2] = h2;
}

// position i of np.linspace(0, n - 1, n_out): i * step with step = (n - 1) / (n_out - 1) made on the host in float64 (0 for n_out = 1), the
// last one forced to n - 1 - interp1d_kernel's ALIGN 1 (envelope.hip)
__device__ __forceinline__ double spline2_pos(int64_t i, int64_t n, int64_t n_out, double step) {
#pragma clang fp contract(off)
  return (i == n_out - 1 && n_out > 1) ? (double)(n - 1) : (double)i * step;
}

// s(x) in float64: (c[l-2] h0 + c[l-1] h1) + c[l] h2, three products and two sums, each rounded
__device__ __forceinline__ double spline2_eval64(const double* __restrict__ c, int64_t n, double x) {
#pragma clang fp contract(off)
  const int64_t l = spline2_interval(x, n);
  double h[3];
  spline2_basis(x, l, n, h);
  return (c[l - 2] * h[0] + c[l - 1] * h[1]) + c[l] * h[2];
}

// the value every kernel uses: sample i of n_out, rounded to float32 once
__device__ __forceinline__ float spline2_eval(const double* __restrict__ c, int64_t n, int64_t i, int64_t n_out, double step) {
  return (float)spline2_eval64(c, n, spline2_pos(i, n, n_out, step));
}

}  // namespace mmk
