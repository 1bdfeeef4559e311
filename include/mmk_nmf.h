/* libmmk_hip: the non-negative matrix factorisation's entry points (csrc/nmf.hip; mimikit_amd/features/functionals.py NMF).
 *
 * A header of its own beside mmk.h, whose conventions hold here unchanged: raw device pointers and strides in ELEMENTS, every call
 * enqueues on `stream`, 0 = MMK_OK or a negative MMK_ERR_* with the text in mmk_last_error().  MMK_ABI_VERSION does not change: these
 * are additions, and the binding types them from a table of its own (native.NMF_SYMBOLS).
 *
 * X ~ W H with X (n, d) >= 0, W (n, k) >= 0 and H (k, d) >= 0, as sklearn.decomposition.NMF(init=None -> "nndsvda", solver="cd",
 * beta_loss="frobenius", no regularisation, no shuffle) computes it.  H is kept TRANSPOSED: ht (d, k), as sklearn's solver keeps it.
 *
 * Common to the entry points:
 *   - x is n rows of d floats, x_row_stride >= 0 floats apart, 4-byte aligned; w (n, k) and ht (d, k) are contiguous float64, 8-byte
 *     aligned like every workspace; everything is float64 inside, x is converted while it is loaded;
 *   - 1 <= k <= MMK_NMF_MAX_COMPONENTS, d <= MMK_NMF_MAX_D (beyond the two limits: MMK_ERR_UNSUPPORTED); the start also needs
 *     k <= min(n, d), the sweeps do not (a transform of fewer rows than components is one);
 *   - tails are masked in the kernels, the caller pads nothing; nothing but the stated outputs and the workspace is written;
 *   - no atomics, no workgroup waits for another; every sum has one order that depends on the sizes alone, so two calls give the same
 *     bits.  NaN and inf are not handled.
 *   - streams: the two half-sweeps return without waiting.  mmk_nmf_start_f64 waits for `stream` (inside mmk_pca_eig_f64, and once more
 *     to read the smallest entry and the eigenvalues); mmk_nmf_solve_f64 waits every `poll` iterations to read its convergence flag.
 *     Neither can be captured into a graph.
 */
#ifndef MMK_NMF_H_
#define MMK_NMF_H_

#include "mmk.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MMK_NMF_MAX_D MMK_PCA_MAX_D                   /* the Gram matrix and its eigenpairs come from the PCA kernels */
#define MMK_NMF_MAX_COMPONENTS MMK_PCA_MAX_COMPONENTS /* a row of W and a row of X H^T live in one lane's registers */
#define MMK_NMF_POLL 8                                /* poll = 0: the host reads the convergence flag every 8 iterations */
#define MMK_NMF_EPS 1e-6                              /* the cut of sklearn's _initialize_nmf: the literal, not a machine epsilon */
#define MMK_NMF_RANK_MARGIN 64.0                      /* see mmk_nmf_start_f64 */

/* The NNDSVDA start of sklearn's _initialize_nmf from the k leading eigenpairs (lambda_j, v_j) of G = X^T X:
 *     G by mmk_pca_cov_f64 (mean 0, scale 1), the pairs by mmk_pca_eig_f64;  S_j = sqrt(lambda_j), u_j = X v_j / S_j;
 *     column 0: sqrt(S_0) |u_0|, sqrt(S_0) |v_0|;  column j >= 1: the positive parts of u_j and v_j if the product of their norms is
 *     STRICTLY larger than that of the negative parts', else the negative parts; each normalised, then scaled by sqrt(S_j m);
 *     entries < MMK_NMF_EPS become 0, zeros become mean(X).
 *   w (n, k), ht (d, k)   the start
 *   s (k), v (k, d)       the singular values and right singular vectors it was made from (the signs are mmk_pca_eig_f64's)
 *   part (k) int32        1: the positive parts were taken, 0: the negative ones, 2: absolute values (column 0)
 * MMK_ERR_INVALID when x has a negative entry, n < 2, or lambda_{k-1} <= MMK_NMF_RANK_MARGIN ((n + 2) 2^-53 + MMK_PCA_TOL sqrt(d)) lambda_0:
 * the Gram sum rounds lambda by up to (n + 2) 2^-53 lambda_0, the eigen step stops at a residual of MMK_PCA_TOL |G|_inf <= MMK_PCA_TOL sqrt(d)
 * lambda_0, and a singular pair below 64 times the two is not determined by the frames (all-zero frames included).
 * Workspace: mmk_nmf_start_workspace_bytes(n, d, k). */
size_t mmk_nmf_start_workspace_bytes(int64_t n, int32_t d, int32_t k);
int mmk_nmf_start_f64(const float* x, int64_t x_row_stride, int64_t n, int32_t d, int32_t k, double* w, double* ht, double* s, double* v,
                      int32_t* part, void* workspace, size_t workspace_bytes, mmk_stream_t stream);

/* One half-sweep of sklearn's _update_cdnmf_fast, cyclic, without shuffle.  The W half, with B = ht and A = w:
 *     G = B^T B (k, k), P = X B (n, k);  for every row i, for t = 0 .. k-1 in order:
 *         g = -P[i,t] + sum_r G[t,r] A[i,r];   violation += |W[i,t] == 0 ? min(0, g) : g|;   if G[t,t] != 0: A[i,t] = max(A[i,t] - g / G[t,t], 0)
 * P is never written: a workgroup forms the rows of X B that its lanes sweep.  The H half is the same with X^T, B = w and A = ht; X^T B is
 * summed over runs of rows whose partial sums are added in rising run order.
 *   violation  one float64: the half-sweep's sum, the workgroups' partial sums added in a fixed order by a second launch.
 * Workspace of either: mmk_nmf_half_workspace_bytes(n, d, k). */
size_t mmk_nmf_half_workspace_bytes(int64_t n, int32_t d, int32_t k);
int mmk_nmf_w_half_f64(const float* x, int64_t x_row_stride, int64_t n, int32_t d, int32_t k, const double* ht, double* w, double* violation,
                       void* workspace, size_t workspace_bytes, mmk_stream_t stream);
int mmk_nmf_h_half_f64(const float* x, int64_t x_row_stride, int64_t n, int32_t d, int32_t k, const double* w, double* ht, double* violation,
                       void* workspace, size_t workspace_bytes, mmk_stream_t stream);

/* sklearn's _fit_coordinate_descent from (w, ht), in place: iterations 1 .. max_iter of a W half, an H half (update_h != 0; 0 is
 * sklearn's transform, which the caller starts from w = 0) and the stop test
 *     violation_1 == 0  or  violation_it / violation_1 <= tol.
 * A device flag takes the iteration that met it; every kernel of a later iteration returns at once, so w and ht are frozen there
 * whenever the host looks: it reads the flag every `poll` iterations (0: MMK_NMF_POLL) and after the last.
 *   n_iter        the flag's value, or max_iter if the test was never met (sklearn's n_iter_)
 *   check_nonneg  != 0: the smallest entry of x is reduced first and a negative one is MMK_ERR_INVALID (w and ht are then undefined)
 * max_iter >= 1, tol >= 0.  Workspace: mmk_nmf_solve_workspace_bytes(n, d, k). */
size_t mmk_nmf_solve_workspace_bytes(int64_t n, int32_t d, int32_t k);
int mmk_nmf_solve_f64(const float* x, int64_t x_row_stride, int64_t n, int32_t d, int32_t k, double* w, double* ht, int32_t update_h, double tol,
                      int32_t max_iter, int32_t poll, int32_t check_nonneg, int32_t* n_iter, void* workspace, size_t workspace_bytes,
                      mmk_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* MMK_NMF_H_ */
