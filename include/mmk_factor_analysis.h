/* libmmk_hip: the factor analysis' entry points (csrc/factor_analysis.hip; mimikit_amd/features/functionals.py FactorAnalysis).
 *
 * A header of its own beside mmk.h, whose conventions hold here unchanged: raw device pointers, every call enqueues on `stream`,
 * 0 = MMK_OK or a negative MMK_ERR_* with the text in mmk_last_error().  MMK_ABI_VERSION does not change: these are additions, and the
 * binding types them from a table of its own (native.FACTOR_ANALYSIS_SYMBOLS).
 *
 * X ~ Z W + mean + noise with W (k, d) and a diagonal noise covariance psi (d), as sklearn.decomposition.FactorAnalysis (1.7,
 * _factor_analysis.py) fits it by EM - written in Gram form: per EM step sklearn takes the k leading singular values and right vectors of
 * Xc / (sqrt(psi) sqrt(n)), which are the k leading eigenpairs of G(psi) = S C S with C = Xc^T Xc / n and S = diag(1 / (sqrt(psi) + 1e-12)).
 * The frames enter through C alone: neither entry point takes rows, so there is no row stride here.
 *
 * Common to the entry points:
 *   - every array is contiguous float64, 8-byte aligned like every workspace; c is (d, d) and symmetric to the bit (mmk_pca_cov_f64
 *     mirrors it), components (k, d), noise_variance (d);
 *   - 1 <= k <= MMK_FA_MAX_COMPONENTS, k <= d <= MMK_FA_MAX_D (beyond the two limits: MMK_ERR_UNSUPPORTED);
 *   - tails are masked in the kernels, the caller pads nothing; nothing but the stated outputs and the workspace is written;
 *   - no atomics, no workgroup waits for another; every sum has one order that depends on the sizes alone, so two calls give the same
 *     bits.  NaN and inf are not handled (a NaN residual ends mmk_fa_fit_f64 with MMK_ERR_CONVERGENCE).
 *   - streams: mmk_fa_transform_matrix_f64 returns without waiting.  mmk_fa_fit_f64 waits for `stream` every MMK_FA_POLL inner
 *     iterations to read its state; it cannot be captured into a graph.
 */
#ifndef MMK_FACTOR_ANALYSIS_H_
#define MMK_FACTOR_ANALYSIS_H_

#include "mmk.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MMK_FA_MAX_D MMK_PCA_MAX_D                   /* the eigen step is the PCA kernels' block subspace iteration */
#define MMK_FA_MAX_COMPONENTS MMK_PCA_MAX_COMPONENTS /* its Jacobi block, and the k x k Cholesky of the transform, fit LDS */
#define MMK_FA_POLL 8                                /* the host reads the state every 8 inner iterations */
#define MMK_FA_SMALL 1e-12                           /* sklearn's SMALL: the floor of psi and the guard added to sqrt(psi) */

/* The whole EM loop on the device from c = Xc^T Xc / n (n: the number of frames, >= 2).  From psi = 1 and old = -inf, for i < max_iter:
 *     sp = sqrt(psi) + MMK_FA_SMALL;   theta, V = the k leading eigenpairs of G = c / sp_r / sp_c
 *     W = sqrt(max(theta - 1, 0))[:, None] V^T sp
 *     ll_i = -n/2 (d log 2 pi + k + sum log theta + (trace G - sum theta) + sum log psi)
 *     stop if ll_i - old < tol;   else old = ll_i, psi = max(diag(c) - sum_k W^2, MMK_FA_SMALL)
 * The eigen step is mmk_pca_eig_f64's block subspace iteration (b = min(d, k + 16) columns, Householder QR, Rayleigh-Ritz by cyclic
 * Jacobi, stop at MMK_PCA_TOL |G|_inf over the first k columns) with the product Z = S c S Q' by v_mfma_f64_16x16x4_f64; G is never
 * written, |G|_inf and trace G are recomputed from c and psi.  EM step 0 starts from the counter-based hash block, every later step from
 * the block the previous step left (Y = G_prev Q, whose span is the converged Q).  One launch sequence per inner iteration; its last
 * kernel, once the residuals meet the stop rule, forms ll and the stop test, updates psi and counts the EM step.  A device word takes
 * the EM step count at the stop and every later kernel returns at once, so the result does not depend on when the host looks.
 *   components (k, d)      W of the last EM step, each row's entry of largest magnitude (the first of equals) positive
 *   noise_variance (d)     psi: the one W was computed with when the tolerance stopped the loop, the one updated after the last W when
 *                          max_iter ran out (sklearn's for ... else)
 *   loglike (max_iter)     ll_0 .. ll_{n_iter - 1}; the rest is not written
 *   n_iter                 EM steps taken (sklearn's n_iter_)
 *   converged              1: ll_i - old < tol stopped the loop, 0: max_iter ran out
 *   inner_iters[2]         inner iterations in all, and those of EM step 0
 * An inner solve that does not meet its stop rule within MMK_PCA_MAX_ITER iterations: MMK_ERR_CONVERGENCE, the message names the EM step
 * and the residual (n_components beyond the number of factors in the frames leaves G without a gap after theta_k).
 * max_iter >= 1, tol >= 0.  Workspace: mmk_fa_fit_workspace_bytes(d, n_components). */
size_t mmk_fa_fit_workspace_bytes(int32_t d, int32_t n_components);
int mmk_fa_fit_f64(const double* c, int32_t d, int32_t n_components, int64_t n, double tol, int32_t max_iter, double* components,
                   double* noise_variance, double* loglike, int32_t* n_iter, int32_t* converged, int32_t* inner_iters, void* workspace,
                   size_t workspace_bytes, mmk_stream_t stream);

/* a (k, d) = (I + Wpsi W^T)^-1 Wpsi with Wpsi = components / noise_variance: the matrix whose product with the centred frames is sklearn's
 * FactorAnalysis.transform (mmk_pca_project_f32 with scale 1 and `a` as the components).  The k x k matrix is symmetric positive
 * definite; one workgroup factors it by Cholesky in LDS and inverts the factor, a second launch applies the inverse.  No library solver.
 * Workspace: mmk_fa_transform_matrix_workspace_bytes(d, n_components). */
size_t mmk_fa_transform_matrix_workspace_bytes(int32_t d, int32_t n_components);
int mmk_fa_transform_matrix_f64(const double* components, const double* noise_variance, int32_t d, int32_t n_components, double* a,
                                void* workspace, size_t workspace_bytes, mmk_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* MMK_FACTOR_ANALYSIS_H_ */
