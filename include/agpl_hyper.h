/*
 * agpl_hyper.h -- C ABI of libagpl_hyper.so: the gradient of the sweep's bound with respect to the kernel hyperparameters (the ARD
 * lengthscales and the variance) of a plan made from raw inputs (include/agpl_se.h, include/agpl_kernels.h), at the plan's q(v).
 *
 * An extension of libagpl.so (include/agpl.h): it links against libagpl.so, takes the plans agpl_plan_create_se /
 * agpl_plan_create_stationary return and keeps agpl.h's conventions -- int32 status, device pointers, the context's stream, errors
 * through agpl_last_error of the context.  Kept in its own library so that agpl.h / libagpl.so stay the 45 entry points of
 * AGPL_VERSION 121 and the other six extension libraries their own.
 */
#ifndef AGPL_HYPER_H
#define AGPL_HYPER_H

#include "agpl.h"

#ifdef __cplusplus
extern "C" {
#endif

/*
 * The objective, for a plan made from (x, z, ell, variance, jitter, kind, param) that holds q(v) = N(m, S), S = U'U, m = U'v
 * (agpl_plan_state), and the expected potential / precision beta_li, gamma_li of a pass (beta_out / gamma_out of agpl_cavi_pass_plan):
 *     Lb(theta) = sum_l sum_i [ beta_li mu_li - gamma_li (mu_li^2 + var_li) / 2 ]
 *     mu_li = mu0_li + phi_i' m_l,   var_li = variance - |phi_i|^2 + phi_i' S_l phi_i,   phi_i = L^-1 k_Z(x_i),  K_ZZ + jitter I = L L'
 * with m, S, beta, gamma, mu0, z, jitter and the kernel's parameter held fixed: the theta-dependent part of the augmented bound the
 * sweep maximises over q(v) (docs/src/index.md:154-163 of the reference; both KL terms are constant in the whitened
 * parametrisation).  The residual variance - |phi_i|^2 is NOT clamped at 0 here (the plan's stored residual is): the gradient is
 * that of the unclamped expression.
 *   grad_out  : float64 [D + 1], device:  dLb / d log ell_d (d < D), then dLb / d log variance.
 *   x         : [N][D] float64, device -- the x the plan was made from (N must be the plan's N); mu0 [L][N] float32 or NULL;
 *               beta, gamma [L][N] float32.
 *   G, g      : [L][M][M], [L][M] float64 (M: the caller's feature count), the naturals G_l = Phi Diag(gamma_l) Phi', g_l = Phi beta_l
 *               of the same pass (summed over ranks: what the sweep exchanges), or both NULL.
 * Two parts.  The POINTS' part (always, over the N local points) differentiates k_Z(x_i) and the variance with L held fixed:
 *     dLb / dk_Z(x_i) = gamma_li C_l phi_i + b_li p_l,   C_l = L^-T (I - S_l - m_l m_l'),  p_l = L^-T m_l,  b_li = beta_li - gamma_li mu0_li
 *     grad[log ell_d]    += sum_a (gamma_i R_ai + b_i p_a) (-variance kappa'(r_ai) / r_ai) ((x_id - z_ad) / ell_d)^2,   R = C_l Phi
 *     grad[log variance] += sum_a (gamma_i R_ai + b_i p_a) k_ai  -  gamma_i variance / 2
 * The K_ZZ part (the dependence through L) is M x M work in float64: with A = sum_l (I - S_l) G_l + m_l (gt_l - G_l m_l)',
 * gt_l = sum_i b_li phi_i, Lbar = -tril(L^-T A), Kbar = sym(L^-T Phi(L' Lbar) L^-1) (the reverse rule of the Cholesky
 * factorisation, Phi = lower triangle with the diagonal halved) and grad += sum_ab Kbar_ab dK_ZZ,ab / dtheta (the variance sees
 * K_ZZ without the jitter).  The sweep's g carries no prior-mean correction (g_l = Phi beta_l), so gt_l = g_l - h_l with
 * h_l = sum_i gamma_li mu0_li phi_i.  A is linear in (G, g, h): the call adds the (G, g) terms when G, g are given and the -m_l h_l'
 * term of ITS OWN points when mu0 is given.  In a run that shards N, ONE rank passes the exchanged G, g, every rank passes its own
 * points, and the D + 1 numbers summed over ranks are the gradient.
 *   kappa'(r)/r : agpl_kernel_rules.h, once per kind, in closed form, with its limit at r = 0 where it has one; the Matern-1/2
 *               kernel has none (kappa is not differentiable at 0) and 0 is used there.
 *   features  : the plan's own generator at the plan's own scale, in chunks of 65536 points whose marginal image goes to the plan's
 *               prediction scratch (agpl_plan_predict's; grown here if needed, freed with the plan): bit for bit the features
 *               agpl_plan_features decodes.  Nothing else the plan holds is written.
 *   numerics  : L^-1 in float64 as the plan's creation forms it (K_ZZ in float64, the library's float64 factor route), from the
 *               scaled inducing inputs z / ell the plan holds; C_l, p_l in float64 once per call; C_l packed as split float16 with
 *               a power-of-two scale per latent, R = C_l Phi on the matrix cores (v_mfma_f32_32x32x16_f16: hi hi + hi lo + lo hi,
 *               float32 accumulation) and contracted in the same kernel with kappa and kappa'/r regenerated in float32 (r^2 in
 *               float64): R never reaches memory.  Products and sums after that are float64; per-workgroup partial sums are
 *               float64 and reduced in a fixed order, without float atomics: two calls on the same inputs give the same bits.
 *   errors    : a plan not made from raw inputs, a plan with AGPL_PLAN_NO_MARGINALS, N != the plan's N, a null plan / x / beta /
 *               gamma / grad_out, exactly one of G, g -> AGPL_ERR_INVALID_ARGUMENT; a non-finite x -> AGPL_ERR_DOMAIN with its
 *               index (grad_out is then not meaningful).  The context stays usable after every error.
 *   The call waits once, at its end (the domain check of x).                                                                     */
AGPL_API int32_t agpl_plan_hyper_grad(agpl_plan *plan, int64_t N, const double *x, const float *mu0, const float *beta,
                                      const float *gamma, const double *G, const double *g, double *grad_out);

#ifdef __cplusplus
}
#endif
#endif /* AGPL_HYPER_H */
