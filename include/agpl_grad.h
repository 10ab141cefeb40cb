/*
 * agpl_grad.h -- C ABI of libagpl_grad.so: the posterior of the GRADIENT of f at new inputs under a plan's q(v) -- the marginal
 * mean and variance of every partial derivative d f_l / d x_d -- for plans made from raw inputs (include/agpl_se.h,
 * include/agpl_kernels.h).  The derivative of a GP is a GP, so this is a closed-form Gaussian: no difference quotient of
 * agpl_plan_predict can give it (its float32 outputs carry about 2e-5 of relative error, and the variance of a derivative is not a
 * difference of variances at all).
 *
 * An extension of libagpl.so (include/agpl.h): it links against libagpl.so, takes the plans agpl_plan_create_se /
 * agpl_plan_create_stationary return and keeps agpl.h's conventions -- int32 status, device pointers, the context's stream, errors
 * through agpl_last_error of the context.  Kept in its own library so that agpl.h / libagpl.so stay the 45 entry points of
 * AGPL_VERSION 121 and the other extension libraries their own.
 */
#ifndef AGPL_GRAD_H
#define AGPL_GRAD_H

#include "agpl.h"

#ifdef __cplusplus
extern "C" {
#endif

/*
 * For a plan of (x, z, ell, variance = sigma^2, jitter, kind, param) with K_ZZ + jitter I = L L' and q(v) = (U_l, v_l), S_l = U_l' U_l,
 * m_l = U_l' v_l; u_ad = (x_d - z_ad) / ell_d, r^2 = sum_d u_ad^2, and c = -lim_{r -> 0} kappa'(r) / r (1 for the squared exponential
 * and the rational quadratic, 3 for Matern-3/2, 5/3 for Matern-5/2): the prior variance of d f / d x_d is c sigma^2 / ell_d^2.
 * In a dimension whose distance a kind warps (include/agpl_kernels.h: every dimension of AGPL_KERNEL_PERIODIC, the last one of
 * AGPL_KERNEL_SE_PERIODIC) u_ad is sin(pi (x_d - z_ad) / p) / ell_d, d k / d x_d gains the factor (pi / p) cos(pi (x_d - z_ad) / p) and
 * c the factor (pi / p)^2 -- per dimension: an AGPL_KERNEL_SE_PERIODIC plan has c = 1 for d < D - 1 and (pi / p)^2 for the last.
 * AGPL_KERNEL_SE_COSINE (k = sigma^2 E m, E = exp(-r^2 / 2), m = cos(2 pi (x_{D-1} - z_{a,D-1}) / p)) warps nothing; its derivative has a
 * product rule in the last dimension: d k / d x_d = -sigma^2 E m u_ad / ell_d for d < D - 1 and sigma^2 E (-m u_ad / ell_d -
 * (2 pi / p) sin(2 pi (x_d - z_ad) / p)) for the last, and c = 1 for d < D - 1 and 1 + (2 pi ell_d / p)^2 for the last, so that the prior
 * variance of d f / d x_d, c sigma^2 / ell_d^2, is sigma^2 / ell_d^2 and sigma^2 (1 / ell_d^2 + (2 pi / p)^2).
 *   d k(x, z_a) / d x_d = sigma^2 (kappa'(r) / r) u_ad / ell_d
 *   psi_d(x)            = (ell_d / sqrt c) L^-1 d k_Z(x) / d x_d       the normalised derivative feature: |psi_d|^2 <= sigma^2 (the
 *                                                                      Nystrom bound of the derivative process), so every
 *                                                                      |psi_ad| <= sigma -- the bound the plan's image scale is from
 *   dmu_out[l][d][i]    = (sqrt c / ell_d) psi_d(x_i)' m_l                                       = E   d f_l / d x_d (x_i)
 *   dvar_out[l][d][i]   = (c / ell_d^2) (sigma^2 - |psi_d(x_i)|^2 + |U_l psi_d(x_i)|^2)           = Var d f_l / d x_d (x_i)
 * A fresh plan (U = I, v = 0) gives 0 and the prior variance c sigma^2 / ell_d^2.
 *   outputs   : float32 [L][D][Ns] each; either may be NULL, not both.
 *   route     : chunks of 65536 points, as agpl_plan_predict.  For each chunk and each d, the plan's own generator in its derivative
 *               mode (the column sigma^2 (kappa'(r) / r) u_d / sqrt c, kappa'(r) / r the rule the hyperparameter gradient uses,
 *               whitened on the matrix cores by the same code) writes the marginal image of psi_d at the plan's own scale and the
 *               residual sigma^2 - |psi_d|^2 (agpl_plan_create's clamp) into the plan's prediction scratch (agpl_plan_predict's;
 *               grown here if needed, freed with the plan); the marginal pass of agpl_marginals_plan runs on them, and one
 *               element-wise kernel applies (sqrt c / ell_d, c / ell_d^2) into the rows [l][d].  D generator and marginal launches
 *               per chunk.
 *   numerics  : those of agpl_plan_predict on psi_d (distance in float64, the rule in float32, float32 whitening, split-float16
 *               marginal pass), then one float32 multiplication.  Fixed orders, no float atomics: a point's outputs depend on
 *               its own x only -- not on Ns, its position or the chunk -- bit for bit.  A non-finite x_s row gives NaN in that
 *               point's outputs and nothing else.  x_s equal to an inducing input (u = 0, r = 0) is an ordinary point.
 *   prior mean: the outputs are those of the zero-mean process; the gradient of a prior mean function is the caller's to add to
 *               dmu_out.
 *   errors    : a null plan, a plan not made from raw inputs, a plan with AGPL_PLAN_NO_MARGINALS (its U is not maintained;
 *               agpl_plan_predict refuses it too), Ns < 0, a null x_s or both outputs NULL with Ns > 0 -> AGPL_ERR_INVALID_ARGUMENT.
 *               A Matern-1/2 plan -> AGPL_ERR_UNSUPPORTED: that kernel is not mean-square differentiable (kappa'(r) / r has no limit
 *               at 0).  Ns = 0 -> AGPL_OK, nothing written, nothing launched.  The context stays usable after every error.
 *   The call is asynchronous on the context's stream: it does not wait on the host (growing the scratch waits for earlier work
 *   that may still use it, once).
 *   Out of scope: derivatives from a chain of inducing draws (agpl_plan_predict_chain), derivatives of pathwise draws
 *   (agpl_plan_sample_paths), the D x D covariance between the partial derivatives of a point, second derivatives.           */
AGPL_API int32_t agpl_plan_predict_grad(agpl_plan *plan, int64_t Ns, const double *x_s, float *dmu_out, float *dvar_out);

#ifdef __cplusplus
}
#endif
#endif /* AGPL_GRAD_H */
