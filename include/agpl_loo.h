/*
 * agpl_loo.h -- C ABI of libagpl_loo.so: the leave-one-out cavity of a plan's q(v) at the training points (Opper & Winther 2000;
 * Vehtari, Mononen, Tolvanen, Sivula, Winther 2016).  agpl_plan_update forms
 *     q(v) ~ N(v; 0, I) exp(eta0'v) prod_i exp(beta_i phi_i'v - gamma_i (phi_i'v)^2 / 2),   S = (I + G)^-1, m = S (g + eta0),
 * one site per (point, latent).  Taking site i out of q(v) is a rank-one downdate of I + G, and the marginal of f_i under what is left --
 * the cavity -- follows from the marginal under q(v) by Sherman-Morrison: with q_i = phi_i'S phi_i = var_i - d_i (d the plan's Nystrom
 * residual), a_i = phi_i'm = mu_i - mu0_i and the leverage h_i = gamma_i q_i,
 *     var_-i = d_i + q_i / (1 - h_i),        mu_-i = mu0_i + (a_i - beta_i q_i) / (1 - h_i),
 * what a refit with S_-i = (I + G - gamma_i phi_i phi_i')^-1, m_-i = S_-i (g + eta0 - beta_i phi_i) gives.  The sum of the leverages
 * of a latent is tr(G S) = M - tr S, its effective number of parameters.  The outputs are in the layout agpl_predictive
 * (include/agpl_predictive.h), agpl_predictive_cdf (include/agpl_quantile.h) and the float64 operators take, so that log p(y_i | y_-i),
 * the LOO probability integral transform and the LOO moments of y are those entry points at the cavity.
 *
 * An extension of libagpl.so (include/agpl.h): it links against libagpl.so and keeps agpl.h's conventions -- int32 status, device
 * pointers, the context's stream, errors through agpl_last_error of the plan's context.  Kept in its own library so that agpl.h /
 * libagpl.so stay the 45 entry points of AGPL_VERSION 121 and the other extension libraries their own.
 *
 * THE RULE (stated once, here).  agpl_plan_loo runs agpl_marginals_plan(plan, mu0, mu, var) into the work area and then, for every
 * (point i, latent l), from the float32 numbers mu = mu[l][i], var = var[l][i], d = the plan's residual[i] (agpl_plan_state),
 * m0 = mu0[l][i] (0 without mu0), g = gamma[l][i], b = beta[l][i], each converted to float64 (exactly), in IEEE float64 arithmetic,
 * every operation rounded once, nothing fused, in this order:
 *     q = var - d;  if (!(q > 0)) q = 0          (q negative by round-off is 0)
 *     a = mu - m0
 *     h = g * q
 *     t = 1 - h
 *     var_out = d + q / t
 *     u = b * q;  w = a - u;  mu_out = m0 + w / t
 *     lev_out = h
 * The pair HAS NO CAVITY if g, b, mu or var is not finite, g < 0, or !(h < 1): then var_out = mu_out = lev_out = NaN, the pair is
 * counted in `info` and left out of `lev_sum`; it is not an error.  (The test on q comes after the one on var, so a NaN never reaches it.)
 *
 *   case                                                    | result
 *   --------------------------------------------------------+------------------------------------------------------------------------
 *   g = 0 (b anything finite)                               | the rule as it stands: h = 0, t = 1, both divisions exact -- the cavity is
 *                                                           | the marginal with the linear site taken out, mu_out = m0 + (a - b q),
 *                                                           | var_out = d + q
 *   h >= 1, g < 0, or a non-finite g, b, mu or var          | NaN in all three outputs of that pair; counted in info; not an error
 *   q negative by round-off                                 | 0 (the cavity is the prior's: var_out = d, mu_out = m0 + a)
 *   a plan created with AGPL_PLAN_NO_MARGINALS; a null      | AGPL_ERR_INVALID_ARGUMENT with a message (a null plan: the status alone,
 *   plan, gamma, beta, mu_out or var_out; a null or short   | there is no context to carry one)
 *   work                                                    |
 * At a q(v) made by agpl_plan_update from the same gamma, h < 1 always holds (I + G - gamma_i phi_i phi_i' is positive definite), so
 * h >= 1 means that the caller's sites are not those of the plan's q(v).
 *
 * lev_sum[l] = the sum over the points WITH a cavity of h, in float64 in a fixed order: a wave of 64 consecutive points is summed by the
 * butterfly s += shfl_xor(s, o), o = 32, 16, .., 1 (a point without a cavity enters as +0); a workgroup of 256 lanes takes the
 * 256-point tiles b, b + B, b + 2 B, .. (B = min(ceil(N / 256), 1024) workgroups), wave w the points 64 w .. 64 w + 63 of each, and
 * every wave adds the sums of its quarter-tiles in that order into one accumulator starting from 0; the workgroup's partial is
 * ((w0 + w1) + w2) + w3 of the four accumulators; the second level sums the B
 * partials as agpl_predictive's logp_sum does (lane j of 256 adds partials j, j + 256, .. ascending, then a halving tree 128, 64, .., 1).
 * No float atomics: the bits are the same from call to call.
 *
 * The work area (caller-owned device memory, agpl_plan_loo_bytes(N, L) bytes, 256-byte aligned), in this order:
 *     mu       float32 [L][N]        at byte 0
 *     var      float32 [L][N]        at byte al(4 L N),  al(x) = x rounded up to a multiple of 256
 *     partials float64 [L][1024]     at byte 2 al(4 L N)
 * After the call it holds agpl_marginals_plan's output for (plan, mu0).  The call allocates nothing.
 */
#ifndef AGPL_LOO_H
#define AGPL_LOO_H

#include "agpl.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The bytes of the work area for N points and L latents (a pure host function); 0 for sizes a plan does not take (N < 1, L outside
 * [1, 64]).                                                                                                                          */
AGPL_API int64_t agpl_plan_loo_bytes(int64_t N, int32_t L);

/*
 * The cavity of every (point, latent) of the plan, THE RULE above.  Asynchronous on the context's stream.
 *   mu0          : float32 [L][N] or NULL, as agpl_marginals_plan takes it
 *   gamma, beta  : float32 [L][N], the sites of the q(v) the plan holds (gamma_out / beta_out of the agpl_cavi_pass_plan whose G, g
 *                  agpl_plan_update was given)
 *   work         : the work area; work_bytes >= agpl_plan_loo_bytes(N, L) of the plan's N, L
 *   mu_out, var_out : float64 [N][L], point-major
 *   lev_out      : float64 [N][L], the leverages h; may be NULL
 *   lev_sum      : float64 [L]; may be NULL
 *   info         : int64 [2]; may be NULL.  Word 0: the number of pairs without a cavity; word 1: the lowest flat index l N + i of
 *                  one, -1 if there is none
 * Errors: the last row of the table; whatever agpl_marginals_plan reports.                                                          */
AGPL_API int32_t agpl_plan_loo(agpl_plan *plan, const float *mu0, const float *gamma, const float *beta, void *work,
                               int64_t work_bytes, double *mu_out, double *var_out, double *lev_out, double *lev_sum, int64_t *info);

#ifdef __cplusplus
}
#endif
#endif /* AGPL_LOO_H */
