/*
 * agpl_predictive.h -- C ABI of libagpl_predictive.so: the predictive distribution of y at new inputs and the log predictive
 * density of held-out observations, from the marginals q(f) = N(mu, var) that agpl_plan_predict / agpl_marginals_plan return.
 *
 * An extension of libagpl.so (include/agpl.h): it links against libagpl.so, takes its contexts and likelihood descriptors, and
 * keeps agpl.h's conventions -- int32 status, device pointers, the context's stream, errors through agpl_last_error of the
 * context.  Kept in its own library so that agpl.h / libagpl.so stay the 45 entry points of AGPL_VERSION 121 and agpl_se.h /
 * libagpl_se.so their four.
 */
#ifndef AGPL_PREDICTIVE_H
#define AGPL_PREDICTIVE_H

#include "agpl.h"

#ifdef __cplusplus
extern "C" {
#endif

/*
 * agpl_predictive: per point i, with q(f_i) = N(mu_i, var_i) (independent over the latents of a multi-latent likelihood),
 *     mean_out[i] = E[y],  var_out[i] = Var[y]  under p(y) = int p(y | f) q(f) df,      logp_out[i] = log p(y_i),
 *     *logp_sum   = sum_i logp_out[i]
 * for the likelihoods p(y | f) that agpl_synth_xy samples from and agpl_logtilt with the auxiliary prior integrates to:
 *     Bernoulli       sigma((2y - 1) f)                                   mean p = E sigma(f), variance p (1 - p)
 *     NegBinomial(r)  Gamma(y + r) / (y! Gamma(r)) sigma(f)^y sigma(-f)^r lognormal moments: r E e^f,
 *                                                                         r (E e^f + E e^2f) + r^2 (E e^2f - (E e^f)^2)
 *     StudentT        Student-t, nu d.o.f., location f, scale sigma       mu (NaN for nu <= 1), var + sigma^2 nu / (nu - 2) (+inf
 *                                                                         for nu <= 2)
 *     Poisson(lambda) Poisson(y; lambda sigma(f))                         lambda E sigma, lambda E sigma + lambda^2 Var sigma
 *     Laplace(beta)   exp(-|y - f| / beta) / (2 beta)                     mu, var + 2 beta^2
 *     HeteroGauss     N(y; f, 1 / (lambda sigma(g))), latents (f, g)      mu_f, var_f + (1 + exp(-mu_g + var_g / 2)) / lambda
 *     Binomial(n)     C(n, y) sigma(f)^y sigma(-f)^(n - y)                n E sigma, n (E sigma - E sigma^2) + n^2 Var sigma;
 *                                                                         log p by the count rule with exponents (y, n - y); a
 *                                                                         count outside 0 .. n has log p = -inf (AGPL_LIK_BINOMIAL)
 *     AsymLaplace(sigma, tau)  tau (1 - tau) / sigma exp(-rho_tau((y - f) / sigma)), rho_tau(u) = u (tau - 1[u < 0]) (AGPL_LIK_ASYMLAPLACE):
 *                     mu + sigma (1 - 2 tau) / (tau (1 - tau)), var + sigma^2 (1 - 2 tau + 2 tau^2) / (tau (1 - tau))^2;  log p in closed
 *                     form as Laplace's, the two exponential x Phi products with a rate each (a = tau / sigma, b = (1 - tau) / sigma)
 *                     through the scaled erfc; var = 0 gives the likelihood's own log density
 *     LogisticNoise(s)  sech^2((y - f) / 2 s) / (4 s) (AGPL_LIK_LOGISTIC_NOISE):  mu, var + s^2 pi^2 / 3;  log p = -log s +
 *                     log E sigma(g) sigma(-g), g ~ N((y - mu) / s, var / s^2), by the count rule at the exponent pair (1, 1) (never as
 *                     E sigma - E sigma^2, which cancels in the tails); var = 0 gives the likelihood's own log density
 *     Categorical     theta_k sigma(f_k) / sum_j theta_j sigma(f_j), theta = exp(logtheta); the bijective link adds class L with the
 *                     constant weight theta_L / 2.  mean_out = the class probabilities [n][K] (K = nlatent, + 1 if bijective),
 *                     var_out is not written, logp = log of the probability of the observed class (an all-zero one-hot row of
 *                     the bijective link means class L).
 *   arguments : mu, var float64 [n], or [n][L] point-major (L contiguous per point), as the float64 operators of agpl.h take q(f);
 *               y in the operator layout of agpl.h (uint8 / int32 / float64; one-hot uint8 [n][L]) or NULL: logp_out and logp_sum
 *               need y; mean_out, var_out, logp_out ([n] each) and logp_sum (ONE DEVICE double) may each be NULL.
 *   numerics  : float64, one lane per point.  Bernoulli, NegBinomial, Poisson and (over g, with f integrated analytically) the
 *               heteroscedastic Gaussian: the mode of p(y | f) q(f) from a 65-point grid over mu +- 8 s and safeguarded Newton steps,
 *               then a trapezoid rule centred on it over +- 8 s, spaced by half the peak's width, at most s / 4 and at most 0.5
 *               (the integrands have poles at distance pi from the real axis); E sigma and E sigma^2 by the same rule centred on
 *               mu.  StudentT: the Gamma scale mixture of the augmentation, a trapezoid rule in the logarithm of the mixing
 *               variable centred on the integrand's maximum, spaced by half its width and at most 0.5, marched out until the
 *               terms fall below exp(-30) of the largest.  Laplace: closed form (scaled erfc).  A mode beyond the grid (a
 *               likelihood that pulls it more than 8 s from mu) is followed by moving the grid.  var = 0 gives log p(y | mu)
 *               exactly.
 *   domain    : the supported domain is the grid of tests/predictive_domain.py: s = sqrt(var) from 1e-8 to 50,
 *               |mu| <= 40 (Bernoulli, NegBinomial: down to -300); StudentT nu from 0.01 to 1e6, sigma from 1e-3 to 1e3, residuals
 *               up to 50 predictive standard deviations; counts up to 2^31 - 1, r from 1e-3 to 1e4, lambda from 1e-6 to 1e6;
 *               HeteroGauss var_g <= 100, mu_g in [-30, 30]; Laplace beta from 1e-3 to 10, var <= 400, |y - mu| <= 3000 beta.
 *               There log p(y) is within 1e-4 of adaptive float64 integration (measured worst: 3e-6) and the moments within
 *               1e-5 relative (DESIGN.md 4.23 names the points).  Accuracy outside the domain is not promised.  A NegBinomial
 *               mean that overflows has variance +inf.
 *               Categorical: Monte Carlo with `nsamples` draws of f per point (0 = 4096; fewer than 16 or more than 2^20 is
 *               AGPL_ERR_INVALID_ARGUMENT), normalised per draw so that a row sums to 1; the normal of (draw j, latent k) of point
 *               i is block j of sub-stream 1 + k of the Philox stream (seed, point_offset + i, sweep) of agpl.h: a pure function
 *               of the context's seed, the point's global index and `sweep`.  nsamples and sweep are ignored otherwise.
 *   edge cases: a negative or non-finite var or a non-finite mu gives NaN in every output of that point (not an error); a count
 *               y < 0 gives logp = -inf; a one-hot row without a class (non-bijective link) gives logp = -inf.
 *   logp_sum  : two-level float64 reduction in a fixed order (per workgroup, then over at most 1024 workgroup sums): bit-identical
 *               from call to call for the same n; NaN points propagate.
 *   Asynchronous on the context's stream.  The first call on a context may allocate 8 KB of device memory for the workgroup sums
 *   (shared with agpl_cavi_pass_plan's ELBO terms, freed by agpl_ctx_destroy); later calls allocate nothing.
 *   Errors: null context / descriptor / mu / var, n < 0, logp outputs without y, parameters outside the likelihood's domain,
 *   bad nsamples -> AGPL_ERR_INVALID_ARGUMENT.                                                                              */
AGPL_API int32_t agpl_predictive(agpl_ctx *ctx, const agpl_lik_desc *lik, int64_t n, const double *mu, const double *var,
                                 const void *y, uint32_t nsamples, uint32_t sweep, double *mean_out, double *var_out,
                                 double *logp_out, double *logp_sum);

#ifdef __cplusplus
}
#endif
#endif /* AGPL_PREDICTIVE_H */
