/*
 * agpl_likgrad.h -- C ABI of libagpl_likgrad.so: the expected log-likelihood sum_i E_{q(f_i)} log p(y_i | f_i; theta) of the
 * marginals q(f) = N(mu, var) that agpl_marginals_plan / agpl_plan_predict return, and its gradient for the logarithms of the
 * likelihood's own parameters.  It is the theta-dependent term of the un-augmented sparse-GP bound
 *     F = sum_i E_{q(f_i)} log p(y_i | f_i; theta) - KL(q(v) || p(v)),
 * a lower bound for any q(f): a step on it is a valid M-step between CAVI sweeps.
 *
 * An extension of libagpl.so (include/agpl.h): it links against libagpl.so, takes its contexts and likelihood descriptors, and
 * keeps agpl.h's conventions -- int32 status, device pointers, the context's stream, errors through agpl_last_error of the
 * context.  Kept in its own library so that agpl.h / libagpl.so stay the 45 entry points of AGPL_VERSION 121.
 */
#ifndef AGPL_LIKGRAD_H
#define AGPL_LIKGRAD_H

#include "agpl.h"

#ifdef __cplusplus
extern "C" {
#endif

/*
 * agpl_expected_loglik: per point i, with q(f_i) = N(mu_i, var_i) (the heteroscedastic kind: independent q(f_i) q(g_i)),
 *     ell_out[i]       = E_q log p(y_i | f_i)
 *     dell_out[i][p]   = d ell_out[i] / d log theta_p,   p = 0 .. P - 1 (P contiguous per point)
 *     *ell_sum         = sum_i ell_out[i],      grad_sum[p] = sum_i dell_out[i][p]
 * for the densities p(y | f) that agpl_predictive documents.  P and the order of theta follow the descriptor's p[]:
 *     Bernoulli       P = 0   value only: dell_out / grad_sum must be NULL
 *     NegBinomial     P = 1   log r        r [psi(y + r) - psi(r) + E log sigma(-f)]
 *     StudentT        P = 2   log nu       nu [psi((nu + 1) / 2) / 2 - psi(nu / 2) / 2 - 1 / (2 nu) - E log1p(z^2 / nu) / 2
 *                                              + (nu + 1) / 2 E z^2 / (nu (nu + z^2))],     z = (y - f) / sigma
 *                             log sigma    -1 + (nu + 1) E z^2 / (nu + z^2)
 *     Poisson         P = 1   log lambda   y - lambda E sigma(f)
 *     Laplace         P = 1   log beta     -1 + E|y - f| / beta
 *     HeteroGauss     P = 1   log lambda   1 / 2 - lambda E sigma(g) E (y - f)^2 / 2
 *     Binomial(n)     P = 0   value only, log C(n, y) + y E log sigma(f) + (n - y) E log sigma(-f) by the Bernoulli kind's rule (n is
 *                             data, not a learnable parameter): dell_out / grad_sum must be NULL; a count outside 0 .. n gives -inf
 *     AsymLaplace(sigma, tau)  P = 1   log sigma   -1 + E|y - f| / (2 sigma) + (tau - 1/2) (y - mu) / sigma;  the value is
 *                             log(tau (1 - tau) / sigma) - E|y - f| / (2 sigma) - (tau - 1/2) (y - mu) / sigma, E|y - f| as Laplace's (tau is
 *                             the chosen level, not a parameter); a non-finite y as for Laplace
 *     LogisticNoise(s)  P = 1   log s   -1 + m (2 e1 - 1) + 2 R^2 (e1 - e2) = -1 + E[g tanh(g / 2)] (Stein's lemma), g ~ N(m, R^2),
 *                             m = (y - mu) / s, R^2 = var / s^2, e1 = E sigma(g), e2 = E sigma(g)^2;  the value is -log s + E log sigma(g)
 *                             + E log sigma(-g).  R < 1: the Bernoulli kind's rule over N(m, R^2); R >= 1 (R is not bounded by the count
 *                             kinds' s <= 50): the rule over the noise's own measure, csrc/agpl_logistic_noise.h; a non-finite y as
 *                             for Laplace (AGPL_LIK_LOGISTIC_NOISE)
 *     Categorical (both links): AGPL_ERR_INVALID_ARGUMENT.  Their expectation couples the L latents of a point and would need
 *                     Monte Carlo (as agpl_predictive uses for them); out of scope here.
 *   arguments : mu, var float64 [n], or [n][2] point-major for the heteroscedastic kind, y in the operator layout of agpl.h
 *               (uint8 / int32 / float64), as agpl_predictive takes them.  ell_out [n], dell_out [n][P], ell_sum (ONE DEVICE
 *               double) and grad_sum (P DEVICE doubles) may each be NULL.
 *   numerics  : float64, one lane per point.  Closed forms: E (y - f)^2 = d^2 + s^2 and E|y - f| = s sqrt(2 / pi) exp(-d^2 / 2 s^2)
 *               + d erf(d / (s sqrt 2)), d = y - mu, s = sqrt(var); lgamma of the device's math library; psi by recurrence to
 *               x >= 6 and the asymptotic series (no library call).  E log sigma(+-f), E sigma(f), E log1p(z^2 / nu) and
 *               E z^2 / (nu + z^2): the trapezoid rule centred on mu over mu +- 8 s, normalised by its own weights, with spacing
 *               min(s / 4, a / 4), a = the distance of the integrand's nearest complex singularity from the real axis (pi for the
 *               logistic terms, sigma sqrt(nu) for the Student-t terms; the rule's error falls as exp(-2 pi a / spacing)).
 *               At most 2048 nodes on each side of mu: enough for s / a <= 64.  Beyond that, per family:
 *                 Student-t terms, y inside mu +- 8 s: the rule runs in x, y - f = a sinh x, where the integrands are 2 log cosh x
 *                   and tanh^2 x (singular at x = +- i pi / 2 whatever s / a is) and the weight is N(a sinh x; d, s^2) cosh x:
 *                   nodes x = j h between asinh((d -+ 8 s) / a), h = min(pi / 16, 1 / (2 (|d| / s + 4))), normalised by its own
 *                   weights; at most 24 ln(32 s / a) nodes (a few hundred), and at most 1024 intervals (s / a <= 4e7; where 16 s / a
 *                   overflows, NaN).  It resolves the peak of width a at f = y: the expectations are within 1e-12 of a 30-digit
 *                   integral for s / a up to 2e5.
 *                 Student-t terms, y outside mu +- 8 s: the spacing is 8 s / 2048; the unresolved peak carries a weight below
 *                   exp(-32), and the rule is exact to rounding.
 *                 logistic terms: the spacing is 8 s / 2048 -- no error is reported -- and the accuracy degrades smoothly with
 *                   s / pi, as exp(-2 pi pi / spacing) does: s / pi > 64 is s > 201, outside the supported domain.
 *               var = 0 gives log p(y | mu) and its derivatives exactly.
 *   domain    : tests/likgrad_domain.py states the supported domain as named points: s from 1e-8 to 50 and
 *               var in {0, 1e-320, 1e-30}, mu within +-40 (-300 for the Bernoulli and NegBinomial kinds), nu from 0.01 to 1e6,
 *               sigma from 1e-3 to 1e3, s / (sigma sqrt(nu)) up to 2e5, residuals up to 50 predictive standard deviations, counts up
 *               to 2^31 - 1, r from 1e-3 to 1e4, lambda from 1e-6 to 1e6, beta from 1e-3 to 10.  On it every output is within
 *               1e-6 max(1, |value|) + 4 e^{-8 pi} T_q + 64 eps T_c of the float64 reference (T_q: the sum of |coefficient x
 *               expectation| over the terms that pass through a quadrature rule, T_c: the sum of the magnitudes of the closed-form
 *               terms).  Accuracy outside the grid's ranges is not promised.
 *   edge cases: a negative or non-finite var or a non-finite mu gives NaN in every output of that point (not an error) and the
 *               NaN propagates into the sums; a count y < 0 gives ell = -inf and NaN derivatives.  A real-valued y (Student-t,
 *               Laplace, heteroscedastic) follows the same convention: y = +-inf gives ell = -inf and NaN derivatives, y = NaN gives
 *               NaN in every output, at that point only, and the NaN reaches the sums.
 *   sums      : two-level float64 reduction in a fixed order (per workgroup of 512 lanes, then over at most 256 workgroup sums
 *               per quantity), no float atomics: bit-identical from call to call for the same n.
 *   Asynchronous on the context's stream.  The first call on a context may allocate the 8 KB of device memory for workgroup sums
 *   that agpl_predictive and agpl_cavi_pass_plan's ELBO terms share (freed by agpl_ctx_destroy); later calls allocate nothing.
 *   Errors: null context / descriptor, null mu / var / y with n > 0, n < 0, a categorical kind, dell_out / grad_sum with the
 *   Bernoulli kind, parameters outside the likelihood's domain -> AGPL_ERR_INVALID_ARGUMENT.                                */
AGPL_API int32_t agpl_expected_loglik(agpl_ctx *ctx, const agpl_lik_desc *lik, int64_t n, const double *mu, const double *var,
                                      const void *y, double *ell_out, double *dell_out, double *ell_sum, double *grad_sum);

#ifdef __cplusplus
}
#endif
#endif /* AGPL_LIKGRAD_H */
