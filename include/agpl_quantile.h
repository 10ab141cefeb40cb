/*
 * agpl_quantile.h -- C ABI of libagpl_quantile.so: the predictive distribution function of y at new inputs, its upper tail and its
 * quantiles, from the marginals q(f) = N(mu, var) that agpl_plan_predict / agpl_marginals_plan return -- prediction intervals,
 * exceedance probabilities and the probability integral transform of held-out observations, for the likelihoods whose predictive
 * has no "mean +- 2 sd" (Student-t with nu <= 2, Laplace, the heteroscedastic scale mixture, the skewed and discrete Poisson and
 * negative binomial, Bernoulli).
 *
 * An extension of libagpl.so (include/agpl.h): it links against libagpl.so, takes its contexts and likelihood descriptors, and
 * keeps agpl.h's conventions -- int32 status, device pointers, the context's stream, errors through agpl_last_error of the
 * context.  Kept in its own library so that agpl.h / libagpl.so stay the 45 entry points of AGPL_VERSION 121.
 */
#ifndef AGPL_QUANTILE_H
#define AGPL_QUANTILE_H

#include "agpl.h"

#ifdef __cplusplus
extern "C" {
#endif

/*
 * agpl_predictive_cdf: per point i, with q(f_i) = N(mu_i, var_i),
 *     cdf_out[i] = P(Y <= y_i),   sf_out[i] = P(Y > y_i)      under p(y) = int p(y | f) q(f) df
 * for the p(y | f) of agpl_predictive (include/agpl_predictive.h).  sf_out is computed from the upper tail itself (Phi(-z), the
 * other class's probability), not as 1 - cdf: an exceedance probability of 1e-12 keeps its digits.
 *     Bernoulli       sf(0) = E sigma(f), cdf(0) = E sigma(-f) (the predictive's rule for E sigma, at mu and at -mu); y = 1: 1 and 0
 *     StudentT        E_w Phi((y - mu) / sqrt(var + sigma^2 / w)), w ~ Gamma(nu / 2, rate nu / 2): the Gamma scale mixture of the
 *                     augmentation by the trapezoid rule in log w, spaced min(1 / sqrt(2 nu), 1 / 4), out to where the weight is
 *                     exp(-50) of its largest; nodes and weights depend on nu and sigma alone (not on the point or on y): each
 *                     workgroup forms them once, at most 2048 (enough for nu >= 0.2).  var = 0 goes through the same rule.
 *     Laplace(beta)   closed form, Phi(d / s) -+ the two exponential x Phi products, each through the scaled erfc (no overflow for
 *                     s / beta large); the tail below the location is summed from positive terms, the other is its mirror image
 *     HeteroGauss     E_g Phi((y - mu_f) / sqrt(var_f + (1 + exp(-g)) / lambda)): the trapezoid rule over mu_g +- 10 s_g, spaced
 *                     min(s_g / 4, 1 / 2), normalised by its own weights
 *     Poisson(lambda) given f, F(y | f) = Q(y + 1, lambda sigma(f)), the regularised upper incomplete gamma.  By parts,
 *                     P(Y <= y) = Q(y + 1, lambda) + int Phi((f - mu) / s) k(f) df,   P(Y > y) = int Phi((mu - f) / s) k(f) df,
 *                     k(f) = Pois(y; lambda sigma(f)) lambda sigma(f) sigma(-f): both tails are sums of positive terms.  The integral
 *                     is taken by composite 16-point Gauss-Legendre panels from the maximum of k out to exp(-60) of it, no panel
 *                     wider than s inside mu +- 10 s (where Phi steps).  var = 0 is Q(y + 1, lambda sigma(mu)) itself: the series for
 *                     x < a + 1, the modified Lentz continued fraction otherwise, at most 20000 terms each.
 *     NegBinomial(r)  given f, F(y | f) = I_{sigma(-f)}(r, y + 1).  By parts with k(f) = sigma(f)^(y+1) sigma(-f)^r / B(r, y + 1) and no
 *                     boundary term; var = 0 is the regularised incomplete beta by its continued fraction.
 *     Binomial(n)     given f, F(y | f) = I_{sigma(-f)}(n - y, y + 1) for 0 <= y < n: the NegBinomial rule at the same y with r = n - y, for
 *                     both tails; P(Y <= y) = 1 and P(Y > y) = 0 exactly for y >= n.  Quantiles: integer bisection of [0, n].
 *     AsymLaplace(sigma, tau)  closed form, a = tau / sigma, b = (1 - tau) / sigma, d = y - mu, s^2 = var:
 *                     F = Phi(d / s) - (1 - tau) exp(a^2 s^2 / 2 - a d) Phi(d / s - a s) + tau exp(b^2 s^2 / 2 + b d) Phi(-d / s - b s).
 *                     The predictive is not symmetric: the tail on y's side of mu is formed as such from the scaled erfc (the Laplace
 *                     rule's rearrangement, with the rates and weights of that side), the other is what is left of 1.  Quantiles: the
 *                     bracketing solve of the continuous kinds, started at mu with the predictive's standard deviation.
 *     LogisticNoise(s)  P(Y <= y) = E sigma(g) and P(Y > y) = E sigma(-g), g ~ N(m, R^2), m = (y - mu) / s, R = sqrt(var) / s, each
 *                     formed as such from positive terms.  R < 1: the logarithm of each by the count rule at the exponent pairs (1, 0)
 *                     and (0, 1) (its second-order expansion below R = 1e-3).  R >= 1: E_eps Phi(+-(m - eps) / R) over eps ~ Logistic(0, 1), the trapezoid rule centred on the
 *                     logistic's mode, spacing 1/2, |eps| <= 50 (csrc/agpl_logistic_noise.h).  Quantiles: the bracketing solve of the
 *                     continuous kinds, started at mu with the predictive's standard deviation.
 *     Categorical     classes have no order -> AGPL_ERR_INVALID_ARGUMENT.
 *   arguments : mu, var float64 [n] ([n][2] point-major for the heteroscedastic kind), y uint8 / int32 / float64 [n], as agpl_predictive
 *               takes them; cdf_out, sf_out float64 [n], either may be NULL (not both).
 *   randomised PIT of a discrete y: cdf(y) - cdf(y - 1) is the probability of y itself; a caller who wants u ~ U(cdf(y - 1), cdf(y))
 *               calls twice.
 *   edge cases: a negative or non-finite var or a non-finite mu gives NaN in that point's outputs (not an error, the predictive's
 *               convention); y = +inf gives (1, 0), y = -inf (0, 1), y = NaN gives NaN; a count y < 0 gives (0, 1).
 *   domain    : narrower than agpl_predictive's -- the grid of tests/quantile_domain.py: s = sqrt(var) from 1e-6
 *               to 20 and var = 0, |mu| <= 20; StudentT nu from 0.5 to 1e4, sigma from 1e-2 to 1e2; Laplace beta from 1e-2 to 10;
 *               HeteroGauss |mu_g| <= 10, var_g <= 25, lambda from 1e-3 to 1e3; thresholds out to 30 predictive scales; counts
 *               y <= 1e5, Poisson lambda from 1e-3 to 1e5, NegBinomial r from 1e-2 to 1e3.  StudentT nu < 0.2 is refused (the
 *               rule's nodes do not hold its left tail).  There cdf
 *               and sf are within 1e-8 of adaptive float64 integration, and within 1e-4 of themselves wherever they are >= 1e-12
 *               (measured worst on the grid: 3.3e-10 absolute, NegBinomial; 3.9e-7 relative, heteroscedastic).  Accuracy
 *               outside the domain is not promised.
 *   float64, one lane per point, no reductions, no allocation, asynchronous on the context's stream.
 *   Errors: null context / descriptor / mu / var / y (n > 0), both outputs null, n < 0, parameters outside the likelihood's domain,
 *   a categorical kind -> AGPL_ERR_INVALID_ARGUMENT.  n = 0 succeeds and writes nothing.                                         */
AGPL_API int32_t agpl_predictive_cdf(agpl_ctx *ctx, const agpl_lik_desc *lik, int64_t n, const double *mu, const double *var,
                                     const void *y, double *cdf_out, double *sf_out);

/*
 * agpl_predictive_quantile: q_out[i][j] = inf { y : P(Y <= y) >= probs[j] } of the same predictive, j < nq, nq contiguous per point.
 *   probs     : DEVICE array of nq doubles, 1 <= nq <= 16; a prob outside (0, 1) or NaN gives NaN in that column.
 *   q_out     : float64 [n][nq] for every kind; a count quantile is an integer-valued double: the smallest y with P(Y <= y) >= p on
 *               the tail p is in, by doubling from 0 and integer bisection (a quantile beyond the cap of the domain is not
 *               promised); the Bernoulli quantile is 0 (probs[j] <= cdf(0)) or 1.
 *   solve     : continuous kinds -- a bracket grown by doubling from the predictive's location and scale (mu and
 *               sqrt(var + the likelihood's own scale^2)), then Newton steps on the logarithm of the tail that the prob is in (cdf
 *               for p <= 1/2, sf above) with the density, bisection where a step leaves the bracket; stopped at |F - p| <= 1e-10
 *               or a two-ulp bracket, 200 steps at most.  Every step is one pass of the distribution function's rule.
 *   domain    : that of agpl_predictive_cdf, probs from 1e-4 to 1 - 1e-4; there the reference distribution function at q_out is
 *               within 2e-8 of the prob.
 *   edge cases: a bad marginal gives NaN in that point's row.
 *   Errors: as agpl_predictive_cdf, with null probs / q_out (n > 0) and nq outside 1 .. 16 -> AGPL_ERR_INVALID_ARGUMENT.         */
AGPL_API int32_t agpl_predictive_quantile(agpl_ctx *ctx, const agpl_lik_desc *lik, int64_t n, const double *mu, const double *var,
                                          int32_t nq, const double *probs, double *q_out);

#ifdef __cplusplus
}
#endif
#endif /* AGPL_QUANTILE_H */
