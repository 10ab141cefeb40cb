/*
 * agpl_sample_y.h -- C ABI of libagpl_sampley.so: posterior-predictive draws of the observable y from a block of function draws,
 * for the likelihoods of agpl.h.
 *
 * An extension of libagpl.so (include/agpl.h): it links against libagpl.so, takes its contexts and likelihood descriptors, and
 * keeps agpl.h's conventions -- int32 status, device pointers, the context's stream, errors through agpl_last_error of the
 * context.  Kept in its own library so that agpl.h / libagpl.so stay the 45 entry points of AGPL_VERSION 121.
 */
#ifndef AGPL_SAMPLE_Y_H
#define AGPL_SAMPLE_Y_H

#include "agpl.h"

#ifdef __cplusplus
extern "C" {
#endif

/*
 * agpl_sample_y: y_out[t][i] ~ p(y | f = F[t][.][i]) for t < T, i < Ns, the p(y | f) that agpl_predictive.h lists per kind.
 *   F         : float32 [T][L][ldf] (L = the likelihood's nlatent), ldf >= Ns: the layout agpl_plan_sample_paths and
 *               agpl_plan_predict_chain (samples) write; ldf > Ns samples a point range of a larger block in place.
 *   y_out     : the operator layout of agpl.h, draw-major: uint8 [T][Ns] (Bernoulli), int32 [T][Ns] (NegBinomial, Poisson, Binomial),
 *               float64 [T][Ns] (StudentT, Laplace, HeteroGauss, AsymLaplace, LogisticNoise), one-hot uint8 [T][Ns][L] (both categorical kinds; an all-zero
 *               row of the bijective link means class L).
 *   streams   : draw (t, i) is a pure function of (context seed, global point p = point_offset + point0 + i, sweep, draw0 + t):
 *               its generator g is sub-stream 1 + draw0 + t of the Philox stream (seed, p, sweep) of agpl.h, i.e. counter words
 *               (block, sweep, p & 0xFFFFFFFF, ((p >> 32) & 0xFF) + ((1 + draw0 + t) << 8)).  The sub-stream id has 24 bits:
 *               0 <= draw0 and draw0 + T <= 2^24 - 2.  Neither the launch geometry nor the split of a block of draws or points
 *               over several calls changes a value.
 *   rules     : float64 arithmetic on (double)F without fused multiply-add; u01, normal (two uniforms, cosine Box-Muller),
 *               rand_gamma (Marsaglia-Tsang) and rand_poisson (exponential arrivals below 6, PTRS from 6) are agpl_random.h's.
 *               sigma(x) = 1 / (1 + exp(-x)).  Each kind consumes g in this order, once:
 *     Bernoulli        u = u01();                                    y = u < sigma(f)
 *     Categorical      w_k = theta_k sigma(f_k), k < L (theta = exp(logtheta)); tot = sum_k w_k in ascending k, started at
 *                      theta_L / 2 for the bijective link and at 0 otherwise; u = u01() tot; cum = 0; the class is the first k
 *                      with u < (cum += w_k), else the implicit class L (bijective: an all-zero row) or class L - 1
 *     Poisson(lam)     y = rand_poisson(g, lam sigma(f))
 *     NegBinomial(r)   a = rand_gamma(g, r); y = rand_poisson(g, a exp(f))
 *     StudentT(nu, s)  z = normal(); ch = 2 rand_gamma(g, nu / 2);   y = f + s z / sqrt(ch / nu)
 *     Laplace(beta)    u = u01(); d = u - 1/2;                       y = f - beta sign(d) log1p(-2 |d|)
 *     HeteroGauss(lam) z = normal();                                 y = f + z / sqrt(lam sigma(g)), latents (f, g)
 *     AsymLaplace(sigma, tau)  u = u01(); d = u - tau;  the inverse distribution function in its log1p forms:
 *                      d < 0:  y = f + sigma log1p(d / tau) / (1 - tau)       (= f + sigma log(u / tau) / (1 - tau))
 *                      else:   y = f - sigma log1p(-d / (1 - tau)) / tau      (= f - sigma log((1 - u) / (1 - tau)) / tau)
 *     LogisticNoise(s) u = u01();                                    y = f + s (log u - log1p(-u))   (the inverse cdf of Logistic(0, 1))
 *     Binomial(n)      p = sigma(f).  n <= 64: y = the number of j < n with u01() < p, n consecutive uniforms.  n > 64 (any n the
 *                      descriptor takes, n < 2^22): q = p if p <= 1/2 else 1 - p (y = k, or n - k for p > 1/2) and
 *                        n q < 10:  the inverse-cdf walk.  s = q / (1 - q); a = (n + 1) s; r = exp(n log1p(-q)); u = u01(); k = 0;
 *                                   while u > r and k < n: u -= r; k += 1; r *= a / k - s
 *                        else:      Hormann's transformed rejection (BTRS).  spq = sqrt(n q (1 - q)); b = 1.15 + 2.53 spq;
 *                                   a = -0.0873 + 0.0248 b + 0.01 q; c = n q + 0.5; vr = 0.92 - 4.2 / b; alpha = (2.83 + 5.1 / b) spq;
 *                                   lpq = log(q / (1 - q)); m = floor((n + 1) q); h = lgamma(m + 1) + lgamma(n - m + 1); repeat
 *                                   U = u01() - 0.5; V = u01(); us = 0.5 - |U|; k = floor((2 a / us + b) U + c); again if k < 0 or
 *                                   k > n; accept if us >= 0.07 and V <= vr; accept if log(V alpha / (a / us^2 + b)) <=
 *                                   h - lgamma(k + 1) - lgamma(n - k + 1) + (k - m) lpq
 *               A count whose Poisson rate is >= 2^31 - 1 (or whose draw exceeds it) saturates at 2^31 - 1.
 *   edge cases: a non-finite F entry is not an error: that draw's output is the "no observation" value of agpl_predictive --
 *               NaN (real kinds), -1 (counts), 255 (uint8; every entry of the row for the categorical kinds).  T == 0 or
 *               Ns == 0 writes nothing.
 *   Asynchronous on the context's stream; allocates nothing and does not wait on the host.
 *   Errors: null context / descriptor, null F / y_out with T Ns > 0, T < 0, Ns < 0, ldf < Ns, a draw0 outside the range above,
 *   parameters outside the likelihood's domain -> AGPL_ERR_INVALID_ARGUMENT.                                                  */
AGPL_API int32_t agpl_sample_y(agpl_ctx *ctx, const agpl_lik_desc *lik, int32_t T, int64_t Ns, int64_t ldf, const float *F,
                               int64_t point0, int32_t draw0, uint32_t sweep, void *y_out);

#ifdef __cplusplus
}
#endif
#endif /* AGPL_SAMPLE_Y_H */
