/*
 * agpl_kernels.h -- C ABI of libagpl_kernels.so: plans built straight from raw inputs for the stationary covariance functions of
 * KernelFunctions.jl beyond the squared exponential (Matern-1/2, -3/2, -5/2, rational quadratic).
 *
 * An extension of libagpl.so (include/agpl.h): it links against libagpl.so, returns the plans agpl_plan_create_se returns
 * (include/agpl_se.h) and keeps agpl.h's conventions -- int32 status, device pointers, the context's stream, errors through
 * agpl_last_error of the context.  Kept in its own library so that agpl.h / libagpl.so stay the 45 entry points of AGPL_VERSION 121,
 * agpl_se.h / libagpl_se.so their four, agpl_predictive.h / libagpl_predictive.so and agpl_chain.h / libagpl_chain.so their one each.
 */
#ifndef AGPL_KERNELS_H
#define AGPL_KERNELS_H

#include "agpl.h"

#ifdef __cplusplus
extern "C" {
#endif

/*
 * k(x, x') = variance kappa(r), r^2 = sum_d ((x_d - x'_d) / lengthscale_d)^2  (with_lengthscale(kernel, ell) scaled by variance, the
 * kernel of examples/bernoulli/script.jl:15 replaced by another one of KernelFunctions.jl):
 *
 *   kind                        KernelFunctions.jl                         kappa(r) = k / variance
 *   AGPL_KERNEL_SE        = 0   SqExponentialKernel()                      exp(-r^2 / 2)
 *   AGPL_KERNEL_MATERN12  = 1   ExponentialKernel() = Matern12Kernel()     exp(-r)
 *   AGPL_KERNEL_MATERN32  = 2   Matern32Kernel()                           (1 + sqrt(3) r) exp(-sqrt(3) r)
 *   AGPL_KERNEL_MATERN52  = 3   Matern52Kernel()                           (1 + sqrt(5) r + 5 r^2 / 3) exp(-sqrt(5) r)
 *   AGPL_KERNEL_RQ        = 4   RationalQuadraticKernel(alpha = param)     (1 + r^2 / (2 alpha))^(-alpha)
 *   AGPL_KERNEL_PERIODIC  = 6   PeriodicKernel(r = lengthscale) on x / p   exp(-r^2 / 2) with the terms of r^2 warped (below)
 *   AGPL_KERNEL_SE_PERIODIC = 8 SqExponentialKernel() on x_1 .. x_{D-1} * PeriodicKernel() on x_D / p   exp(-r^2 / 2), last term warped
 *   AGPL_KERNEL_SE_COSINE = 10  SqExponentialKernel() on x * CosineKernel() on 2 x_D / p   exp(-r^2 / 2) cos(2 pi (x_D - x'_D) / p)
 *   AGPL_KERNEL_ADDITIVE_SE = 14  KernelSum of SqExponentialKernel() on x_d / lengthscale_d, d = 1 .. D, each weighted 1 / D (below)
 *   AGPL_KERNEL_ADDITIVE2_SE = 40  the same KernelSum (share param = w) plus the D (D - 1) / 2 SqExponentialKernel()s on pairs of inputs (below)
 *   AGPL_KERNEL_MATERN32_PRODUCT = 64  KernelTensorProduct of Matern32Kernel() on x_d / lengthscale_d, d = 1 .. D   prod_d (1 + a_d) exp(-a_d), a_d = sqrt(3) |u_d| (below)
 *   AGPL_KERNEL_MATERN52_PRODUCT = 66  KernelTensorProduct of Matern52Kernel() on x_d / lengthscale_d, d = 1 .. D   prod_d (1 + a_d + a_d^2 / 3) exp(-a_d), a_d = sqrt(5) |u_d| (below)
 *   AGPL_KERNEL_SE_MATERN32 = 70  SqExponentialKernel() on x_1 .. x_{D-1} * Matern32Kernel() on x_D   (1 + a) exp(-(r_lead^2 / 2 + a)), a = sqrt(3) |u_D| (below)
 *   AGPL_KERNEL_SE_MATERN52 = 72  SqExponentialKernel() on x_1 .. x_{D-1} * Matern52Kernel() on x_D   (1 + a + a^2 / 3) exp(-(r_lead^2 / 2 + a)), a = sqrt(5) |u_D| (below)
 *   AGPL_KERNEL_ANOVA_SE = 80  KernelTensorProduct of (1 - eta) ConstantKernel() + eta SqExponentialKernel() on x_d / lengthscale_d, eta = param   prod_d (1 - eta (1 - exp(-u_d^2 / 2))) (below)
 *   AGPL_KERNEL_SE_CATEGORICAL = 96  SqExponentialKernel() on x_1 .. x_{D-C} * an exchangeable (Hamming) correlation on each of the last C = param inputs   exp(-(r_lead^2 + sum_{d > D-C} [x_d != x'_d] / lengthscale_d^2) / 2) (below)
 *
 * The periodic kind (param = the period p, one scalar for all dimensions) is the squared exponential's kappa on a warped distance:
 *     r^2 = sum_d (sin(pi (x_d - x'_d) / p) / lengthscale_d)^2,   k = variance exp(-r^2 / 2),   k(x, x' + p e_d) = k(x, x'),
 * the one kind whose r is not the scaled Euclidean distance (csrc/agpl_kernel_rules.h: kernel_warp; sinpi in float64).  5 is not a
 * kind: it stays refused as an unknown kind.
 *
 * The squared exponential x periodic kind (param = the period p) warps the LAST dimension only:
 *     r^2 = sum_{d < D-1} ((x_d - x'_d) / lengthscale_d)^2 + (sin(pi (x_{D-1} - x'_{D-1}) / p) / lengthscale_{D-1})^2,
 * k = variance exp(-r^2 / 2): periodic in the last input (time, an angle) and squared exponential in the others, x = (..., t); with
 * x = (t, t) it is the locally periodic kernel SE(t) Per(t).  At D = 1 it is the periodic kind.  Which dimensions a kind warps is stated
 * once (csrc/agpl_kernel_rules.h: kernel_dim_warped).  7 is not a kind: it stays refused as an unknown kind.
 *
 * The squared exponential x cosine kind (param = the period p) warps nothing: r is the scaled Euclidean distance over all D dimensions,
 * and kappa is multiplied by a cosine of the LAST input's difference,
 *     k = variance exp(-r^2 / 2) cos(2 pi (x_{D-1} - x'_{D-1}) / p)
 * (SqExponentialKernel o ARDTransform times CosineKernel o ScaleTransform(2 / p) on the last coordinate; at D = 1 one component of a
 * spectral mixture).  It is the one kind that takes negative values: k = -variance exp(-r^2 / 2) half a period away, 0 a quarter
 * period away.  It is stationary with k(x, x) = variance and positive definite (its spectral measure is the squared exponential's
 * Gaussian shifted to +-2 pi / p in the last dimension), so the Nystrom bound and everything built on it hold.  k is not a function
 * of r^2 and one parameter: the factor and its derivative are stated once (csrc/agpl_kernel_rules.h: kernel_dim_modulated,
 * kernel_modulation), and every derivative of k in x or z has a product rule in the last dimension; d k / d log lengthscale_d is
 * ((x_d - x'_d) / lengthscale_d)^2 k in every dimension, the factor not depending on the lengthscales.  9 is not a kind: it stays
 * refused as an unknown kind.
 *
 * The additive squared exponential kind (no parameter: param is ignored) is no function of r^2 at all: with u_d = (x_d - x'_d) /
 * lengthscale_d it is the sum over the inputs of a squared exponential in each alone,
 *     k = (variance / D) sum_{d < D} exp(-u_d^2 / 2),
 * the first-order additive Gaussian process f(x) = sum_d f_d(x_d) (Duvenaud, Nickisch and Rasmussen 2011; a KernelSum of
 * SqExponentialKernel o ScaleTransform(1 / lengthscale_d) o SelectTransform(d)), the prior of a generalised additive model.  It is
 * stationary with k(x, x) = variance and positive semi-definite, so the Nystrom bound and everything built on it hold; at D = 1 it is
 * the squared exponential, bit for bit.  Two points far apart in one input keep the covariance of the others.  The per-dimension term
 * and its derivative are stated once (csrc/agpl_kernel_rules.h: kernel_kind_additive, kernel_term, kernel_dterm); every derivative of
 * k in x_d, z_d or log lengthscale_d holds dimension d's own term only: d k / d log lengthscale_d = (variance / D) u_d^2 exp(-u_d^2 / 2),
 * and the prior variance of d f / d x_d is variance / (D lengthscale_d^2).  11, 12 and 13 are not kinds: they stay refused.
 *
 * The second-order additive squared exponential kind (param = w, the share of the prior variance carried by the first-order part,
 * 0 < w <= 1, else AGPL_ERR_INVALID_ARGUMENT; not learned) adds the pairwise interactions the first-order kind cannot express ("the
 * effect of x_1 depends on x_2"; main effects plus pairwise interactions, the second order of Duvenaud, Nickisch and Rasmussen 2011).
 * With e_d = exp(-u_d^2 / 2), S1 = sum_d e_d, E2 = sum_{d < d'} e_d e_d' and P = D (D - 1) / 2,
 *     k = variance (w S1 / D + (1 - w) E2 / P)   for D >= 2,        k = variance e_0   for D = 1 (no pairs: w is ignored),
 * a KernelSum of the D one-dimensional squared exponentials and the P two-dimensional ones on SelectTransform([d, d']).  It is
 * stationary with k(x, x) = variance (S1 = D, E2 = P at u = 0), positive semi-definite and even in every u_d to the bit; at w = 1 it
 * is the additive kind above and at D = 1 the squared exponential, bit for bit.  Every sum runs over d = 0 .. D - 1 in that order by
 * the recurrence E2 <- fma(e_d, S1, E2), S1 <- S1 + e_d, never (S1^2 - sum e_d^2) / 2, which cancels when one input dominates.  The
 * derivatives are d k / d u_d = variance (-u_d e_d) c_d with c_d = w / D + (1 - w) (S1 - e_d) / P, and d k / d log lengthscale_d =
 * variance u_d^2 e_d c_d; the prior variance of d f / d x_d is variance (2 - w) / (D lengthscale_d^2).  The two weights and that
 * factor are stated once (csrc/agpl_kernel_rules.h: kernel_kind_additive2, kernel_sum_weight1, kernel_sum_weight2,
 * kernel_sum_curvature).  The kind is 40 and not 15: tests/test_additive_se_rules_cpu.py holds that no kind between 15 and 39 is
 * known, so 15 ... 39 are not kinds and stay refused.
 *
 * The two product (separable, tensor-product) Matern kinds (no parameter: param is ignored) are a PRODUCT over the inputs of a
 * one-dimensional Matern in each alone: with u_d = (x_d - x'_d) / lengthscale_d, a_d = c |u_d| (c = sqrt(3) or sqrt(5)) and the
 * polynomial p(a) = 1 + a (3/2) or 1 + a + a^2 / 3 (5/2),
 *     k = variance (prod_{d < D} p(a_d)) exp(-sum_{d < D} a_d),
 * a KernelTensorProduct of Matern32Kernel() / Matern52Kernel() o ScaleTransform(1 / lengthscale_d): what Matern(time) * Matern(space)
 * means, the separable space-time model, and the kernel of the Sobolev spaces of dominating mixed smoothness.  It is stationary with
 * k(x, x) = variance and positive definite, so the Nystrom bound and everything built on it hold; at D = 1 it is AGPL_KERNEL_MATERN32 /
 * AGPL_KERNEL_MATERN52 (to float32 rounding in the generated features: a_d is rounded once from the float64 product c |u_d|).  The sum
 * and the product run over d = 0 .. D - 1 in that order; |u_d| is even to the bit, so K_ZZ is symmetric to the bit.  No square root is
 * taken anywhere.  The derivatives never divide by p(a_d): with t(a) = kappa'(|u|) / |u| e^a = -3 (3/2) or -(5 / 3) (1 + a) (5/2),
 *     d k / d u_d = variance u_d t(a_d) (prod_{d' != d} p(a_d')) exp(-sum a),     d k / d log lengthscale_d = -u_d d k / d u_d,
 * continuous at u_d = 0; the prior variance of d f / d x_d is variance c0 / lengthscale_d^2 with c0 = -t(0) = 3 or 5 / 3, the isotropic
 * kinds' values.  All of it is stated once (csrc/agpl_kernel_rules.h: kernel_kind_product, kernel_product_scale, kernel_pterm,
 * kernel_dpterm, kernel_product_curvature).  The product Matern-1/2, exp(-sum_d |u_d|), is left out: it is not differentiable, so every
 * gradient consumer would have to refuse it.  The kinds start at 64 because tests/test_additive2_se_rules_cpu.py holds the set of
 * kinds below 64; 65 and every other number from 64 on are not kinds and stay refused.
 *
 * The two squared exponential x Matern kinds (no parameter: param is ignored) are smooth in the leading inputs and of finite smoothness
 * in the LAST one, x = (covariates or space ..., t): the separable SE(space) Matern(time) prior, whose paths in t are those of a
 * stochastic differential equation's output.  With r_lead^2 = sum_{d < D-1} u_d^2, a = c |u_{D-1}| and c, p, t, c0 of the product kinds
 * above,
 *     k = variance p(a) exp(-(r_lead^2 / 2 + a)),
 * a KernelTensorProduct of SqExponentialKernel() o ARDTransform on x_1 .. x_{D-1} and Matern32Kernel() / Matern52Kernel() o
 * ScaleTransform(1 / lengthscale_D) on x_D.  It is stationary with k(x, x) = variance and positive definite; u^2 and |u| are even to
 * the bit, so K_ZZ is symmetric to the bit; at D = 1 it is AGPL_KERNEL_MATERN32 / AGPL_KERNEL_MATERN52 (to float32 rounding in the
 * generated features, as the product kinds).  The generator takes ONE float32 exponential per element and no square root.  The
 * derivatives never divide by p: d k / d u_d = -u_d k in a leading dimension and variance u t(a) exp(-(r_lead^2 / 2 + a)) in the last;
 * d k / d log lengthscale_d = -u_d d k / d u_d; the prior variance of d f / d x_d is variance / lengthscale_d^2 in a leading dimension
 * and variance c0 / lengthscale_d^2 in the last.  All of it is stated once (csrc/agpl_kernel_rules.h: kernel_kind_se_matern and the
 * helpers beside it, which take p and t from the product kinds').  The Matern-1/2 in the last input (71, as 65) is left out: it is
 * not differentiable.  The kinds are 70 and 72 because tests/test_matern_product_rules_cpu.py holds the set of kinds below 70; 71 and
 * every other number from 67 to 79 are not kinds and stay refused.
 *
 * The all-orders additive (ANOVA) squared exponential kind (param = eta, 0 < eta <= 1, else AGPL_ERR_INVALID_ARGUMENT; not learned)
 * closes the family the two additive kinds opened: main effects, pairs, triples ... up to the full D-way interaction, in one product
 * over the inputs of (constant + one-dimensional squared exponential).  With e_d = exp(-u_d^2 / 2),
 *     k = variance prod_{d < D} g_d,        g_d = 1 - eta (1 - e_d),
 * a KernelTensorProduct of (1 - eta) ConstantKernel() + eta SqExponentialKernel() o ScaleTransform(1 / lengthscale_d).  Expanded it is
 * the sum of all 2^D interaction terms: a given set of n inputs carries eta^n (1 - eta)^(D - n) of the variance, so the interaction
 * order is Binomial(D, eta)-distributed; small eta is dominated by the first order, and eta = 1 is mathematically the squared
 * exponential (not bit for bit: D float32 exponentials and a product where that kind takes one exponential of r^2).  The share
 * (1 - eta)^D belongs to a shared random level: FAR FROM ALL DATA k TENDS TO variance (1 - eta)^D AND NOT TO 0.  It is stationary with
 * k(x, x) = variance to the bit (g = fma(-eta, 1 - e, 1) is exactly 1 at u = 0) and positive semi-definite, so the Nystrom bound and
 * everything built on it hold; g is even in u_d to the bit, so K_ZZ is symmetric to the bit; g lies in [1 - eta, 1], so the running
 * product, taken over d = 0 .. D - 1 in that order everywhere, never overflows.  The derivatives never divide by g_d (it underflows
 * at eta = 1): they take the product excluding d,
 *     d k / d u_d = variance eta (-u_d e_d) prod_{d' != d} g_d',        d k / d log lengthscale_d = -u_d d k / d u_d;
 * the prior variance of d f / d x_d is variance eta / lengthscale_d^2.  All of it is stated once (csrc/agpl_kernel_rules.h:
 * kernel_kind_anova, kernel_anova_factor, kernel_anova_dfactor, kernel_anova_curvature).  The kind is 80 because
 * tests/test_se_matern_rules_cpu.py holds the set of kinds in -2 .. 79; 73 .. 79 and 81 .. 95 are not kinds and stay refused.
 *
 * The squared exponential x categorical kind (param = C, an integer, 1 <= C <= 16 and C <= D, else AGPL_ERR_INVALID_ARGUMENT; not
 * learned) serves MIXED inputs: the first D - C inputs are continuous, the LAST C are category codes (a region, a species, a machine,
 * the task index of a multi-task model), in the "trailing inputs are the special ones" convention of kinds 8, 10, 70 and 72.  A code
 * has no distance: it is compared for equality only.  With u_d = (x_d - x'_d) / lengthscale_d in the leading inputs,
 *     k = variance exp(-(sum_{d < D-C} u_d^2 + sum_{d >= D-C} [x_d != x'_d] / lengthscale_d^2) / 2):
 * the squared exponential in the continuous inputs times the exchangeable (compound-symmetry, Hamming) correlation in each categorical
 * one, the CategoricalKernel of the mixed-input literature; with one categorical input it is the multi-task model with exchangeable
 * task correlation.  Two points that differ in categorical input d are correlated rho_d = exp(-1 / (2 lengthscale_d^2)) through it:
 * a large lengthscale_d says the category does not matter, a small one says independent groups, and rho_d is learned through
 * log lengthscale_d like any other lengthscale.  It is SqExponentialKernel() on the one-hot encoding of that input with lengthscale
 * sqrt(2) lengthscale_d, at the cost of one input dimension per categorical INPUT and not per level.  The codes are any float64
 * values (integers are recommended): the library compares the scaled values x_d / lengthscale_d it holds anyway, equal codes give a
 * difference of exactly 0 and distinct integer codes never do.  It is the squared exponential's rule on a warped distance with
 * u_d = [x_d != x'_d] / lengthscale_d and d u_d / d x_d = 0 in a categorical input: stationary, k(x, x) = variance, symmetric to
 * the bit.  d k / d log lengthscale_d = u_d^2 k in every input; every derivative in a categorical input itself is exactly 0: the
 * gradient for the inducing inputs leaves their codes alone (they must carry codes there: agpl_select_inducing_greedy picks them from
 * the data), and the mean and variance of d f / d x_d are written as 0.  C = D (categorical inputs only) is allowed.  All of it is
 * stated once (csrc/agpl_kernel_rules.h: kernel_kind_categorical, kernel_dim_categorical, kernel_categorical_warp).  The kind is 96
 * because tests/test_anova_se_rules_cpu.py holds the set of kinds in -2 .. 95; 81 .. 95 and every number from 97 on are not kinds
 * and stay refused.
 */
typedef enum {
    AGPL_KERNEL_SE = 0,
    AGPL_KERNEL_MATERN12 = 1,
    AGPL_KERNEL_MATERN32 = 2,
    AGPL_KERNEL_MATERN52 = 3,
    AGPL_KERNEL_RQ = 4,
    AGPL_KERNEL_PERIODIC = AGPL_KERNEL_RQ + 2 /* 6 */,
    AGPL_KERNEL_SE_PERIODIC = AGPL_KERNEL_RQ + 4 /* 8 */,
    AGPL_KERNEL_SE_COSINE = AGPL_KERNEL_RQ + 6 /* 10 */,
    AGPL_KERNEL_ADDITIVE_SE = AGPL_KERNEL_RQ + 10 /* 14 */,
    AGPL_KERNEL_ADDITIVE2_SE = AGPL_KERNEL_RQ + 36 /* 40 */,
    AGPL_KERNEL_MATERN32_PRODUCT = AGPL_KERNEL_RQ + 60 /* 64 */,
    AGPL_KERNEL_MATERN52_PRODUCT = AGPL_KERNEL_RQ + 62 /* 66 */,
    AGPL_KERNEL_SE_MATERN32 = AGPL_KERNEL_RQ + 66 /* 70 */,
    AGPL_KERNEL_SE_MATERN52 = AGPL_KERNEL_RQ + 68 /* 72 */,
    AGPL_KERNEL_ANOVA_SE = AGPL_KERNEL_RQ + 76 /* 80 */,
    AGPL_KERNEL_SE_CATEGORICAL = AGPL_KERNEL_RQ + 92 /* 96 */
} agpl_kernel_kind;

/*
 * agpl_plan_create_stationary: agpl_plan_create_se (include/agpl_se.h) for the covariance function `kind` -- the same arguments
 * (storage of agpl_plan_se_bytes(N, M, L, D, flags) bytes or NULL, whatever the kind), the same single pass over the points, the
 * same errors and single synchronisation, the same starting q(v) = N(0, I), and a plan that agpl_plan_predict,
 * agpl_plan_predict_chain and agpl_plan_features serve with this covariance function.  kind = AGPL_KERNEL_SE gives the plan of
 * agpl_plan_create_se bit for bit.  K_ZZ is evaluated in float64; the generator forms r^2 and r in float64 and takes the exponential
 * (rational quadratic: exp(-alpha log1p(r^2 / (2 alpha)))) in float32.  The images' scale is the Nystrom bound |phi_ai| <= sigma,
 * which holds for every kernel with k(x, x) = variance.
 *   param : alpha of AGPL_KERNEL_RQ, the period p of AGPL_KERNEL_PERIODIC, AGPL_KERNEL_SE_PERIODIC and AGPL_KERNEL_SE_COSINE (positive and finite, else AGPL_ERR_INVALID_ARGUMENT),
 *           the first-order share w of AGPL_KERNEL_ADDITIVE2_SE and eta of AGPL_KERNEL_ANOVA_SE (0 < param <= 1, else AGPL_ERR_INVALID_ARGUMENT);
 *           the number C of trailing categorical inputs of AGPL_KERNEL_SE_CATEGORICAL (an integer, 1 <= C <= min(D, 16), else AGPL_ERR_INVALID_ARGUMENT);
 *           ignored for the other kinds.
 *   An unknown kind -> AGPL_ERR_INVALID_ARGUMENT.                                                                                  */
AGPL_API int32_t agpl_plan_create_stationary(agpl_ctx *ctx, int64_t N, int32_t M, int32_t L, int32_t D, int32_t kind, double param,
                                             const double *x, const double *z, const double *lengthscale, double variance,
                                             double jitter, uint32_t flags, void *storage, agpl_plan **plan_out);

#ifdef __cplusplus
}
#endif
#endif /* AGPL_KERNELS_H */
