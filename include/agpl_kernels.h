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
 */
typedef enum {
    AGPL_KERNEL_SE = 0,
    AGPL_KERNEL_MATERN12 = 1,
    AGPL_KERNEL_MATERN32 = 2,
    AGPL_KERNEL_MATERN52 = 3,
    AGPL_KERNEL_RQ = 4,
    AGPL_KERNEL_PERIODIC = AGPL_KERNEL_RQ + 2 /* 6 */,
    AGPL_KERNEL_SE_PERIODIC = AGPL_KERNEL_RQ + 4 /* 8 */,
    AGPL_KERNEL_SE_COSINE = AGPL_KERNEL_RQ + 6 /* 10 */
} agpl_kernel_kind;

/*
 * agpl_plan_create_stationary: agpl_plan_create_se (include/agpl_se.h) for the covariance function `kind` -- the same arguments
 * (storage of agpl_plan_se_bytes(N, M, L, D, flags) bytes or NULL, whatever the kind), the same single pass over the points, the
 * same errors and single synchronisation, the same starting q(v) = N(0, I), and a plan that agpl_plan_predict,
 * agpl_plan_predict_chain and agpl_plan_features serve with this covariance function.  kind = AGPL_KERNEL_SE gives the plan of
 * agpl_plan_create_se bit for bit.  K_ZZ is evaluated in float64; the generator forms r^2 and r in float64 and takes the exponential
 * (rational quadratic: exp(-alpha log1p(r^2 / (2 alpha)))) in float32.  The images' scale is the Nystrom bound |phi_ai| <= sigma,
 * which holds for every kernel with k(x, x) = variance.
 *   param : alpha of AGPL_KERNEL_RQ, the period p of AGPL_KERNEL_PERIODIC, AGPL_KERNEL_SE_PERIODIC and AGPL_KERNEL_SE_COSINE (positive and finite, else AGPL_ERR_INVALID_ARGUMENT);
 *           ignored for the other kinds.
 *   An unknown kind -> AGPL_ERR_INVALID_ARGUMENT.                                                                                  */
AGPL_API int32_t agpl_plan_create_stationary(agpl_ctx *ctx, int64_t N, int32_t M, int32_t L, int32_t D, int32_t kind, double param,
                                             const double *x, const double *z, const double *lengthscale, double variance,
                                             double jitter, uint32_t flags, void *storage, agpl_plan **plan_out);

#ifdef __cplusplus
}
#endif
#endif /* AGPL_KERNELS_H */
