/*
 * agpl_se.h -- C ABI of libagpl_se.so: plans of the squared-exponential model built straight from raw inputs, and prediction.
 *
 * An extension of libagpl.so (include/agpl.h): it links against libagpl.so and returns ordinary agpl_plan objects, which every
 * plan entry point of agpl.h serves (agpl_cavi_pass_plan, agpl_plan_update, agpl_marginals_plan, agpl_gibbs_pass_plan,
 * agpl_plan_state, agpl_plan_destroy, ...).  Conventions are agpl.h's: int32 status, device pointers, the context's stream,
 * errors through agpl_last_error of the context.  Kept in its own library so that agpl.h and libagpl.so's export list stay the
 * 45 entry points of AGPL_VERSION 121.
 */
#ifndef AGPL_SE_H
#define AGPL_SE_H

#include "agpl.h"

#ifdef __cplusplus
extern "C" {
#endif

/*
 * k(x, x') = variance exp(-sum_d ((x_d - x'_d) / lengthscale_d)^2 / 2)  (with_lengthscale(SqExponentialKernel(), ell) scaled by
 * variance, examples/bernoulli/script.jl:15), inducing inputs z, features Phi = L^-1 K_ZX with K_ZZ + jitter I = L L'.
 *   agpl_plan_se_bytes  : agpl_plan_bytes(N, M, L, flags) + the generator's state: L^-1 as float32 (Mp^2 floats), z / ell as float64
 *                         (Mp D doubles), the lengthscales (16 doubles), each rounded up to 256 bytes (Mp = M rounded up to 256);
 *                         0 for sizes a plan does not take or D outside 1 .. 16.
 *   agpl_plan_create_se : x [N][D], z [M][D], lengthscale [D]: float64 DEVICE arrays, 1 <= D <= 16.  L^-1 = chol(I + G)^-1 with
 *                         G = K_ZZ + (jitter - 1) I at Mp (agpl_gaussian_factor's float64 route; identity beyond M), then ONE pass
 *                         over the points generates K_ZX tile by tile, whitens it on the matrix cores and writes both images and
 *                         the residual d_i = variance - |phi_i|^2 (agpl_plan_create's clamp): neither K_ZX nor Phi is ever stored.
 *                         The images' scale comes from the Nystrom bound |phi_ai| <= sigma (sigma^2 = variance) before anything is
 *                         written; a realised max |phi| above sigma (1 + 1e-3) is AGPL_ERR_DOMAIN.  Every value a point gets depends
 *                         on its own x only (not on N, its position or the launch): a rank's plan of x[i0:i1] holds rows i0 .. i1
 *                         of the one-process plan bit for bit.  Errors: lengthscale <= 0, variance <= 0, jitter < 0, bad sizes ->
 *                         AGPL_ERR_INVALID_ARGUMENT; non-finite x or z -> AGPL_ERR_DOMAIN with the index; K_ZZ + jitter I not
 *                         positive definite, or a pivot below 16 eps M variance (duplicate z without jitter) -> AGPL_ERR_NOT_POSDEF.
 *                         Synchronises once, as agpl_plan_create.  Everything else is agpl_plan_create's contract.
 *   agpl_plan_predict   : q(f) of the plan's q(v) at Ns new inputs x_s [Ns][D] (float64, device):
 *                             mu = mu0_s + phi_s' m,   var = variance - |phi_s|^2 + |U phi_s|^2      ([L][Ns] float32 each)
 *                         (u_posterior(fz, m, S)(x_te) of examples/bernoulli/script.jl:46-56), in chunks of 65536 points: each chunk's
 *                         marginal image (with the plan's own scale) and residual go to scratch the plan allocates at its first
 *                         prediction and frees with the plan (4 Mp bytes per point of a chunk), then the marginal pass of
 *                         agpl_marginals_plan runs on them: predict(x) at the plan's own x equals agpl_marginals_plan bit for bit.
 *                         mu0_s may be NULL.  A plan not made by agpl_plan_create_se, or with AGPL_PLAN_NO_MARGINALS ->
 *                         AGPL_ERR_INVALID_ARGUMENT.  Asynchronous; a non-finite x_s gives NaN outputs.
 *   agpl_plan_features  : the features the plan holds, (hi + lo) 2^-e decoded from the accumulate image, points i0 .. i0 + n - 1:
 *                         Phi_out float32 [n][M] (any plan).  Asynchronous.                                                      */
AGPL_API int64_t agpl_plan_se_bytes(int64_t N, int32_t M, int32_t L, int32_t D, uint32_t flags);
AGPL_API int32_t agpl_plan_create_se(agpl_ctx *ctx, int64_t N, int32_t M, int32_t L, int32_t D, const double *x, const double *z,
                                     const double *lengthscale, double variance, double jitter, uint32_t flags, void *storage,
                                     agpl_plan **plan_out);
AGPL_API int32_t agpl_plan_predict(agpl_plan *plan, int64_t Ns, const double *x_s, const float *mu0_s, float *mu_out,
                                   float *var_out);
AGPL_API int32_t agpl_plan_features(const agpl_plan *plan, int64_t i0, int64_t n, float *Phi_out);

#ifdef __cplusplus
}
#endif
#endif /* AGPL_SE_H */
