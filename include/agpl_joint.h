/*
 * agpl_joint.h -- C ABI of libagpl_joint.so: the JOINT posterior of f at new inputs under a plan's q(v) -- the covariance between
 * any two inputs (`cov` of u_posterior(fz, m, S)(x_te), examples/bernoulli/script.jl:46-56), from which coherent function draws
 * (`rand`) are made -- for plans made from raw inputs (include/agpl_se.h, include/agpl_kernels.h).
 *
 * An extension of libagpl.so (include/agpl.h): it links against libagpl.so, takes the plans agpl_plan_create_se /
 * agpl_plan_create_stationary return and keeps agpl.h's conventions -- int32 status, device pointers, the context's stream, errors
 * through agpl_last_error of the context.  Kept in its own library so that agpl.h / libagpl.so stay the 45 entry points of
 * AGPL_VERSION 121 and the other four extension libraries their own.
 */
#ifndef AGPL_JOINT_H
#define AGPL_JOINT_H

#include "agpl.h"

#ifdef __cplusplus
extern "C" {
#endif

/*
 * For latent l, inputs x_a [Na][D] and x_b [Nb][D] (float64, device) and the plan's q(v) = (U_l, v_l), S_l = U_l' U_l:
 *   cov_out[l][i][j] = k(x_a_i, x_b_j) - phi(x_a_i)' phi(x_b_j) + (U_l phi(x_a_i))' (U_l phi(x_b_j))
 *                    = k(x_a_i, x_b_j) + phi(x_a_i)' (U_l' U_l - I) phi(x_b_j)
 * with phi = L^-1 K_Z. the plan's own features and k the plan's own covariance function (any kind of agpl_kernels.h).  Its
 * diagonal at x_a = x_b is the var of agpl_plan_predict; a fresh plan (U = I) gives the prior covariance k(x_a, x_b).
 *   cov_out   : float32 [L][Na][ld], row-major, ld >= Nb.  Columns j >= Nb of every row are NOT written: a caller assembles a
 *               large matrix block by block through ld.
 *   x_b NULL  : the symmetric form, x_b = x_a (Nb must equal Na).  Only tiles on or below the diagonal are computed and every
 *               entry above the diagonal is the copy of its mirror image: the output is symmetric bit for bit, and its entries
 *               with i >= j are bit for bit those of the general call on a copy of x_a.
 *   features  : the plan's own generator at the plan's own scale, in chunks of 65536 points of either set whose images go to the
 *               plan's prediction scratch (agpl_plan_predict's; carved anew and grown here if needed, freed with the plan).
 *   numerics  : W_l = U_l' U_l - I in float64 (entries in [-1, 1]), packed as split float16 (hi + lo) at 2^15; T = W_l Phi_b and
 *               then Phi_a' T on the matrix cores (v_mfma_f32_32x32x16_f16: hi hi + hi lo + lo hi, float32 accumulation), T held
 *               as a second split-float16 image at the plan's scale; k = variance kappa(r) with r^2 in float64 and kappa in
 *               float32, the generator's own rule.  Fixed summation orders, no float atomics: an entry depends on (x_a_i, x_b_j,
 *               the plan) only -- not on Na, Nb, ld, the position of either point or its chunk -- so a block of a larger call
 *               equals that block computed alone, bit for bit (the mirrored upper triangle of the symmetric form excepted).
 *   errors    : a plan not made from raw inputs, a plan with AGPL_PLAN_NO_MARGINALS (its U is not maintained; agpl_plan_predict
 *               refuses it too), a null plan / x_a / cov_out, ld < Nb, a negative size, x_b NULL with Nb != Na ->
 *               AGPL_ERR_INVALID_ARGUMENT.  A non-finite input gives NaN in its row (x_a) or column (x_b) and nothing else.
 *               Na = 0 or Nb = 0 -> AGPL_OK, nothing written, nothing launched.  The context stays usable after every error.
 *   The call is asynchronous on the context's stream: it does not wait on the host (growing the scratch waits for earlier work
 *   that may still use it, once).                                                                                              */
AGPL_API int32_t agpl_plan_predict_cov(agpl_plan *plan, int64_t Na, const double *x_a, int64_t Nb, const double *x_b,
                                       float *cov_out, int64_t ld);

#ifdef __cplusplus
}
#endif
#endif /* AGPL_JOINT_H */
