/*
 * agpl_zgrad.h -- C ABI of libagpl_zgrad.so: the gradient of the sweep's bound with respect to the inducing inputs z of a plan made
 * from raw inputs (include/agpl_se.h, include/agpl_kernels.h), at the plan's q(v) -- and, in the same pass over the points, the
 * gradient for the kernel hyperparameters that include/agpl_hyper.h describes.
 *
 * An extension of libagpl.so (include/agpl.h): it links against libagpl.so, takes the plans agpl_plan_create_se /
 * agpl_plan_create_stationary return and keeps agpl.h's conventions -- int32 status, device pointers, the context's stream, errors
 * through agpl_last_error of the context.  Kept in its own library so that agpl.h / libagpl.so stay the 45 entry points of
 * AGPL_VERSION 121 and the other seven extension libraries (libagpl_hyper.so and its one entry point among them) their own.
 */
#ifndef AGPL_ZGRAD_H
#define AGPL_ZGRAD_H

#include "agpl.h"

#ifdef __cplusplus
extern "C" {
#endif

/*
 * The objective Lb, q(v) = N(m, S), beta, gamma, mu0, phi_i = L^-1 k_Z(x_i), K_ZZ + jitter I = L L' and every other symbol are those
 * of include/agpl_hyper.h; here m, S, beta, gamma, mu0, jitter, the kernel's parameter, the lengthscales and the variance are held
 * fixed and z moves.  With u_d = (z_ad - x_id) / ell_d and q(r) = kappa'(r) / r:
 *   grad_z_out     : float64 [M][D], device (M: the caller's feature count):  dLb / dz_ad, z in the CALLER's units (not the scaled
 *                    z / ell the plan holds).
 *   grad_theta_out : float64 [D + 1], device, or NULL:  dLb / d log ell_d (d < D), then dLb / d log variance -- bit for bit what
 *                    agpl_plan_hyper_grad writes on the same arguments (the same code, stated once), from the same pass over the points.
 *   x, mu0, beta, gamma, G, g : as agpl_plan_hyper_grad.
 * Two parts, split as those of agpl_plan_hyper_grad.  The POINTS' part (always, over the N local points; L held fixed):
 *     dLb / dz_ad  = sum_l sum_i W_ai variance q(r_ai) (z_ad - x_id) / ell_d^2,   W_ai = gamma_li R_ai + b_li p_a,  R = C_l Phi
 * (W: the weight dLb / dk_Z(x_i) of agpl_hyper.h).  The K_ZZ part (through L; float64, M x M):
 *     dLb / dz_ad += 2 sum_{b != a} Kbar_ab variance q(r_ab) (z_ad - z_bd) / ell_d^2
 * with agpl_hyper.h's Kbar, the prior-mean term h included: it runs when G, g are given (the (G, g) terms of A) or mu0 is given (the
 * -m_l h_l' term of the call's OWN points).  The diagonal of K_ZZ does not depend on z.  In a run that shards N, ONE rank passes the
 * exchanged G, g, every rank passes its own points, and the numbers summed over ranks are the gradient.
 *   r = 0       : a point on an inducing input, or two coincident inducing inputs, contributes 0 (z_ad - x_id = 0; q has a finite
 *               limit for four kinds, and for Matern-1/2, which has none, 0 is used: agpl_kernel_rules.h).
 *   numerics    : everything up to the weight as agpl_plan_hyper_grad (L^-1, C_l, p_l in float64; R = C_l Phi on the matrix cores
 *               from split float16; q in float32 from r^2 in float64).  cq_ai = -W_ai variance q(r_ai), formed in float64, is
 *               rounded ONCE to float32 and left in the workgroup's [row][point] tile; a second phase of the same kernel, one thread
 *               per (row a, half of the tile's 128 points), sums cq_ai (x_id - z_ad) / ell_d over its points in float64 and the two
 *               halves are added: part_z[tile][a][d].  A reduction kernel adds the tiles in ascending order into a float64 [M][D]
 *               accumulator, a last kernel adds the K_ZZ part (float64 throughout: one workgroup per row a, a fixed tree) and
 *               divides by ell_d.  No float atomics, no sum depends on the launch: two calls on the same inputs give the same bits.
 *   scratch     : the plan's prediction scratch, grown as agpl_plan_hyper_grad grows it, plus 2 [M][D] float64 and part_z.  part_z
 *               is bounded: the points of a 65536-point chunk are taken in groups of tiles whose part_z (tiles x M x D x 8 bytes)
 *               fits 16 MiB -- never fewer than one tile, i.e. at most max(16 MiB, 8 M D) bytes -- and reduced after each group.
 *               Nothing else the plan holds is written.
 *   errors      : a plan not made from raw inputs, a plan with AGPL_PLAN_NO_MARGINALS, N != the plan's N, a null plan / x / beta /
 *               gamma / grad_z_out, exactly one of G, g -> AGPL_ERR_INVALID_ARGUMENT; a non-finite x -> AGPL_ERR_DOMAIN with its
 *               index (the outputs are then not meaningful).  The context stays usable after every error.
 *   The call waits once, at its end (the domain check of x).                                                                     */
AGPL_API int32_t agpl_plan_inducing_grad(agpl_plan *plan, int64_t N, const double *x, const float *mu0, const float *beta,
                                         const float *gamma, const double *G, const double *g, double *grad_theta_out,
                                         double *grad_z_out);

#ifdef __cplusplus
}
#endif
#endif /* AGPL_ZGRAD_H */
