/*
 * agpl_inducing.h -- C ABI of libagpl_inducing.so: inducing inputs chosen from the data by Lloyd's k-means on the device, in the
 * covariance functions' own metric u = x / ell per dimension (the r^2 of every kind of include/agpl_kernels.h), so that the z it
 * returns serves agpl_plan_create_se / agpl_plan_create_stationary as it is (KmeansAlg of InducingPoints.jl).
 * (That metric is not the periodic kinds', AGPL_KERNEL_PERIODIC and AGPL_KERNEL_SE_PERIODIC, whose distance is warped: these entry
 * points take no kind, so the Python driver refuses select_inducing(kernel=("periodic", p)) and ("se_periodic", p) as unsupported and
 * points to agpl_select_inducing_greedy.  It refuses ("se_cosine", p), AGPL_KERNEL_SE_COSINE, likewise: the metric is that kind's
 * envelope's, but it does not see the cosine factor, which changes sign inside a cluster.)
 *
 * An extension of libagpl.so (include/agpl.h): it links against libagpl.so and keeps agpl.h's conventions -- int32 status, device
 * pointers, the context's stream, errors through agpl_last_error of the context.  Kept in its own library so that agpl.h /
 * libagpl.so stay the 45 entry points of AGPL_VERSION 121 and the other five extension libraries their own.
 *
 * SHARD-EXACT: the centres are the same bits however the points are split over ranks, workgroups or launches.  A step does not sum
 * floating-point numbers across points: it adds INTEGERS (a count, the coordinates and the squared distance in fixed point) into
 * `acc`, int64 [M][D + 2], with 64-bit integer atomics (LDS, then global memory); integer sums are associative, so `acc` after all
 * ranges of the points have been added does not depend on the split, the order, the grid or the number of calls.  No float atomics.
 *
 * The fixed-point rule (stated once, here; agpl_kmeans_quanta evaluates it): with bound = f 2^eb, 1/2 <= f < 1 (frexp: bound <
 * 2^eb), cl = ceil(log2 N_total), cd = ceil(log2 D),
 *     sx = 61 - cl - eb                 a coordinate u_d = x_d / ell_d enters as  rint(u_d 2^sx)      (ties to even)
 *     sd = 61 - cl - 2 eb - 2 - cd      a squared distance r2 enters as           rint(min(r2, 4 D bound^2) 2^sd)
 * (each clamped to [-1000, 1000]).  |u_d| <= bound < 2^eb gives |rint(u_d 2^sx)| <= 2^(61 - cl), and r2 <= 4 D bound^2 <
 * 2^(2 eb + 2 + cd) the same for the distance; at most N_total <= 2^cl points add into a column, so no column can exceed 2^61 <
 * 2^62 -- the count (<= N_total) least of all.  (The clamp of r2 binds only when NO centre lies within the box of the data.)  A
 * centre's coordinate is off the float64 mean of its points by at most half a quantum, 2^-(sx + 1) <= bound 2^(cl - 61) in u.
 *
 * `lengthscale` is a HOST array of D numbers (validated before any device work); everything else with a pointer is device memory.
 * Sizes: 1 <= D <= 16, 1 <= M <= 2048, M <= N_total < 2^48.
 */
#ifndef AGPL_INDUCING_H
#define AGPL_INDUCING_H

#include "agpl.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The rule above as a pure host function: sx_out, sd_out <- the two exponents.  AGPL_ERR_INVALID_ARGUMENT (ctx may be NULL: no
 * message then) for a bound that is not positive and finite, N_total outside [1, 2^48), D outside [1, 16] or a null output.      */
AGPL_API int32_t agpl_kmeans_quanta(agpl_ctx *ctx, double bound, int64_t N_total, int32_t D, int32_t *sx_out, int32_t *sd_out);

/*
 * A stratified start: centre j is the data point with global index
 *     idx_j = lo_j + floor(u_j (hi_j - lo_j)),   lo_j = floor(j N_total / M),  hi_j = floor((j + 1) N_total / M),
 * in integer arithmetic (u_j = (k_j + 1/2) 2^-52: idx_j = lo_j + floor(k_j (hi_j - lo_j) / 2^52)), so lo_j <= idx_j < hi_j always and
 * the indices are distinct (N_total >= M).  u_j is the first uniform of the Philox stream (context seed, stream j, sweep 0) on
 * sub-stream 0xFFFFFF of csrc/agpl_random.h, reserved for this purpose (the sampler's sub-streams end below 2^22).
 *   x_local : float64 [n][D], the points i0 .. i0 + n - 1 of the N_total
 *   z_out   : float64 [M][D]: the rows this range owns; every other row is written as zeros, so that ranks combine by a sum
 *   idx_out : int64 [M] or NULL: all M indices (the same from every range)
 * Asynchronous on the context's stream.  n = 0: all rows zero.                                                                  */
AGPL_API int32_t agpl_kmeans_seed(agpl_ctx *ctx, int64_t N_total, int64_t i0, int64_t n, int32_t M, int32_t D,
                                  const double *x_local, double *z_out, int64_t *idx_out);

/* max over the n points and D dimensions of |x_d / ell_d|, non-finite values left out (agpl_kmeans_step reports those), merged
 * into bound_inout[0] (device, one float64 >= 0; the caller starts it at zero; ranks combine by a max).  Asynchronous.          */
AGPL_API int32_t agpl_kmeans_bound(agpl_ctx *ctx, int64_t n, int32_t D, const double *x_local, const double *lengthscale,
                                   double *bound_inout);

/*
 * ONE pass over the points, the hot path.  For each point the nearest centre: r2_j = sum over d ascending of (x_d / ell_d -
 * z_jd / ell_d)^2 in float64, one accumulator per (point, centre), every term a fused multiply-add; the smallest r2 wins and on an
 * exact tie the lowest j: the assignment is a pure function of (x_i, Z, ell).  Then acc[j] += (1, rint(u_d 2^sx) for d < D,
 * rint(min(r2_j, 4 D bound^2) 2^sd)) by the rule above.
 *   bound      : an upper bound of max |x_d / ell_d| over ALL N_total points of all ranks (agpl_kmeans_bound)
 *   acc        : int64 [M][D + 2], ADDED to (the caller zeroes it before the first range)
 *   assign_out : int32 [n] or NULL: the assignment (-1 for a point that was refused)
 * Errors: AGPL_ERR_DOMAIN with the index -- a non-finite x (index within x_local), a point beyond `bound`, a non-finite z; such a
 * point adds nothing.  To report them the call waits for the stream.  n = 0: AGPL_OK, nothing added, nothing launched.           */
AGPL_API int32_t agpl_kmeans_step(agpl_ctx *ctx, int64_t N_total, int64_t n, int32_t M, int32_t D, const double *x_local,
                                  const double *lengthscale, const double *z, double bound, int64_t *acc, int32_t *assign_out);

/*
 * The centres of a summed acc: z_jd = ell_d * (((double)acc[j][1 + d] / (double)acc[j][0]) * 2^-sx), in input units; a centre with
 * count 0 keeps its value (deterministic, no data access).  Every rank calls this itself on the summed acc and ends with the same
 * bits.
 *   info_out : float64 [3] (device) or NULL: the number of empty centres, the largest movement of a centre in the scaled metric
 *              (sqrt of sum_d ((z_new - z_old)_d / ell_d)^2), and the cost sum_i min_j r2 = (the integer sum of column D + 1) 2^-sd.
 * Asynchronous.                                                                                                                  */
AGPL_API int32_t agpl_kmeans_centres(agpl_ctx *ctx, int64_t N_total, int32_t M, int32_t D, const double *lengthscale, double bound,
                                     const int64_t *acc, double *z_inout, double *info_out);

/*
 * The one-process convenience: bound by a max pass of its own (an all-zero x counts as bound = 1), the stratified start unless z0
 * (float64 [M][D], device) is given, niter x (zero acc, step, centres), then one last step for the final cost.  niter = 0 returns
 * the start.  The same bits as the building blocks above driven over any split of x.
 *   z_out    : float64 [M][D]
 *   info_out : float64 [3] (device) or NULL: the empty centres of the final assignment, the movement of the last update (0 for
 *              niter = 0), the final cost.
 * Waits for the stream once, at the end, for the domain check (errors as agpl_kmeans_step).                                      */
AGPL_API int32_t agpl_select_inducing_kmeans(agpl_ctx *ctx, int64_t N, int32_t M, int32_t D, const double *x,
                                             const double *lengthscale, int32_t niter, const double *z0, double *z_out,
                                             double *info_out);

#ifdef __cplusplus
}
#endif
#endif /* AGPL_INDUCING_H */
