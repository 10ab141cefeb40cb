/*
 * agpl_greedy.h -- C ABI of libagpl_greedy.so: inducing inputs chosen from the data by greedy conditional variance, i.e. the partial
 * pivoted Cholesky factorisation of K_XX (Burt, Rasmussen, van der Wilk, JMLR 2020; ConditionalVariance of GPflow's robustgp), for
 * the five stationary covariance functions of include/agpl_kernels.h.  Repeatedly the data point whose prior variance given the
 * inputs chosen so far is largest is taken; that residual d_i = k_ii - k_iZ K_ZZ^-1 k_Zi is the Nystrom residual every plan carries,
 * its sum is tr(K - Q), and "stop when max d <= threshold variance" chooses how many inputs are needed.
 *
 * An extension of libagpl.so (include/agpl.h): it links against libagpl.so and keeps agpl.h's conventions -- int32 status, device
 * pointers, the context's stream, errors through agpl_last_error of the context.  Kept in its own library so that agpl.h /
 * libagpl.so stay the 45 entry points of AGPL_VERSION 121 and the other extension libraries their own.
 *
 * THE ALGORITHM (stated once, here).  The arithmetic is float64 throughout; x is float64 [n][D].  State of a range of points:
 * the residual d [n] and the columns cols [Mmax][n] (column-major: a column is contiguous over the points).
 *   Start.     d_i = variance.
 *   Pick.      p = argmax_i d_i over all points of all ranges; on an exact tie the lowest global index wins.  Selection ends before
 *              step j if d_p <= threshold variance.
 *   Column j.  c_i = (variance kappa(r2(x_i, x_p)) - S_i) / sqrt(d_p),   S_i = sum over t < j of cols[t][i] cols[t][p],
 *              r2 = sum over the dimensions ascending of (x_id / ell_d - x_pd / ell_d)^2, every term a fused multiply-add into one
 *              accumulator; kappa is the float64 rule of the kind (csrc/agpl_kernel_rules.h); S_i is summed over t ASCENDING,
 *              every term a fused multiply-add into ONE accumulator per point, starting from 0.  The order is part of the contract.
 *   Update.    d_i <- max(d_i - c_i c_i, 0) (a product, then a difference: two roundings); the pivot's own d is set to exactly 0.
 * Every number formed belongs to one point and no floating-point sum crosses a point, so the selection is the same bits however the
 * points are split over ranks, workgroups or launches.
 *
 * The trace.  After step j every range adds ONE int64 into trace_acc[j]: the sum over its points of
 *     rint((d_i / variance) 2^s)  (ties to even),   s = 61 - ceil(log2 N_total),
 * so that tr(K - Q) / variance = trace_acc[j] 2^-s.  d_i <= variance, so the sum over N_total <= 2^(61 - s) points stays below 2^62;
 * integer sums are exact, so the trace is independent of the split too.  No float atomics anywhere.
 *
 * The candidate record of a range: int64 [2] = {the bit pattern of its largest d, the GLOBAL index of the first point that holds it};
 * an empty range writes {-1, INT64_MAX}.  Non-negative doubles order as their bit patterns: ranks combine by MAX of word 0, then MIN of
 * word 1 among the ranks that hold that maximum.
 * The pivot record of step j: float64 [D + 1 + j] = x_p (input units), d_p, cols[0 .. j)[p].  The range that owns p writes it, every
 * other range writes zeros, so that ranks combine by a sum with one owner (as agpl_kmeans_seed of include/agpl_inducing.h).
 *
 * The work area of a range (caller-owned device memory, agpl_greedy_bytes(n, Mmax) bytes, 8-byte aligned), in this order:
 *     cols     float64 [Mmax][n]      at byte 0
 *     d        float64 [n]            at byte 8 Mmax n
 *     partials int64 [1024][2]        at byte 8 (Mmax + 1) n   (per-workgroup argmax partials of the step)
 * At N = 1e7, Mmax = 512 that is 41 GB, the size of a plan.  Every entry point that takes `work` takes its size `work_bytes` and refuses
 * one below agpl_greedy_bytes.
 *
 * `lengthscale` is a HOST array of D numbers (validated before any device work); everything else with a pointer is device memory.
 * Sizes: 1 <= D <= 16, 1 <= Mmax <= 2048, 1 <= N_total < 2^48; a range [i0, i0 + n) inside the N_total points, n = 0 allowed
 * everywhere.  variance and the lengthscales positive and finite; a known kind, alpha of AGPL_KERNEL_RQ positive and finite.
 */
#ifndef AGPL_GREEDY_H
#define AGPL_GREEDY_H

#include "agpl.h"
#include "agpl_kernels.h"

#ifdef __cplusplus
extern "C" {
#endif

/* bytes_out <- the bytes of the work area of a range of n points and at most Mmax steps (a pure host function).
 * AGPL_ERR_INVALID_ARGUMENT for n outside [0, 2^48), Mmax outside [1, 2048] or a null output.                                     */
AGPL_API int32_t agpl_greedy_bytes(int64_t n, int32_t Mmax, int64_t *bytes_out);

/*
 * Start: d_i = variance over the range, and the range's candidate record.
 *   x_local  : float64 [n][D], the points i0 .. i0 + n - 1 of the N_total
 *   cand_out : int64 [2]
 * A non-finite x is AGPL_ERR_DOMAIN with its index within x_local; to report it the call waits for the stream.                   */
AGPL_API int32_t agpl_greedy_begin(agpl_ctx *ctx, int64_t N_total, int64_t i0, int64_t n, int32_t Mmax, int32_t D,
                                   const double *x_local, double variance, void *work, int64_t work_bytes, int64_t *cand_out);

/*
 * The pivot record of step j (0 <= j < Mmax) for the point with global index index[0] (device): written by the range that owns
 * it, zeros from every other range.
 *   pivot_out : float64 [D + 1 + j]
 * Asynchronous.                                                                                                                  */
AGPL_API int32_t agpl_greedy_pivot(agpl_ctx *ctx, int64_t N_total, int64_t i0, int64_t n, int32_t Mmax, int32_t D, int32_t j,
                                   const double *x_local, const void *work, int64_t work_bytes, const int64_t *index,
                                   double *pivot_out);

/*
 * ONE pass over the range's points for step j, the hot path: column j, the update of d, the range's new candidate record and its
 * integer added into trace_acc[j].  The pivot's index and record are read from device memory, so the host never waits.
 *   index     : int64 [1], the pivot's global index
 *   pivot     : float64 [D + 1 + j], the (summed) pivot record; pivot[D] = d_p must be positive
 *   cand_out  : int64 [2]
 *   trace_acc : int64 [Mmax], word j ADDED to (the caller zeroes it before the first step)
 * Asynchronous.  n = 0: the empty candidate record, nothing added.                                                               */
AGPL_API int32_t agpl_greedy_step(agpl_ctx *ctx, int64_t N_total, int64_t i0, int64_t n, int32_t Mmax, int32_t D, int32_t kind,
                                  double param, int32_t j, const double *x_local, const double *lengthscale, double variance,
                                  const int64_t *index, const double *pivot, void *work, int64_t work_bytes, int64_t *cand_out,
                                  int64_t *trace_acc);

/*
 * The one-process call: begin, then M x (pick + pivot record, step), all enqueued at once; the end of selection is a flag on the
 * device that turns the remaining launches into immediate returns.  Waits for the stream once, at the end (errors as
 * agpl_greedy_begin).  The same bits as the building blocks above driven over any split of x.  M > N is allowed: selection ends
 * once every point is taken.
 *   threshold : 1e-12 <= threshold < 1 (the floor keeps sqrt(d_p) away from the rounding residue of duplicated points)
 *   work      : agpl_greedy_bytes(N, M) bytes
 *   z_out     : float64 [M][D], the chosen inputs in input units; rows beyond the selected count are zero
 *   idx_out   : int64 [M], their indices (zero beyond the selected count)
 *   info_out  : float64 [1 + 2 M]: the selected count m; max d / variance before each pick (non-increasing); tr(K - Q) / variance
 *               after each pick, decoded from the integer sums (zero beyond m, both)                                             */
AGPL_API int32_t agpl_select_inducing_greedy(agpl_ctx *ctx, int64_t N, int32_t M, int32_t D, int32_t kind, double param,
                                             const double *x, const double *lengthscale, double variance, double threshold,
                                             void *work, int64_t work_bytes, double *z_out, int64_t *idx_out, double *info_out);

#ifdef __cplusplus
}
#endif
#endif /* AGPL_GREEDY_H */
