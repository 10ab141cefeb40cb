/*
 * agpl_chain.h -- C ABI of libagpl_chain.so: the posterior of f at new inputs from a CHAIN of inducing draws (the output of Gibbs
 * sweeps, or draws of q(v) from agpl_gibbs_draw_v), for plans of the squared-exponential model (include/agpl_se.h).
 *
 * An extension of libagpl.so (include/agpl.h): it links against libagpl.so, takes the plans agpl_plan_create_se returns and keeps
 * agpl.h's conventions -- int32 status, device pointers, the context's stream, errors through agpl_last_error of the context.  Kept
 * in its own library so that agpl.h / libagpl.so stay the 45 entry points of AGPL_VERSION 121, agpl_se.h / libagpl_se.so their
 * four and agpl_predictive.h / libagpl_predictive.so its one.
 */
#ifndef AGPL_CHAIN_H
#define AGPL_CHAIN_H

#include "agpl.h"

#ifdef __cplusplus
extern "C" {
#endif

/*
 * Given draws v_t (t < T) of the whitened inducing coordinates, the posterior of f at x* is the equal-weight mixture over t of
 * N(mu0 + phi(x*)' v_t, d*), d* = variance - |phi(x*)|^2 (u_posterior of examples/bernoulli/script.jl applied to each Gibbs sample).
 * agpl_plan_predict_chain computes the per-draw conditional means and their first two moments over the chain:
 *   V          [T][L][M] float64, device: the chain (M: the caller's feature count), T >= 1
 *   x_s        [Ns][D]   float64, device;  mu0_s [L][Ns] float32 or NULL
 *   mean_out   [L][Ns] float32:  mu0 + (1/T) sum_t phi' v_t
 *   spread_out [L][Ns] float32:  (1/T) sum_t (phi' (v_t - vbar))^2        (between-draw variance of the conditional mean)
 *   resid_out  [Ns]    float32 or NULL:  d* = variance - |phi|^2 (agpl_plan_create's clamp); Var f* = resid + spread
 *   F_out      [T][L][Ns] float32 or NULL:  mu0 + phi' v_t, the per-draw conditional means ("function samples")
 * for a plan made by agpl_plan_create_se, with or without the marginal image (AGPL_PLAN_NO_MARGINALS: the plan of Gibbs sweeps).
 *   features  : phi is the plan's own generator at the plan's own scale, in chunks of 65536 points whose marginal image goes to the
 *               plan's prediction scratch (agpl_plan_predict's; grown here if needed, freed with the plan): at the plan's training
 *               x the features are bit for bit those agpl_plan_features decodes.
 *   numerics  : vbar = (1/T) sum_t v_t in float64; the centred draws v_t - vbar and vbar are packed as split float16 (hi + lo), each
 *               with a power-of-two scale from its largest magnitude, and projected on the matrix cores
 *               (v_mfma_f32_32x32x16_f16: hi hi + hi lo + lo hi, float32 accumulation).  The spread is the mean square of the
 *               CENTRED projections -- never a difference of two sums: a tight chain far from the origin keeps its digits; T = 1
 *               gives spread = 0 exactly.  Reductions run in a fixed order, without float atomics: every output of a point depends
 *               on that point's x and on V only (not on Ns, the point's position or chunk, or the launch).
 *   errors    : a plan not made by agpl_plan_create_se, T < 1, Ns < 0, a null V / x_s / mean_out / spread_out ->
 *               AGPL_ERR_INVALID_ARGUMENT; a non-finite entry of V -> AGPL_ERR_DOMAIN naming the first such draw (nothing is
 *               written); a non-finite x_s gives NaN at that point only (as agpl_plan_predict); Ns = 0 -> AGPL_OK.  The context
 *               stays usable after every error.
 *   The call waits once, behind the pass that packs V (its domain check); the feature build and the projection of every chunk are
 *   enqueued behind it on the context's stream and the call returns without waiting for them.                                     */
AGPL_API int32_t agpl_plan_predict_chain(agpl_plan *plan, int32_t T, const double *V, int64_t Ns, const double *x_s,
                                         const float *mu0_s, float *mean_out, float *spread_out, float *resid_out, float *F_out);

#ifdef __cplusplus
}
#endif
#endif /* AGPL_CHAIN_H */
