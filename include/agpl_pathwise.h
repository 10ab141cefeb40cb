/*
 * agpl_pathwise.h -- C ABI of libagpl_pathwise.so: pathwise (Matheron-rule) draws of the posterior FUNCTION, evaluated at any number
 * of new inputs without an Ns x Ns factor, for plans made from raw inputs (include/agpl_se.h, include/agpl_kernels.h).
 *
 * An extension of libagpl.so (include/agpl.h): it links against libagpl.so, takes the plans agpl_plan_create_se /
 * agpl_plan_create_stationary return and keeps agpl.h's conventions -- int32 status, device pointers, the context's stream, errors
 * through agpl_last_error of the context.  Kept in its own library so that agpl.h / libagpl.so stay the 45 entry points of
 * AGPL_VERSION 121 and the other eight extension libraries their sixteen.
 */
#ifndef AGPL_PATHWISE_H
#define AGPL_PATHWISE_H

#include "agpl.h"

#ifdef __cplusplus
extern "C" {
#endif

/*
 * A posterior draw is a prior function draw plus a correction through the plan's own whitened features phi(x) = L^-1 k_Z(x),
 * K_ZZ + jitter I = L L':
 *     f_tl(x) = mu0_l(x) + fp_tl(x) + phi(x)' (V_tl - L^-1 up_tl)
 * with V_tl a draw of the whitened inducing coordinates (of q(v), or one draw of a Gibbs chain), fp a draw of the prior process and
 * up = fp(Z) + sqrt(jitter) xi (the jitter noise makes Cov(up) = L L' for an exact prior draw).  The prior draw is a sum of F random
 * Fourier features of the kernel's spectral measure, which the CALLER draws (the rule is below):
 *     psi_j(x) = cos(omega_j . x / ell + b_j)
 *     fp_tl(x) = sigma sqrt(2 / F) sum_j W_tlj psi_j(x)
 *     up_tl    = fp_tl(Z) + sqrt(jitter) Xi_tl
 *     c_tl     = V_tl - L^-1 up_tl
 *     F_out[t][l][i] = mu0 + sigma sqrt(2 / F) psi(x_i)' W_tl + phi(x_i)' c_tl
 *   V      [T][L][M] float64: draws of the whitened inducing coordinates (M: the caller's feature count), T >= 1
 *   omega  [F][D]    float64: frequencies in the scaled units u = x / ell;  phase [F] float64: b_j;  1 <= F <= 8192
 *   W      [T][L][F] float64: standard-normal weights
 *   Xi     [T][L][M] float64 or NULL: standard-normal jitter noise (NULL: none)
 *   x_s    [Ns][D]   float64;  mu0_s [L][Ns] float32 or NULL;  F_out [T][L][Ns] float32
 * all on the device, for a plan made from raw inputs, with or without the marginal image (AGPL_PLAN_NO_MARGINALS).
 *   spectral rule : with n ~ N(0, I_D) and b ~ U[0, 2 pi),  squared exponential: omega = n;  Matern-nu (nu = 1/2, 3/2, 5/2):
 *               omega = n sqrt(2 nu / c), c ~ chi^2(2 nu);  rational quadratic: omega = n sqrt(tau), tau ~ Gamma(shape alpha,
 *               scale 1 / alpha).  Then E cos(omega . (u - u')) = kappa(|u - u'|) of include/agpl_kernels.h.
 *               periodic (period p): the measure is discrete.  With a_d = 1 / (4 ell_d^2),
 *               exp(-sin^2(pi delta / p) / (2 ell_d^2)) = sum_{k in Z} e^-a_d I_k(a_d) cos(2 pi k delta / p): per feature and dimension
 *               an integer k_d with probability e^-a_d I_|k|(a_d), omega_d = 2 pi k_d ell_d / p (so that omega . x / ell is
 *               2 pi k . x / p).  The weights by the ratio recurrence I_k / I_{k-1} = 1 / (2 k / a + I_{k+1} / I_k) in float64 on the
 *               host, normalised by their sum and truncated where the tail mass is below 1e-16.
 *               squared exponential x periodic (AGPL_KERNEL_SE_PERIODIC): omega_d = n_d for d < D - 1, the last as the periodic kind's.
 *               squared exponential x cosine (AGPL_KERNEL_SE_COSINE): omega_d = n_d for every d, then the last moved by +-2 pi ell_{D-1} / p
 *               with a fair sign per feature (the Gaussian measure shifted to the cosine's two frequencies), so that
 *               E cos(omega . du) = exp(-|du|^2 / 2) cos(2 pi ell_{D-1} du_{D-1} / p).
 *   approximation : with F features the draws have covariance B'B + jitter q'q + phi' S phi, B = sigma sqrt(2 / F) (Psi(x) -
 *               Psi(Z) L^-T phi), q = L^-T phi, S = Cov(V): it differs from the exact k - phi' phi + phi' S phi by O(sigma^2 /
 *               sqrt(F)).  Their mean, mu0 + phi' E V, is exact.
 *   set-up    : once per call, in float64: L^-1 from the plan's z / ell and its stored jitter (the route of agpl_plan_hyper_grad),
 *               Psi(Z)' W, + sqrt(jitter) Xi, L^-1 times it, c = V - that.
 *   features  : phi is the plan's own generator at the plan's own scale, in chunks of 65536 points whose marginal image goes to the
 *               plan's prediction scratch (grown here if needed, freed with the plan), as agpl_plan_predict_chain.  Psi is written
 *               as a second split-float16 image in the same blocked layout: the phase b_j + sum_d omega_jd u_d in float64 (d
 *               ascending, fused multiply-add), reduced to one period in float64 (t = p / 2 pi - rint(p / 2 pi)), the cosine of
 *               2 pi t in float32; F padded with zero features to a multiple of 16; at most 256 MiB (a chunk is walked in
 *               sub-chunks of floor(256 MiB / (4 Fp)) points, a multiple of 128 and at least 128).
 *   numerics  : rows [c_tl ; sigma sqrt(2 / F) W_tl] are packed as split float16 (hi + lo) and projected on the matrix cores
 *               (v_mfma_f32_32x32x16_f16: hi hi + hi lo + lo hi, float32 accumulation), the features of phi first, then those of
 *               psi, into ONE accumulator: the power-of-two scales 2^ec (c), 2^ew (W) and 2^epsi (the Psi image) are chosen with
 *               e_phi + ec = epsi + ew, 0 <= epsi <= 14, each as large as float16 allows.  The draws are not centred.  Reductions
 *               run in a fixed order, without float atomics: an output depends on its x, the call's arrays and the plan only (not
 *               on Ns, the point's position, chunk or sub-chunk, or the launch).
 *   errors    : a plan not made from raw inputs, T < 1, F outside 1 .. 8192, Ns < 0, a null plan / V / omega / phase / W / x_s /
 *               F_out -> AGPL_ERR_INVALID_ARGUMENT; a non-finite entry of V, W, Xi, omega or phase -> AGPL_ERR_DOMAIN naming the
 *               first such draw or feature (nothing is written); a non-finite x_s gives NaN at that point only; Ns = 0 -> AGPL_OK.
 *               The context stays usable after every error.
 *   The call waits once, behind the set-up (its domain check); the feature builds and the projection of every chunk are enqueued
 *   behind it on the context's stream and the call returns without waiting for them.                                               */
AGPL_API int32_t agpl_plan_sample_paths(agpl_plan *plan, int32_t T, const double *V, int32_t F, const double *omega,
                                        const double *phase, const double *W, const double *Xi, int64_t Ns, const double *x_s,
                                        const float *mu0_s, float *F_out);

#ifdef __cplusplus
}
#endif
#endif /* AGPL_PATHWISE_H */
