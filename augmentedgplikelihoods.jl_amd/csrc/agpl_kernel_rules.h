// agpl_kernel_rules.h -- the stationary covariance functions a plan can be built from (include/agpl_kernels.h), each stated ONCE:
// kappa(r) = k / variance as a function of the scaled squared distance r^2 = sum_d ((x_d - x'_d) / ell_d)^2 and one parameter,
// KernelFunctions.jl's conventions.  r^2 arrives in float64 and r = sqrt(r^2) is formed in float64; T = the arithmetic type of
// everything after that (the exponential or power): float64 for K_ZZ (se_kzz_kernel), float32 for the feature generator
// (se_build_kernel, one instantiation per kind).  The float32 squared-exponential rule is the expression the generator always had:
// do not reassociate.  The periodic kinds are the squared exponential's rule on a warped distance: kernel_dim_warped and kernel_warp
// below are the one place that states which terms of r^2 a kind warps, and how.  The squared exponential x cosine kind warps nothing and
// multiplies kappa by a factor of the last dimension's difference: kernel_dim_modulated and kernel_modulation state that once.
#pragma once
#include "../../include/agpl_kernels.h"
#include "agpl_common.h"

namespace agpl {

__host__ __device__ inline float kernel_exp(float v) { return expf(v); }
__host__ __device__ inline double kernel_exp(double v) { return exp(v); }
__host__ __device__ inline float kernel_log1p(float v) { return log1pf(v); }
__host__ __device__ inline double kernel_log1p(double v) { return log1p(v); }

// kappa(r) of KIND (a compile-time constant: the switch folds)
template <int KIND, typename T>
__host__ __device__ __forceinline__ T kernel_rule(double r2, double param) {
    switch (KIND) {
    case AGPL_KERNEL_SE: return kernel_exp((T)-0.5 * (T)r2);
    case AGPL_KERNEL_MATERN12: return kernel_exp(-(T)sqrt(r2));
    case AGPL_KERNEL_MATERN32: {
        const T u = (T)1.7320508075688772 * (T)sqrt(r2);
        return ((T)1 + u) * kernel_exp(-u);
    }
    case AGPL_KERNEL_MATERN52: {
        const T u = (T)2.23606797749979 * (T)sqrt(r2);
        return ((T)1 + u + u * u * (T)(1.0 / 3.0)) * kernel_exp(-u); // 5 r^2 / 3 = u^2 / 3
    }
    case AGPL_KERNEL_RQ: { // exp(-alpha log1p(r^2 / (2 alpha))), never pow
        const T a = (T)param;
        return kernel_exp(-a * kernel_log1p((T)r2 / ((T)2 * a)));
    }
    case AGPL_KERNEL_PERIODIC: return kernel_exp((T)-0.5 * (T)r2); // the squared exponential's, on the warped distance (kernel_warp)
    case AGPL_KERNEL_SE_PERIODIC: return kernel_exp((T)-0.5 * (T)r2); // the same, warped in the last dimension only
    case AGPL_KERNEL_SE_COSINE: return kernel_exp((T)-0.5 * (T)r2); // the squared exponential's: the cosine is a factor beside it (kernel_modulation)
    }
    return (T)0;
}

// kappa'(r) / r of KIND, so that d kappa / d log ell_d = -(kappa'(r) / r) ((x_d - x'_d) / ell_d)^2 (include/agpl_hyper.h), in closed
// form with the limit at r = 0 where there is one: SE -kappa; Matern-3/2 -3 exp(-sqrt3 r); Matern-5/2 -(5/3)(1 + sqrt5 r) exp(-sqrt5 r);
// RQ -kappa / (1 + r^2 / (2 alpha)).  Matern-1/2, -exp(-r) / r, has no limit (kappa is not differentiable at 0): 0 at r = 0.
template <int KIND, typename T>
__host__ __device__ __forceinline__ T kernel_drule(double r2, double param) {
    switch (KIND) {
    case AGPL_KERNEL_SE: return -kernel_exp((T)-0.5 * (T)r2);
    case AGPL_KERNEL_MATERN12: {
        const T r = (T)sqrt(r2);
        return r > (T)0 ? -kernel_exp(-r) / r : (T)0;
    }
    case AGPL_KERNEL_MATERN32: return (T)-3 * kernel_exp(-(T)1.7320508075688772 * (T)sqrt(r2));
    case AGPL_KERNEL_MATERN52: {
        const T u = (T)2.23606797749979 * (T)sqrt(r2);
        return (T)(-5.0 / 3.0) * ((T)1 + u) * kernel_exp(-u);
    }
    case AGPL_KERNEL_RQ: {
        const T a = (T)param, q = (T)r2 / ((T)2 * a);
        return -kernel_exp(-a * kernel_log1p(q)) / ((T)1 + q);
    }
    case AGPL_KERNEL_PERIODIC: return -kernel_exp((T)-0.5 * (T)r2);
    case AGPL_KERNEL_SE_PERIODIC: return -kernel_exp((T)-0.5 * (T)r2);
    case AGPL_KERNEL_SE_COSINE: return -kernel_exp((T)-0.5 * (T)r2);
    }
    return (T)0;
}

// kappa'(r) / r of a run-time kind (the K_ZZ part of the hyperparameter gradient, float64)
template <typename T>
__host__ __device__ inline T kernel_dvalue(int kind, double r2, double param) {
    switch (kind) {
    case AGPL_KERNEL_MATERN12: return kernel_drule<AGPL_KERNEL_MATERN12, T>(r2, param);
    case AGPL_KERNEL_MATERN32: return kernel_drule<AGPL_KERNEL_MATERN32, T>(r2, param);
    case AGPL_KERNEL_MATERN52: return kernel_drule<AGPL_KERNEL_MATERN52, T>(r2, param);
    case AGPL_KERNEL_RQ: return kernel_drule<AGPL_KERNEL_RQ, T>(r2, param);
    // (AGPL_KERNEL_PERIODIC, AGPL_KERNEL_SE_PERIODIC, AGPL_KERNEL_SE_COSINE: the squared exponential's rule, the default)
    default: return kernel_drule<AGPL_KERNEL_SE, T>(r2, param);
    }
}

__host__ __device__ inline bool kernel_kind_known(int kind) {
    return (kind >= AGPL_KERNEL_SE && kind <= AGPL_KERNEL_RQ) || kind == AGPL_KERNEL_PERIODIC || kind == AGPL_KERNEL_SE_PERIODIC ||
           kind == AGPL_KERNEL_SE_COSINE;
}

// Which terms of r^2 a kind warps, stated ONCE: AGPL_KERNEL_PERIODIC every dimension, AGPL_KERNEL_SE_PERIODIC the last one (d == D - 1:
// squared exponential in the leading dimensions, periodic in the last), any other kind none.  A new warped kind is added HERE and
// nowhere else in this file.
__host__ __device__ constexpr bool kernel_dim_warped(int kind, int d, int D) {
    return kind == AGPL_KERNEL_PERIODIC || (kind == AGPL_KERNEL_SE_PERIODIC && d == D - 1);
}
// some dimension of the kind is warped: derived from the predicate above (at the largest D a plan takes), not a second list of kinds
__host__ __device__ constexpr bool kernel_kind_warps(int kind) {
    for (int d = 0; d < 16; ++d)
        if (kernel_dim_warped(kind, d, 16)) return true;
    return false;
}

// Which dimensions carry a factor that is NOT a function of r^2, stated ONCE: AGPL_KERNEL_SE_COSINE the last one (d == D - 1), any other
// kind none.  Such a kind warps nothing: its r^2 is the scaled Euclidean one and its kappa the squared exponential's; k is
// variance kappa(r^2) m with m = kernel_modulation below, so every derivative of k in x, z has a product rule in that dimension
// (d k / d log ell_d has none: m does not depend on ell).
__host__ __device__ constexpr bool kernel_dim_modulated(int kind, int d, int D) { return kind == AGPL_KERNEL_SE_COSINE && d == D - 1; }
// some dimension of the kind is modulated: derived from the predicate above, as kernel_kind_warps is
__host__ __device__ constexpr bool kernel_kind_modulated(int kind) {
    for (int d = 0; d < 16; ++d)
        if (kernel_dim_modulated(kind, d, 16)) return true;
    return false;
}
// The factor of a modulated dimension and its derivative, in float64, from the scaled difference us = (x_d - x'_d) / ell_d the callers
// hold and w = ell_d / param (param = the period p; the table slot the periodic kinds fill): m = cos(2 pi (x_d - x'_d) / p) =
// cospi(2 us w), d m / d us = -2 pi w sinpi(2 us w).  cospi is even bit for bit and us of (x', x) is -us of (x, x') exactly, so m is
// symmetric in its two points to the bit.
__device__ __forceinline__ double kernel_modulation(double us, double w) { return cospi(2.0 * us * w); }
__device__ __forceinline__ double kernel_dmodulation(double us, double w) { return -6.283185307179586 * w * sinpi(2.0 * us * w); }
// the same two of a run-time kind for dimension d of D, from ell_d and param themselves (K_ZZ, the greedy selector, as kernel_warp_value
// below): 1 and 0 where the kind does not modulate d
__device__ inline double kernel_modulation_value(int kind, int d, int D, double us, double ell, double param) {
    return kernel_dim_modulated(kind, d, D) ? kernel_modulation(us, ell / param) : 1.0;
}
__device__ inline double kernel_dmodulation_value(int kind, int d, int D, double us, double ell, double param) {
    return kernel_dim_modulated(kind, d, D) ? kernel_dmodulation(us, ell / param) : 0.0;
}
// -(d^2 k / d tau_d^2)(0) / variance, tau_d = x_d - x'_d, is the envelope's c0 u'(0)^2 / ell_d^2 (c0 = -lim kappa'(r) / r at 0, u'(0) =
// kernel_dwarp_at_zero below) PLUS the factor's own curvature, this: (2 pi / p)^2 in a modulated dimension, 0 else.  So the prior
// variance of d f / d x_d is variance (1 / ell_d^2 + (2 pi / p)^2) there, and the normalisation of that dimension's derivative feature
// (agpl_grad.hip, agpl_se_build.h) is c = c0 u'(0)^2 + this ell_d^2 = 1 + (2 pi ell_d / p)^2.  It needs no lengthscale, which the host
// does not hold: the device multiplies by ell_d^2.
__host__ __device__ inline double kernel_modulation_curvature(int kind, int d, int D, double param) {
    const double a = 6.283185307179586 / param;
    return kernel_dim_modulated(kind, d, D) ? a * a : 0.0;
}

// The distance rule: the term u_d of r^2 = sum_d u_d^2, stated ONCE.  Every caller holds coordinates already divided by ell_d, so
// the rule takes the scaled difference us = (x_d - x'_d) / ell_d, w = ell_d / param and inv_ell = 1 / ell_d (per dimension; the
// caller forms them once, not per pair).  Kinds 0 - 4: u_d = us, the expression the callers always had (w and inv_ell are not
// read).  A warped dimension (kernel_dim_warped; param = the period p): u_d = sinpi((x_d - x'_d) / p) / ell_d = sinpi(us w) inv_ell, in
// float64.  KIND is a compile-time constant: the branch folds.  For a kind that warps only some dimensions (AGPL_KERNEL_SE_PERIODIC)
// these two are the rule of a warped one; the caller takes us and 1 for the others, as kernel_dim_warped says.
template <int KIND>
__device__ __forceinline__ double kernel_warp(double us, double w, double inv_ell) {
    if constexpr (kernel_kind_warps(KIND)) return sinpi(us * w) * inv_ell;
    return us;
}
// d u_d / d us (= ell_d d u_d / d (x_d - x'_d)): 1 for kinds 0 - 4; (pi / p) cospi((x_d - x'_d) / p) = pi w inv_ell cospi(us w) for the
// periodic kind, so that d r^2 / d (x_d / ell_d) = 2 u_d (d u_d / d us).
template <int KIND>
__device__ __forceinline__ double kernel_dwarp(double us, double w, double inv_ell) {
    if constexpr (kernel_kind_warps(KIND)) return 3.141592653589793 * w * inv_ell * cospi(us * w);
    return 1.0;
}
// the same two for dimension d of D of a compile-time kind: the rule where the kind warps d (kernel_dim_warped), us and 1 else.  Kinds
// 0 - 4 and AGPL_KERNEL_PERIODIC fold to what kernel_warp / kernel_dwarp give; AGPL_KERNEL_SE_PERIODIC keeps one uniform test of d.
template <int KIND>
__device__ __forceinline__ double kernel_warp_dim(int d, int D, double us, double w, double inv_ell) {
    return kernel_dim_warped(KIND, d, D) ? kernel_warp<KIND>(us, w, inv_ell) : us;
}
template <int KIND>
__device__ __forceinline__ double kernel_dwarp_dim(int d, int D, double us, double w, double inv_ell) {
    return kernel_dim_warped(KIND, d, D) ? kernel_dwarp<KIND>(us, w, inv_ell) : 1.0;
}
// the same two of a run-time kind, from ell_d and param themselves (K_ZZ, the greedy selector: one uniform branch, once per plan
// or per pivot, so the two divisions are not hoisted), for dimension d of D
__device__ inline double kernel_warp_value(int kind, int d, int D, double us, double ell, double param) {
    return kernel_dim_warped(kind, d, D) ? kernel_warp<AGPL_KERNEL_PERIODIC>(us, ell / param, 1.0 / ell) : us;
}
__device__ inline double kernel_dwarp_value(int kind, int d, int D, double us, double ell, double param) {
    return kernel_dim_warped(kind, d, D) ? kernel_dwarp<AGPL_KERNEL_PERIODIC>(us, ell / param, 1.0 / ell) : 1.0;
}
// d u_d / d us at us = 0 (host), per dimension: pi / param for a warped one, 1 else.  Its square scales the prior variance of
// d f / d x_d and the normalisation c of that dimension's derivative feature (agpl_grad.hip)
inline double kernel_dwarp_at_zero(int kind, int d, int D, double param) {
    return kernel_dim_warped(kind, d, D) ? 3.141592653589793 / param : 1.0;
}
// the one check of a kind's parameter (host): NULL, or what the message names.  below: the caller's own bound of "finite"
// (agpl_se_create: < 1e300, as its variance and jitter; the greedy selector: <= 1.79e308, as its lengthscales), kept per site.
inline const char *kernel_param_refused(int kind, double param, double below, bool inclusive) {
    const bool ok = param > 0.0 && (inclusive ? param <= below : param < below);
    if (kind == AGPL_KERNEL_RQ && !ok) return "alpha of the rational quadratic kernel";
    if (kind == AGPL_KERNEL_PERIODIC && !ok) return "the period p of the periodic kernel";
    if (kind == AGPL_KERNEL_SE_PERIODIC && !ok) return "the period p of the squared exponential x periodic kernel";
    if (kind == AGPL_KERNEL_SE_COSINE && !ok) return "the period p of the squared exponential x cosine kernel";
    return nullptr;
}
inline bool kernel_has_param(int kind) { return kind == AGPL_KERNEL_RQ || kernel_kind_warps(kind) || kernel_kind_modulated(kind); }

// kappa(r) of a run-time kind: one uniform switch (K_ZZ, once per plan; the generator dispatches on the host instead)
template <typename T>
__host__ __device__ inline T kernel_value(int kind, double r2, double param) {
    switch (kind) {
    case AGPL_KERNEL_MATERN12: return kernel_rule<AGPL_KERNEL_MATERN12, T>(r2, param);
    case AGPL_KERNEL_MATERN32: return kernel_rule<AGPL_KERNEL_MATERN32, T>(r2, param);
    case AGPL_KERNEL_MATERN52: return kernel_rule<AGPL_KERNEL_MATERN52, T>(r2, param);
    case AGPL_KERNEL_RQ: return kernel_rule<AGPL_KERNEL_RQ, T>(r2, param);
    // (AGPL_KERNEL_PERIODIC, AGPL_KERNEL_SE_PERIODIC, AGPL_KERNEL_SE_COSINE: the squared exponential's rule, the default)
    default: return kernel_rule<AGPL_KERNEL_SE, T>(r2, param);
    }
}

} // namespace agpl
