// agpl_kernel_rules.h -- the stationary covariance functions a plan can be built from (include/agpl_kernels.h), each stated ONCE:
// kappa(r) = k / variance as a function of the scaled squared distance r^2 = sum_d ((x_d - x'_d) / ell_d)^2 and one parameter,
// KernelFunctions.jl's conventions.  r^2 arrives in float64 and r = sqrt(r^2) is formed in float64; T = the arithmetic type of
// everything after that (the exponential or power): float64 for K_ZZ (se_kzz_kernel), float32 for the feature generator
// (se_build_kernel, one instantiation per kind).  The float32 squared-exponential rule is the expression the generator always had:
// do not reassociate.
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
    default: return kernel_drule<AGPL_KERNEL_SE, T>(r2, param);
    }
}

__host__ __device__ inline bool kernel_kind_known(int kind) { return kind >= AGPL_KERNEL_SE && kind <= AGPL_KERNEL_RQ; }

// kappa(r) of a run-time kind: one uniform switch (K_ZZ, once per plan; the generator dispatches on the host instead)
template <typename T>
__host__ __device__ inline T kernel_value(int kind, double r2, double param) {
    switch (kind) {
    case AGPL_KERNEL_MATERN12: return kernel_rule<AGPL_KERNEL_MATERN12, T>(r2, param);
    case AGPL_KERNEL_MATERN32: return kernel_rule<AGPL_KERNEL_MATERN32, T>(r2, param);
    case AGPL_KERNEL_MATERN52: return kernel_rule<AGPL_KERNEL_MATERN52, T>(r2, param);
    case AGPL_KERNEL_RQ: return kernel_rule<AGPL_KERNEL_RQ, T>(r2, param);
    default: return kernel_rule<AGPL_KERNEL_SE, T>(r2, param);
    }
}

} // namespace agpl
