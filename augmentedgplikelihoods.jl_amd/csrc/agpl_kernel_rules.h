// agpl_kernel_rules.h -- the stationary covariance functions a plan can be built from (include/agpl_kernels.h), each stated ONCE:
// kappa(r) = k / variance as a function of the scaled squared distance r^2 = sum_d ((x_d - x'_d) / ell_d)^2 and one parameter,
// KernelFunctions.jl's conventions.  r^2 arrives in float64 and r = sqrt(r^2) is formed in float64; T = the arithmetic type of
// everything after that (the exponential or power): float64 for K_ZZ (se_kzz_kernel), float32 for the feature generator
// (se_build_kernel, one instantiation per kind).  The float32 squared-exponential rule is the expression the generator always had:
// do not reassociate.  The periodic kinds are the squared exponential's rule on a warped distance: kernel_dim_warped and kernel_warp
// below are the one place that states which terms of r^2 a kind warps, and how.  The squared exponential x cosine kind warps nothing and
// multiplies kappa by a factor of the last dimension's difference: kernel_dim_modulated and kernel_modulation state that once.  The
// additive squared exponential kind is a sum over the dimensions instead of a function of r^2: kernel_kind_additive, kernel_term.  The
// second-order additive kind adds the products of pairs of those terms: kernel_kind_additive2, kernel_sum_weight1 / 2 (its number is 40
// and not 15: tests/test_additive_se_rules_cpu.py holds that nothing between 15 and 39 is a kind, as 14 is not 12 for a test's sake).  The
// two product Matern kinds (64, 66) are a product over the dimensions of a one-dimensional Matern in each: kernel_kind_product,
// kernel_pterm, kernel_dpterm.  The product Matern-1/2 is left out: it is not differentiable, and every gradient consumer would refuse it.
// The two squared exponential x Matern kinds (70, 72) are the squared exponential in the leading dimensions times a one-dimensional
// Matern in the last: kernel_kind_se_matern and its helpers, which take p and t from kernel_pterm / kernel_dpterm.  The Matern-1/2 in
// the last input (71) is left out for the same reason.  The all-orders additive (ANOVA) squared exponential kind (80) is a product over
// the dimensions of (constant + one-dimensional squared exponential): kernel_kind_anova, kernel_anova_factor, kernel_anova_dfactor.
// The squared exponential x categorical kind (96) is the squared exponential's rule on a distance whose LAST param = C terms compare
// category codes for equality: kernel_kind_categorical, kernel_dim_categorical, kernel_categorical_warp.
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
    case AGPL_KERNEL_ADDITIVE_SE: break; // no function of r^2: a sum of per-dimension terms (kernel_term below)
    case AGPL_KERNEL_ADDITIVE2_SE: break; // nor this: the same terms and their pairwise products
    case AGPL_KERNEL_MATERN32_PRODUCT: break; // nor these: a product of per-dimension factors (kernel_pterm below)
    case AGPL_KERNEL_MATERN52_PRODUCT: break;
    case AGPL_KERNEL_SE_MATERN32: break; // nor these: r^2 of the leading dimensions and a factor of the last (kernel_se_matern_pterm below)
    case AGPL_KERNEL_SE_MATERN52: break;
    case AGPL_KERNEL_ANOVA_SE: break; // nor this: a product of per-dimension factors (kernel_anova_factor below)
    case AGPL_KERNEL_SE_CATEGORICAL: return kernel_exp((T)-0.5 * (T)r2); // the squared exponential's, on the warped distance (kernel_categorical_warp)
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
    case AGPL_KERNEL_ADDITIVE_SE: break; // (kernel_dterm below)
    case AGPL_KERNEL_ADDITIVE2_SE: break;
    case AGPL_KERNEL_MATERN32_PRODUCT: break; // (kernel_dpterm below)
    case AGPL_KERNEL_MATERN52_PRODUCT: break;
    case AGPL_KERNEL_SE_MATERN32: break; // (kernel_se_matern_dpterm below)
    case AGPL_KERNEL_SE_MATERN52: break;
    case AGPL_KERNEL_ANOVA_SE: break; // (kernel_anova_dfactor below)
    case AGPL_KERNEL_SE_CATEGORICAL: return -kernel_exp((T)-0.5 * (T)r2);
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
    // (AGPL_KERNEL_PERIODIC, AGPL_KERNEL_SE_PERIODIC, AGPL_KERNEL_SE_COSINE, AGPL_KERNEL_SE_CATEGORICAL: the squared exponential's rule, the default)
    default: return kernel_drule<AGPL_KERNEL_SE, T>(r2, param);
    }
}

// Which kinds are a SUM over the dimensions and no function of r^2, stated ONCE: AGPL_KERNEL_ADDITIVE_SE, k = variance w sum_{d < D} e_d
// with the weight w = 1 / D (kernel_term_weight) and the term e_d = exp(-u_d^2 / 2) of u_d = (x_d - x'_d) / ell_d alone (kernel_term).
// Every consumer keys off this predicate and takes the term, its derivative and the weight from here; kernel_rule and kernel_drule
// give such a kind 0 (no live code calls them with one).  A derivative of k in x_d, z_d or log ell_d holds dimension d's term
// only: d k / d u_d = variance w kernel_dterm(u_d), d k / d log ell_d = -variance w u_d kernel_dterm(u_d) = variance w u_d^2 e_d.
__host__ __device__ constexpr bool kernel_kind_additive(int kind) { return kind == AGPL_KERNEL_ADDITIVE_SE; }
// The SECOND-ORDER additive kind, stated ONCE: AGPL_KERNEL_ADDITIVE2_SE, param = w, the first-order share of the variance (0 < w <= 1).
// With S1 = sum_d e_d, E2 = sum_{d < d'} e_d e_d' and P = D (D - 1) / 2: k = variance (w1 S1 + w2 E2), w1 = w / D and w2 = (1 - w) / P
// (kernel_sum_weight1 / 2 below; at D = 1 there is no pair and w is ignored: w1 = 1, w2 = 0, the squared exponential).  E2 is ALWAYS
// built by the recurrence E2 <- fma(e_d, S1, E2); S1 <- S1 + e_d over d = 0 .. D - 1 (kernel_sum_step), every term non-negative; never as
// (S1^2 - sum e_d^2) / 2, which cancels when one dimension dominates.  d k / d u_d = variance kernel_dterm(u_d) c_d with
// c_d = w1 + w2 (S1 - e_d), and d k / d log ell_d = -u_d d k / d u_d.  A predicate of its own: kernel_kind_additive and
// kernel_term_weight stay the first-order kind's; consumers that only need "a sum over the dimensions" test kernel_kind_sum.
__host__ __device__ constexpr bool kernel_kind_additive2(int kind) { return kind == AGPL_KERNEL_ADDITIVE2_SE; }
__host__ __device__ constexpr bool kernel_kind_sum(int kind) { return kernel_kind_additive(kind) || kernel_kind_additive2(kind); }

// Which kinds are a PRODUCT over the dimensions (the separable, tensor-product Matern kinds), stated ONCE: AGPL_KERNEL_MATERN32_PRODUCT and
// AGPL_KERNEL_MATERN52_PRODUCT, no parameter.  With u_d = (x_d - x'_d) / ell_d, a_d = c |u_d| (c = kernel_product_scale: sqrt 3, sqrt 5)
// and the polynomial p (kernel_pterm: 1 + a, 1 + a + a^2 / 3), k = variance (prod_d p(a_d)) exp(-sum_d a_d): ONE exponential of the sum
// and a running product, both over d = 0 .. D - 1 in that order, and no square root.  |u_d| is even to the bit, so K_ZZ stays
// bit-symmetric.  Derivatives never divide by p(a_d); they take the product EXCLUDING d.  With t(a) = kappa'(|u|) / |u| e^a
// (kernel_dpterm: -3, -(5 / 3) (1 + a), the polynomial part of kernel_drule's closed forms for the isotropic kinds),
//     d k / d u_d = variance u_d t(a_d) (prod_{d' != d} p(a_d')) exp(-sum a),        d k / d log ell_d = -u_d d k / d u_d,
// continuous at u_d = 0 with no special case.  -(d^2 k / d tau_d^2)(0) ell_d^2 / variance = -t(0) (kernel_product_curvature: 3, 5 / 3,
// the isotropic kinds' c0, every other factor being 1 at the origin): the prior variance of d f / d x_d is variance c0 / ell_d^2 and c0
// the normalisation c of the derivative feature (agpl_grad.hip, agpl_se_build.h).  The kinds are no sum, warp nothing and carry no
// factor: kernel_kind_sum, kernel_kind_warps and kernel_kind_modulated are false for them, and kernel_rule / kernel_drule give them 0
// (no live code calls them with one).  At D = 1 they are the isotropic kinds.
__host__ __device__ constexpr bool kernel_kind_product(int kind) {
    return kind == AGPL_KERNEL_MATERN32_PRODUCT || kind == AGPL_KERNEL_MATERN52_PRODUCT;
}
__host__ __device__ constexpr double kernel_product_scale(int kind) {
    return kind == AGPL_KERNEL_MATERN32_PRODUCT ? 1.7320508075688772 : 2.23606797749979;
}
// p(a), Horner with fused multiply-adds: 1 + a (1 + a / 3) for 5/2.  T = float for the generator, double for K_ZZ and its kin.
template <int KIND, typename T>
__host__ __device__ __forceinline__ T kernel_pterm(T a) {
    static_assert(kernel_kind_product(KIND), "a product kind");
    if constexpr (KIND == AGPL_KERNEL_MATERN32_PRODUCT) return (T)1 + a;
    else if constexpr (sizeof(T) == sizeof(float)) return fmaf(fmaf(a, (T)(1.0 / 3.0), (T)1), a, (T)1);
    else return fma(fma(a, (T)(1.0 / 3.0), (T)1), a, (T)1);
}
// t(a) = kappa'(|u|) / |u| e^a
template <int KIND, typename T>
__host__ __device__ __forceinline__ T kernel_dpterm(T a) {
    static_assert(kernel_kind_product(KIND), "a product kind");
    if constexpr (KIND == AGPL_KERNEL_MATERN32_PRODUCT) return (T)-3;
    else return (T)(-5.0 / 3.0) * ((T)1 + a);
}
// the two of a run-time kind in float64 (K_ZZ, the greedy selector, the K_ZZ part of the gradients: one uniform branch)
__host__ __device__ inline double kernel_pterm_value(int kind, double a) {
    return kind == AGPL_KERNEL_MATERN32_PRODUCT ? kernel_pterm<AGPL_KERNEL_MATERN32_PRODUCT, double>(a)
                                                : kernel_pterm<AGPL_KERNEL_MATERN52_PRODUCT, double>(a);
}
__host__ __device__ inline double kernel_dpterm_value(int kind, double a) {
    return kind == AGPL_KERNEL_MATERN32_PRODUCT ? kernel_dpterm<AGPL_KERNEL_MATERN32_PRODUCT, double>(a)
                                                : kernel_dpterm<AGPL_KERNEL_MATERN52_PRODUCT, double>(a);
}
// c0 = -t(0)
__host__ __device__ inline double kernel_product_curvature(int kind) { return -kernel_dpterm_value(kind, 0.0); }
// P exp(-s) from the two accumulators s = sum_d a_d and P = prod_d p(a_d) (a derivative: u_d t(a_d) in place of p(a_d) for its own
// dimension).  Every factor is at most e^{a_d} in magnitude (p(a) <= e^a; |u t(a)| <= e^a for both orders), so |P| <= e^s and P is
// finite while s is below the cut (87 in float32, 700 in float64: e^s and e^-s are both normal numbers there).  Past the cut P may
// have overflowed and inf 0 would be NaN: the value is 0 there.  What that drops is at most D = 16 factors kappa(s / 16) each, below
// 1e-16 of the variance already at s = 87.
template <typename T>
__host__ __device__ __forceinline__ T kernel_product_value(T s, T P) {
    return s < (T)(sizeof(T) == sizeof(float) ? 87.0 : 700.0) ? P * kernel_exp(-s) : (T)0;
}

// Which kinds are the squared exponential in the leading dimensions times a one-dimensional Matern in the LAST one, stated ONCE:
// AGPL_KERNEL_SE_MATERN32 and AGPL_KERNEL_SE_MATERN52, no parameter (x = (covariates or space ..., t): smooth in the covariates, finite
// smoothness in time).  With u_d = (x_d - x'_d) / ell_d, r_lead^2 = sum_{d < D - 1} u_d^2, a = c |u_{D-1}| and c, p, t the product
// kinds' of the same order (kernel_se_matern_order maps 70 -> 64 and 72 -> 66: kernel_product_scale, kernel_pterm, kernel_dpterm are
// not restated),
//     k = variance p(a) exp(-(r_lead^2 / 2 + a)):
// ONE exponential of s = r_lead^2 / 2 + a, no square root.  u^2 and |u| are even to the bit, so K_ZZ stays bit-symmetric.  With
// E = variance exp(-s): d k / d u_d = -u_d k in a leading dimension and u t(a) E in the last (never a division by p);
// d k / d log ell_d = -u_d d k / d u_d in both.  -(d^2 k / d tau_d^2)(0) ell_d^2 / variance (kernel_se_matern_curvature) is 1 in a
// leading dimension and c0 = -t(0) = 3 or 5 / 3 in the last: the prior variance of d f / d x_d is variance times it over ell_d^2.
// The value is kernel_product_value(s, p(a)): 0 past that rule's cut (p(a) <= e^a <= e^s, |u t(a)| <= e^a, |u_d| p(a) <= e^s likewise).
// The kinds are no sum, no product over all dimensions, warp nothing and carry no factor in the modulated kinds' sense: every older
// predicate is false for them, and kernel_rule / kernel_drule give them 0 (no live code calls them with one).  At D = 1 they are the
// isotropic Matern kinds.
__host__ __device__ constexpr bool kernel_kind_se_matern(int kind) { return kind == AGPL_KERNEL_SE_MATERN32 || kind == AGPL_KERNEL_SE_MATERN52; }
__host__ __device__ constexpr int kernel_se_matern_order(int kind) {
    return kind == AGPL_KERNEL_SE_MATERN32 ? AGPL_KERNEL_MATERN32_PRODUCT : AGPL_KERNEL_MATERN52_PRODUCT;
}
__host__ __device__ constexpr double kernel_se_matern_scale(int kind) { return kernel_product_scale(kernel_se_matern_order(kind)); }
template <int KIND, typename T>
__host__ __device__ __forceinline__ T kernel_se_matern_pterm(T a) {
    static_assert(kernel_kind_se_matern(KIND), "a squared exponential x Matern kind");
    return kernel_pterm<kernel_se_matern_order(KIND), T>(a);
}
template <int KIND, typename T>
__host__ __device__ __forceinline__ T kernel_se_matern_dpterm(T a) {
    static_assert(kernel_kind_se_matern(KIND), "a squared exponential x Matern kind");
    return kernel_dpterm<kernel_se_matern_order(KIND), T>(a);
}
// the two of a run-time kind in float64, beside kernel_pterm_value
__host__ __device__ inline double kernel_se_matern_pterm_value(int kind, double a) { return kernel_pterm_value(kernel_se_matern_order(kind), a); }
__host__ __device__ inline double kernel_se_matern_dpterm_value(int kind, double a) { return kernel_dpterm_value(kernel_se_matern_order(kind), a); }
// s = r_lead^2 / 2 + a and P = p(a) from r_lead^2 and the LAST dimension's scaled difference, in float64 (K_ZZ, the greedy selector, K
// between new inputs: the caller's loop over d holds r_lead^2 when it reaches d = D - 1); k = variance kernel_product_value(s, P)
__host__ __device__ inline void kernel_se_matern_last(int kind, double r2_lead, double us, double &s, double &P) {
    const double a = kernel_se_matern_scale(kind) * fabs(us);
    s = 0.5 * r2_lead + a;
    P = kernel_se_matern_pterm_value(kind, a);
}
// 1 in a leading dimension, c0 = -t(0) in the last
__host__ __device__ inline double kernel_se_matern_curvature(int kind, int d, int D) {
    return d == D - 1 ? kernel_product_curvature(kernel_se_matern_order(kind)) : 1.0;
}

// The all-orders additive (ANOVA) squared exponential kind, stated ONCE: AGPL_KERNEL_ANOVA_SE, param = eta (0 < eta <= 1), a PRODUCT over
// the dimensions of (constant + one-dimensional squared exponential).  With u_d = (x_d - x'_d) / ell_d and e_d = exp(-u_d^2 / 2),
//     k = variance prod_{d < D} g_d,        g_d = 1 - eta (1 - e_d)        (kernel_anova_factor),
// the product running over d = 0 .. D - 1 in that order everywhere.  Expanded it is the sum of all 2^D interaction terms, a set of n
// dimensions carrying eta^n (1 - eta)^(D - n) of the variance: the first-order additive kind towards eta = 0, mathematically (not bit
// for bit) the squared exponential at eta = 1.  Far from all data k tends to variance (1 - eta)^D, the share of the shared level, not 0.
// g is ALWAYS formed as fma(-eta, 1 - e, 1): exactly 1 at u = 0, so k(x, x) = variance to the bit; u enters squared, so g is even in u
// to the bit and K_ZZ stays bit-symmetric; g lies in [1 - eta, 1], so the running product never overflows and needs no cut.
// Derivatives NEVER divide by g_d (at eta = 1 it underflows): they take the product EXCLUDING d, as the product Matern kinds do,
//     d k / d u_d = variance (d g_d / d u_d) prod_{d' != d} g_d',    d g / d u = eta (-u e) (kernel_anova_dfactor),    d k / d log ell_d = -u_d d k / d u_d.
// -(d^2 k / d tau_d^2)(0) ell_d^2 / variance = eta (kernel_anova_curvature; every other factor is 1 at the origin): the prior variance of
// d f / d x_d is variance eta / ell_d^2 and eta the normalisation c of that dimension's derivative feature (agpl_grad.hip,
// agpl_se_build.h).  T = float for the generator (u is rounded ONCE from the float64 difference: no float64 arithmetic after it),
// double for K_ZZ and its kin.  The kind is no sum, no product kind in kernel_kind_product's sense (no p, t or exponential of a sum),
// warps nothing and carries no factor: every older predicate is false for it, and kernel_rule / kernel_drule give it 0.
__host__ __device__ constexpr bool kernel_kind_anova(int kind) { return kind == AGPL_KERNEL_ANOVA_SE; }
template <typename T>
__host__ __device__ __forceinline__ T kernel_anova_term(double u) { // e
    const T v = (T)u;
    return kernel_exp((T)-0.5 * (v * v));
}
template <typename T>
__host__ __device__ __forceinline__ T kernel_anova_factor(T eta, double u) { // g
    if constexpr (sizeof(T) == sizeof(float)) return fmaf(-eta, (T)1 - kernel_anova_term<T>(u), (T)1);
    else return fma(-eta, (T)1 - kernel_anova_term<T>(u), (T)1);
}
template <typename T>
__host__ __device__ __forceinline__ T kernel_anova_dfactor(T eta, double u) { // d g / d u
    return eta * (-(T)u * kernel_anova_term<T>(u));
}
// eta for the kind, 1 for every other (a factor of the derivative feature's c beside kernel_sum_curvature)
__host__ __device__ inline double kernel_anova_curvature(int kind, double param) { return kernel_kind_anova(kind) ? param : 1.0; }

// The squared exponential x categorical kind, stated ONCE: AGPL_KERNEL_SE_CATEGORICAL, param = C (an integer, 1 <= C <= 16, C <= D where
// D is known: kernel_categorical_exceeds), the number of TRAILING inputs that are category codes; the first D - C are continuous.  Which
// dimensions are categorical depends on the run-time param, so the predicate takes it (kernel_dim_warped cannot, and stays false):
//     k = variance exp(-(sum_{d < D - C} u_d^2 + sum_{d >= D - C} [x_d != x'_d] / ell_d^2) / 2),       u_d = (x_d - x'_d) / ell_d,
// the squared exponential's rule (kernel_rule / kernel_drule, as for the periodic kinds) on a warped distance whose categorical terms
// are u_d = [us != 0] / ell_d (kernel_categorical_warp) with d u_d / d us = 0: a code has no distance, only equality.  It equals the
// squared exponential on the one-hot encoding of that input with lengthscale sqrt(2) ell_d; two points that differ in input d are
// correlated rho_d = exp(-1 / (2 ell_d^2)) through it.  Callers hold x / ell_d and z / ell_d: equal codes give us = 0 exactly (the
// same division of the same number), distinct integer codes never do, so the test is us != 0.0 on the scaled difference already
// formed, and the selected constant is 1 / ell_d for r^2 (float64 consumers) or h_d = 1 / (2 ell_d^2) straight into the exponent's
// argument (the generator: kernel_categorical_half, formed once per workgroup).  The comparison is symmetric, so K_ZZ is symmetric to
// the bit, and k(x, x) = variance.  d k / d log ell_d = u_d^2 k in EVERY dimension (u_d^2 = [!=] / ell_d^2 in a categorical one: the
// existing formula on the warped u); d k / d x_d, d k / d z_d are exactly 0 in a categorical one.  The kind is no sum, no product,
// warps nothing in kernel_dim_warped's sense and carries no factor: every older predicate is false for it.
__host__ __device__ constexpr bool kernel_kind_categorical(int kind) { return kind == AGPL_KERNEL_SE_CATEGORICAL; }
__host__ __device__ constexpr bool kernel_dim_categorical(int kind, int d, int D, double param) {
    return kernel_kind_categorical(kind) && d >= D - (int)param;
}
// u_d of a categorical dimension from the scaled difference and 1 / ell_d: a compare and a select, no arithmetic on the codes
__host__ __device__ __forceinline__ double kernel_categorical_warp(double us, double inv_ell) { return us != 0.0 ? inv_ell : 0.0; }
// h_d = u_d^2 / 2 of two different codes, the constant the generator selects into the exponent's argument
__host__ __device__ __forceinline__ double kernel_categorical_half(double ell) { return 0.5 / (ell * ell); }
// C > D (host; the one check that needs D, beside kernel_param_refused)
inline bool kernel_categorical_exceeds(int kind, double param, int D) { return kernel_kind_categorical(kind) && param > (double)D; }

__host__ __device__ inline bool kernel_kind_known(int kind) {
    return (kind >= AGPL_KERNEL_SE && kind <= AGPL_KERNEL_RQ) || kind == AGPL_KERNEL_PERIODIC || kind == AGPL_KERNEL_SE_PERIODIC ||
           kind == AGPL_KERNEL_SE_COSINE || kernel_kind_additive(kind) || kernel_kind_additive2(kind) || kernel_kind_product(kind) ||
           kernel_kind_se_matern(kind) || kernel_kind_anova(kind) || kernel_kind_categorical(kind);
}

// e_d and d e_d / d u_d = -u_d e_d from the float64 difference; T = the arithmetic type of the exponential, as for kernel_rule.
// e_d is the squared exponential's rule on r^2 = u_d^2, the same expression: at D = 1 the kind is that kind to the bit.  Even in u_d
// to the bit (u_d enters squared), so K_ZZ stays bit-symmetric.
template <typename T>
__host__ __device__ __forceinline__ T kernel_term(double u) {
    return kernel_exp((T)-0.5 * (T)(u * u));
}
template <typename T>
__host__ __device__ __forceinline__ T kernel_dterm(double u) {
    return -(T)u * kernel_term<T>(u);
}
// each term's share of the variance: 1 / D for an additive kind (k(x, x) = variance), 1 for every other.  It also scales the prior
// variance of d f / d x_d, variance w / ell_d^2, and so the normalisation c of that dimension's derivative feature (agpl_grad.hip).
__host__ __device__ inline double kernel_term_weight(int kind, int D) { return kernel_kind_additive(kind) ? 1.0 / (double)D : 1.0; }
// The two mixing weights of a sum kind (kernel_kind_sum), k = variance (w1 S1 + w2 E2): the first-order kind's are 1 / D and 0 (its
// kernel_term_weight), the second-order kind's w / D and (1 - w) / P with w = param where there is a pair (D >= 2) and 1 where there
// is none.  At w = 1 the two kinds' weights are the same doubles.
__host__ __device__ inline double kernel_sum_share(int kind, int D, double param) { return kernel_kind_additive2(kind) && D >= 2 ? param : 1.0; }
__host__ __device__ inline double kernel_sum_weight1(int kind, int D, double param) { return kernel_sum_share(kind, D, param) / (double)D; }
__host__ __device__ inline double kernel_sum_weight2(int kind, int D, double param) {
    return D >= 2 ? (1.0 - kernel_sum_share(kind, D, param)) / (0.5 * (double)D * (double)(D - 1)) : 0.0;
}
// -(d^2 k / d tau_d^2)(0) ell_d^2 / variance of a sum kind: c_d at u = 0, w1 + w2 (D - 1) = (2 - w) / D (1 / D at w = 1 and for the
// first-order kind, 1 at D = 1).  The prior variance of d f / d x_d is variance times this over ell_d^2, and this is the normalisation
// c of that dimension's derivative feature (agpl_grad.hip, agpl_se_build.h); 1 for every other kind.
__host__ __device__ inline double kernel_sum_curvature(int kind, int D, double param) {
    return kernel_kind_sum(kind) ? (2.0 - kernel_sum_share(kind, D, param)) / (double)D : 1.0;
}
// one step of the elementary-symmetric recurrence, dimensions ascending: T = float for the generator, double for K_ZZ and its kin
template <typename T>
__host__ __device__ __forceinline__ void kernel_sum_step(T e, T &S1, T &E2) {
    if constexpr (sizeof(T) == sizeof(float)) E2 = fmaf(e, S1, E2);
    else E2 = fma(e, S1, E2);
    S1 += e;
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
// or per pivot, so the two divisions are not hoisted), for dimension d of D.  A categorical dimension (kernel_dim_categorical) has its
// own rule, [us != 0] / ell_d, and the derivative exactly 0: K_ZZ and the K_ZZ parts of both gradients take the kind from here.
__device__ inline double kernel_warp_value(int kind, int d, int D, double us, double ell, double param) {
    if (kernel_dim_categorical(kind, d, D, param)) return kernel_categorical_warp(us, 1.0 / ell);
    return kernel_dim_warped(kind, d, D) ? kernel_warp<AGPL_KERNEL_PERIODIC>(us, ell / param, 1.0 / ell) : us;
}
__device__ inline double kernel_dwarp_value(int kind, int d, int D, double us, double ell, double param) {
    if (kernel_dim_categorical(kind, d, D, param)) return 0.0;
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
    if (kernel_kind_additive2(kind) && !(ok && param <= 1.0)) return "the first-order share w of the second-order additive kernel";
    if (kernel_kind_anova(kind) && !(ok && param <= 1.0)) return "eta of the all-orders additive (ANOVA) squared exponential kernel";
    if (kernel_kind_categorical(kind) && !(param >= 1.0 && param <= 16.0 && param == (double)(int)param))
        return "the number C of trailing categorical inputs of the squared exponential x categorical kernel";
    return nullptr;
}
// what the refusal says the parameter must be
inline const char *kernel_param_range(int kind) {
    if (kernel_kind_categorical(kind)) return "an integer in 1 ... 16 and at most D";
    return kernel_kind_additive2(kind) || kernel_kind_anova(kind) ? "positive and at most 1" : "positive and finite";
}
inline bool kernel_has_param(int kind) {
    return kind == AGPL_KERNEL_RQ || kernel_kind_warps(kind) || kernel_kind_modulated(kind) || kernel_kind_additive2(kind) ||
           kernel_kind_anova(kind) || kernel_kind_categorical(kind);
}

// kappa(r) of a run-time kind: one uniform switch (K_ZZ, once per plan; the generator dispatches on the host instead)
template <typename T>
__host__ __device__ inline T kernel_value(int kind, double r2, double param) {
    switch (kind) {
    case AGPL_KERNEL_MATERN12: return kernel_rule<AGPL_KERNEL_MATERN12, T>(r2, param);
    case AGPL_KERNEL_MATERN32: return kernel_rule<AGPL_KERNEL_MATERN32, T>(r2, param);
    case AGPL_KERNEL_MATERN52: return kernel_rule<AGPL_KERNEL_MATERN52, T>(r2, param);
    case AGPL_KERNEL_RQ: return kernel_rule<AGPL_KERNEL_RQ, T>(r2, param);
    // (AGPL_KERNEL_PERIODIC, AGPL_KERNEL_SE_PERIODIC, AGPL_KERNEL_SE_COSINE, AGPL_KERNEL_SE_CATEGORICAL: the squared exponential's rule, the default)
    default: return kernel_rule<AGPL_KERNEL_SE, T>(r2, param);
    }
}

} // namespace agpl
