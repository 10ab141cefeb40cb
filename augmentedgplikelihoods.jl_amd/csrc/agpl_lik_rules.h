// agpl_lik_rules.h -- the per-point rules of the twelve likelihoods, each stated ONCE: aux_posterior!, the expected potential /
// precision of the CAVI side, the sampled potential / precision of the Gibbs side, and the predicates on the kind.  The rules
// take accessors (k = latent of the point at hand) and hand their results to a `put`, so the same expressions serve the
// array-fed operator kernels (agpl_operators.hip), the sweep's fused per-point kernel (registers in between) and the Gibbs
// point pass (agpl_sampler.hip, LDS in between): the same expressions, hence the same results bit for bit (both files are
// compiled without fused-multiply-add contraction).  T = the arithmetic type; every accessor returns T.
// The float32 order of operations is that of the sweep's kernel: do not reassociate.
#pragma once
#include "agpl_common.h"
#include "agpl_random.h"

// ---- predicates on the kind (host + device)
// the categorical / Poisson / heteroscedastic augmentations carry latent counts n beside omega ...
__host__ __device__ inline bool lik_needs_counts(int kind) {
    return kind == AGPL_LIK_CATEGORICAL || kind == AGPL_LIK_CATEGORICAL_BIJ || kind == AGPL_LIK_POISSON ||
           kind == AGPL_LIK_HETEROGAUSS;
}
// ... and their aux_posterior! has a second output (the rate of those counts: out2 / q2)
__host__ __device__ inline bool lik_needs_second(int kind) { return lik_needs_counts(kind); }
// aux_posterior! reads y (the PG kinds' c = sqrt(E f^2) does not; the per-point binomial's c does not either, but its
// theta = E PG(n_i, c) reads the point's trials: a caller that forms both from one load of y must load it)
__host__ __device__ inline bool lik_needs_y(int kind) {
    return kind == AGPL_LIK_STUDENTT || kind == AGPL_LIK_LAPLACE || kind == AGPL_LIK_HETEROGAUSS || kind == AGPL_LIK_ASYMLAPLACE ||
           kind == AGPL_LIK_LOGISTIC_NOISE || kind == AGPL_LIK_BINOMIAL_N;
}
// (lik_is_categorical: agpl_lik_desc.h, beside the list of the kinds)

namespace agpl {

// The one run-time switch over the kind: body(l) with l = lik and l.kind a compile-time constant, so that the switches of the
// rules below fold and a kernel whose kind is a run-time value branches ONCE per point, around everything it does for the point.
// (Where the kind already is a constant this switch folds too.)
template <class BODY>
__device__ __forceinline__ void lik_dispatch(const agpl_lik_dev &lik, BODY body) {
    agpl_lik_dev l = lik;
    switch (lik.kind) {
#define AGPL_LIK_CASE_(K) \
    case K: \
        l.kind = K; \
        body(l); \
        break;
        AGPL_LIK_KINDS(AGPL_LIK_CASE_) // the one list (agpl_lik_desc.h)
#undef AGPL_LIK_CASE_
    default:
        break;
    }
}

// The asymmetric Laplace kind (agpl.h) is the Laplace kind at beta = 2 sigma, tilted by exp(kappa (y - f)): its auxiliary
// variable never reads tau, its potential is shifted by -kappa and its tilts gain kappa (y - f) + log(4 tau (1 - tau)).
template <typename T>
__host__ __device__ __forceinline__ T ald_beta(const agpl_lik_dev &lik) { return T(2) * (T)lik.p[0]; }
template <typename T>
__host__ __device__ __forceinline__ T ald_kappa(const agpl_lik_dev &lik) { return (T)((1.0 - 2.0 * lik.p[1]) / (2.0 * lik.p[0])); }
__host__ __device__ __forceinline__ double ald_logconst(const agpl_lik_dev &lik) { return log(4.0 * lik.p[1] * (1.0 - lik.p[1])); }

// the binomial kinds' trials at the point at hand: p[0] for kind 8, column 1 of the observation (NaN outside its domain) for kind 11
template <typename T, class Y>
__device__ __forceinline__ T binomial_n(const agpl_lik_dev &lik, Y y) {
    return lik.kind == AGPL_LIK_BINOMIAL ? (T)lik.p[0] : binomial_trials<T>(y(1));
}

template <typename T>
__device__ __forceinline__ T second_moment(T mu, T var) { return mu * mu + var; } // utils.jl:1-3
template <typename T>
__device__ __forceinline__ T second_moment_y(T mu, T var, T y) { return (mu - y) * (mu - y) + var; } // :5-7

// y of (point i, latent k) as a T, by the likelihood's observation type (REAL: the element type of real-valued y)
template <typename REAL, typename T = double>
struct YAcc {
    const void *y;
    int64_t i;
    int kind, L;
    __device__ __forceinline__ T operator()(int k) const {
        switch (kind) {
        case AGPL_LIK_BERNOULLI_LOGISTIC:
            return (T)((const uint8_t *)y)[i];
        case AGPL_LIK_NEGBINOMIAL:
        case AGPL_LIK_POISSON:
        case AGPL_LIK_BINOMIAL:
            return (T)((const int32_t *)y)[i];
        case AGPL_LIK_CATEGORICAL:
        case AGPL_LIK_CATEGORICAL_BIJ:
            return (T)((const uint8_t *)y)[i * L + k];
        case AGPL_LIK_BINOMIAL_N: // int32 [N][2]: k = 0 successes, k = 1 trials
            return (T)((const int32_t *)y)[2 * i + k];
        default:
            return (T)((const REAL *)y)[i];
        }
    }
};

// aux_posterior! (bernoulli.jl:17-25, negativebinomial.jl:24-33, studentt.jl:50-58, categorical.jl:80-110, poisson.jl:30-39,
// laplace.jl:44-52, heteroscedasticgaussian.jl:34-46) for auxiliary variable k of one point: o1 always; o2 where
// lik_needs_second; o3 (psi) for the heteroscedastic kind, whose one auxiliary variable reads both latents.
template <typename T, class Y, class MU, class VAR>
__device__ __forceinline__ void lik_aux_posterior_at(const agpl_lik_dev &lik, int k, Y y, MU mu, VAR var, T &o1, T &o2, T &o3) {
    o2 = o3 = T(0);
    switch (lik.kind) {
    case AGPL_LIK_BERNOULLI_LOGISTIC:
    case AGPL_LIK_NEGBINOMIAL:
    case AGPL_LIK_BINOMIAL: // (no file in the reference: agpl.h) q(omega) = PG(n, c)
    case AGPL_LIK_BINOMIAL_N:
        o1 = sqrt(second_moment<T>(mu(0), var(0)));
        break;
    case AGPL_LIK_STUDENTT: {
        const T nu = (T)lik.p[0], sg = (T)lik.p[1];
        o1 = (nu / (sg * sg) + second_moment_y<T>(mu(0), var(0), y(0))) / T(2);
    } break;
    case AGPL_LIK_CATEGORICAL:
    case AGPL_LIK_CATEGORICAL_BIJ: {
        const T den = lik.kind == AGPL_LIK_CATEGORICAL ? (T)lik.nlatent : (T)(lik.cat_const + (double)lik.nlatent);
        const T m = mu(k);
        o1 = sqrt(second_moment<T>(m, var(k)));
        o2 = approx_expected_logistic(-m, o1) / den;
    } break;
    case AGPL_LIK_POISSON: {
        const T m = mu(0);
        o1 = sqrt(second_moment<T>(m, var(0)));
        o2 = (T)lik.p[0] * approx_expected_logistic(-m, o1);
    } break;
    case AGPL_LIK_LAPLACE:
        o1 = T(1) / (T(2) * (T)lik.p[0] * sqrt(second_moment_y<T>(mu(0), var(0), y(0))));
        break;
    case AGPL_LIK_ASYMLAPLACE: // Laplace's at beta = 2 sigma: tau is not read
        o1 = T(1) / (T(2) * ald_beta<T>(lik) * sqrt(second_moment_y<T>(mu(0), var(0), y(0))));
        break;
    case AGPL_LIK_LOGISTIC_NOISE: // (agpl.h) q(omega) = PG(2, c), c = sqrt(E (y - f)^2) / s
        o1 = sqrt(second_moment_y<T>(mu(0), var(0), y(0))) / (T)lik.p[0];
        break;
    case AGPL_LIK_HETEROGAUSS: {
        o3 = second_moment_y<T>(mu(0), var(0), y(0)) / T(2);
        const T m = mu(1);
        o1 = sqrt(second_moment<T>(m, var(1)));
        o2 = (T)lik.p[0] * approx_expected_logistic(-m, o1) * o3;
    } break;
    default:
        o1 = T(0);
        break;
    }
}
// the whole point: put(k, out1, out2, out3) per auxiliary variable
template <typename T, class Y, class MU, class VAR, class PUT>
__device__ __forceinline__ void lik_aux_posterior(const agpl_lik_dev &lik, Y y, MU mu, VAR var, PUT put) {
    const int na = lik_is_categorical(lik.kind) ? lik.nlatent : 1;
    for (int k = 0; k < na; ++k) {
        T o1, o2, o3;
        lik_aux_posterior_at<T>(lik, k, y, mu, var, o1, o2, o3);
        put(k, o1, o2, o3);
    }
}

// expected_auglik_potential / expected_auglik_precision of one point: put(k, gamma, beta, q1) per latent, q1 = the out1 that
// latent's gamma was formed from (for a caller that forms the auxiliary posterior on the fly and wants to keep it).  aux(k) =
// (out1, out2) of aux_posterior! for auxiliary variable k, in one call: such a caller forms both at once; mu_g = the mean of the
// heteroscedastic kind's second latent.
template <typename T>
struct LikAux {
    T q1, q2;
};
template <typename T, class Y, class AUX, class MUG, class PUT>
__device__ __forceinline__ void lik_expected_pp(const agpl_lik_dev &lik, Y y, AUX aux, MUG mu_g, PUT put) {
    switch (lik.kind) {
    case AGPL_LIK_BERNOULLI_LOGISTIC: { // bernoulli.jl:27-29,41-45
        const T c = aux(0).q1;
        put(0, pg_mean(T(1), c), y(0) != T(0) ? T(0.5) : T(-0.5), c);
    } break;
    case AGPL_LIK_NEGBINOMIAL: { // negativebinomial.jl:35-37,47-49
        const T r = (T)lik.p[0], c = aux(0).q1;
        put(0, pg_mean(y(0) + r, c), (y(0) - r) / T(2), c);
    } break;
    case AGPL_LIK_BINOMIAL:
    case AGPL_LIK_BINOMIAL_N: { // (agpl.h) theta = E PG(n, c), beta = y - n / 2; n = p[0] or the point's own
        const T nt = binomial_n<T>(lik, y), c = aux(0).q1;
        put(0, pg_mean(nt, c), y(0) - nt / T(2), c);
    } break;
    case AGPL_LIK_STUDENTT: { // studentt.jl:41-43,68-74
        const T b = aux(0).q1;
        const T w = (((T)lik.p[0] + T(1)) / T(2)) * (T(1) / b);
        put(0, w, w * y(0), b);
    } break;
    case AGPL_LIK_CATEGORICAL:
    case AGPL_LIK_CATEGORICAL_BIJ: { // categorical.jl:121-136, polyagammanegativemultinomial.jl:41-49
        const int L = lik.nlatent;
        T sp = T(0);
        for (int k = 0; k < L; ++k) sp += aux(k).q2;
        const T p0 = T(1) - sp;
        for (int k = 0; k < L; ++k) {
            const LikAux<T> a = aux(k);
            const T nbar = T(1) / p0 * a.q2;
            const T yk = y(k);
            put(k, pg_mean(yk + nbar, a.q1), (yk - nbar) / T(2), a.q1);
        }
    } break;
    case AGPL_LIK_POISSON: { // poisson.jl:49-60, polyagammapoisson.jl:35-41
        const LikAux<T> a = aux(0);
        put(0, pg_mean(y(0) + a.q2, a.q1), (y(0) - a.q2) / T(2), a.q1);
    } break;
    case AGPL_LIK_LAPLACE: { // laplace.jl:62-68
        const T m = aux(0).q1;
        put(0, T(2) * m, T(2) * m * y(0), m);
    } break;
    case AGPL_LIK_ASYMLAPLACE: { // Laplace's, the potential shifted by the tilt's -kappa
        const T m = aux(0).q1;
        put(0, T(2) * m, T(2) * m * y(0) - ald_kappa<T>(lik), m);
    } break;
    case AGPL_LIK_LOGISTIC_NOISE: { // (agpl.h) theta = E PG(2, c); gamma = theta / s^2, beta = theta y / s^2
        const T s = (T)lik.p[0], c = aux(0).q1;
        const T w = pg_mean(T(2), c) / (s * s);
        put(0, w, w * y(0), c);
    } break;
    case AGPL_LIK_HETEROGAUSS: { // heteroscedasticgaussian.jl:94-104
        const LikAux<T> a = aux(0);
        const T lsg = (T)lik.p[0] * (T(1) - approx_expected_logistic(-mu_g(0), a.q1));
        put(0, lsg, y(0) * lsg / T(2), a.q1);
        put(1, pg_mean(T(0.5) + a.q2, a.q1), (T(0.5) - a.q2) / T(2), a.q1);
    } break;
    default:
        break;
    }
}

// auglik_potential / auglik_precision (the sampled twins), float64: put(k, gamma, beta) per latent.  omega(k), nn(k) = the
// draw's auxiliary variables (nn as a double), f(k) = the latent values (read by the heteroscedastic kind only).
template <class Y, class OM, class NN, class F, class PUT>
__device__ __forceinline__ void lik_sampled_pp(const agpl_lik_dev &lik, Y y, OM omega, NN nn, F f, PUT put) {
    switch (lik.kind) {
    case AGPL_LIK_BERNOULLI_LOGISTIC: // bernoulli.jl:27-33
        put(0, omega(0), y(0) != 0.0 ? 0.5 : -0.5);
        break;
    case AGPL_LIK_NEGBINOMIAL:
        put(0, omega(0), (y(0) - lik.p[0]) / 2.0);
        break;
    case AGPL_LIK_BINOMIAL:
    case AGPL_LIK_BINOMIAL_N:
        put(0, omega(0), y(0) - binomial_n<double>(lik, y) / 2.0);
        break;
    case AGPL_LIK_STUDENTT:
        put(0, omega(0), y(0) * omega(0));
        break;
    case AGPL_LIK_CATEGORICAL:
    case AGPL_LIK_CATEGORICAL_BIJ:
        for (int k = 0; k < lik.nlatent; ++k) put(k, omega(k), (y(k) - nn(k)) / 2.0);
        break;
    case AGPL_LIK_POISSON:
        put(0, omega(0), (y(0) - nn(0)) / 2.0);
        break;
    case AGPL_LIK_LAPLACE:
        put(0, 2.0 * omega(0), 2.0 * omega(0) * y(0));
        break;
    case AGPL_LIK_ASYMLAPLACE:
        put(0, 2.0 * omega(0), 2.0 * omega(0) * y(0) - ald_kappa<double>(lik));
        break;
    case AGPL_LIK_LOGISTIC_NOISE: {
        const double w = omega(0) / (lik.p[0] * lik.p[0]);
        put(0, w, w * y(0));
    } break;
    case AGPL_LIK_HETEROGAUSS: {
        const double il = lik.p[0] * logistic(f(1));
        put(0, il, y(0) * il);
        put(1, omega(0), (0.5 - nn(0)) / 2.0);
    } break;
    default:
        break;
    }
}

} // namespace agpl
