// agpl_lik_desc.h -- what every layer has to know about a likelihood kind before it looks at a point, each stated ONCE: the list of
// the kinds, the predicates and small facts derived from it, the check of a descriptor (agpl_lik_to_device of libagpl.so and the
// entry points of the extension libraries that read the descriptor themselves all call it) and the host switch that turns the
// run-time kind into a compile-time one.  No HIP dependency: tests/test_lik_desc_cpu.py compiles this header with g++ and compares
// code and message over a grid of descriptors.  DESIGN.md 4.34 has the list of what a new kind still has to state per kind.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>

#include <type_traits>

#include "../../include/agpl.h"

// ---- the kinds, in enumerator order: the device switch (agpl::lik_dispatch, agpl_lik_rules.h) and the host switch (agpl::lik_switch,
// below) expand this list, and so does agpl_lik_kind_known
#define AGPL_LIK_KINDS(X)          \
    X(AGPL_LIK_BERNOULLI_LOGISTIC) \
    X(AGPL_LIK_NEGBINOMIAL)        \
    X(AGPL_LIK_STUDENTT)           \
    X(AGPL_LIK_CATEGORICAL)        \
    X(AGPL_LIK_CATEGORICAL_BIJ)    \
    X(AGPL_LIK_POISSON)            \
    X(AGPL_LIK_LAPLACE)            \
    X(AGPL_LIK_HETEROGAUSS)        \
    X(AGPL_LIK_BINOMIAL)           \
    X(AGPL_LIK_ASYMLAPLACE)        \
    X(AGPL_LIK_LOGISTIC_NOISE)     \
    X(AGPL_LIK_BINOMIAL_N)

constexpr bool agpl_lik_kind_known(int kind) {
#define AGPL_LIK_OR_(K) || kind == K
    return false AGPL_LIK_KINDS(AGPL_LIK_OR_);
#undef AGPL_LIK_OR_
}

// ---- small facts of a kind (constexpr: host, device and `if constexpr` alike)
constexpr bool lik_is_categorical(int kind) { return kind == AGPL_LIK_CATEGORICAL || kind == AGPL_LIK_CATEGORICAL_BIJ; }
// the nlatent a kind other than the categorical ones requires (those take 1 .. 64)
constexpr int agpl_lik_nlatent(int kind) { return kind == AGPL_LIK_HETEROGAUSS ? 2 : 1; }
// learnable parameters of a kind other than the categorical ones: p[0 .. this) (include/agpl_likgrad.h)
constexpr int agpl_lik_nparams(int kind) {
    return (kind == AGPL_LIK_BERNOULLI_LOGISTIC || kind == AGPL_LIK_BINOMIAL || kind == AGPL_LIK_BINOMIAL_N) ? 0 : (kind == AGPL_LIK_STUDENTT ? 2 : 1);
}

// ---- the parameter rules of the two kinds whose rule is more than a sign (agpl.h; a NaN fails each comparison)
static inline bool agpl_asymlaplace_ok(double sigma, double tau) {
    return sigma > 0.0 && sigma <= 1.7976931348623157e308 && tau > 0.0 && tau < 1.0;
}
#define AGPL_ASYMLAPLACE_MSG "AsymmetricLaplace needs a finite sigma > 0 and 0 < tau < 1 (sigma = %g, tau = %g)"
static inline bool agpl_logistic_noise_ok(double scale) { return scale > 0.0 && scale <= 1.7976931348623157e308; }
#define AGPL_LOGISTIC_NOISE_MSG "LogisticNoise needs a finite scale > 0 (scale = %g)"

// ---- the descriptor check: AGPL_OK, or AGPL_ERR_INVALID_ARGUMENT with the message in err [cap].  In this order: the descriptor is
// there, its kind is one of the list, its nlatent is the kind's (categorical: 1 .. 64, and logtheta is there), its parameters are in
// the kind's domain.  What one entry point alone refuses (a kind it does not take, a non-finite logtheta[k] found while copying)
// stays with that entry point, after this check.
inline int32_t agpl_lik_desc_check(const agpl_lik_desc *lik, char *err, size_t cap) {
#define AGPL_LIK_REFUSE_(...)                              \
    do {                                                   \
        if (err && cap) snprintf(err, cap, __VA_ARGS__);   \
        return AGPL_ERR_INVALID_ARGUMENT;                  \
    } while (0)
    if (!lik) AGPL_LIK_REFUSE_("null likelihood descriptor");
    if (!agpl_lik_kind_known(lik->kind)) AGPL_LIK_REFUSE_("unknown likelihood kind %d", lik->kind);
    if (lik_is_categorical(lik->kind)) {
        if (lik->nlatent < 1 || lik->nlatent > 64 || !lik->logtheta) AGPL_LIK_REFUSE_("categorical needs 1 <= nlatent <= 64 and logtheta");
    } else if (lik->nlatent != agpl_lik_nlatent(lik->kind)) {
        AGPL_LIK_REFUSE_("nlatent = %d, expected %d", lik->nlatent, agpl_lik_nlatent(lik->kind));
    }
    // the rule table: one case per kind; a kind of the list that has none here is refused, not passed
    const double p0 = lik->p[0], p1 = lik->p[1];
    switch (lik->kind) {
    case AGPL_LIK_BERNOULLI_LOGISTIC: // no parameter
    case AGPL_LIK_CATEGORICAL:        // (logtheta, above)
    case AGPL_LIK_CATEGORICAL_BIJ:
    case AGPL_LIK_BINOMIAL_N: // p[] is not read: the trials are data
        break;
    case AGPL_LIK_NEGBINOMIAL:
        if (!(p0 > 0.0 && isfinite(p0))) AGPL_LIK_REFUSE_("NegBinomial failures r must be > 0");
        break;
    case AGPL_LIK_BINOMIAL:
        if (!(p0 >= 1.0 && p0 < 4194304.0 && p0 == floor(p0)))
            AGPL_LIK_REFUSE_("Binomial trials n must be an integer with 1 <= n < 4194304 = 2^22 (n = %g)", p0);
        break;
    case AGPL_LIK_STUDENTT:
        if (!(p0 > 0.0 && p1 > 0.0 && isfinite(p0) && isfinite(p1))) AGPL_LIK_REFUSE_("StudentT needs nu > 0 and sigma > 0");
        break;
    case AGPL_LIK_POISSON:
    case AGPL_LIK_HETEROGAUSS:
        if (!(p0 > 0.0 && isfinite(p0))) AGPL_LIK_REFUSE_("the link's scale lambda must be > 0");
        break;
    case AGPL_LIK_LAPLACE:
        if (!(p0 > 0.0 && isfinite(p0))) AGPL_LIK_REFUSE_("Laplace needs beta > 0");
        break;
    case AGPL_LIK_ASYMLAPLACE:
        if (!agpl_asymlaplace_ok(p0, p1)) AGPL_LIK_REFUSE_(AGPL_ASYMLAPLACE_MSG, p0, p1);
        break;
    case AGPL_LIK_LOGISTIC_NOISE:
        if (!agpl_logistic_noise_ok(p0)) AGPL_LIK_REFUSE_(AGPL_LOGISTIC_NOISE_MSG, p0);
        break;
    default:
        AGPL_LIK_REFUSE_("likelihood kind %d has no parameter rule", lik->kind);
    }
#undef AGPL_LIK_REFUSE_
    return AGPL_OK;
}

namespace agpl {

// The one host switch over the kind: what body(std::integral_constant<int, K>{}) returns for the K that equals `kind`; false if
// the list has none.  A launch site passes a generic lambda that launches kernel<K()> and returns true; it names with
// `if constexpr` only the kinds it treats differently (the branches it discards are not instantiated) and returns false for a
// kind it has no kernel for, so that a false from here is that site's refusal, never a launch of some other kind's kernel.
template <class BODY>
inline bool lik_switch(int kind, BODY body) {
    switch (kind) {
#define AGPL_LIK_CASE_(K) \
    case K:               \
        return body(std::integral_constant<int, K>{});
        AGPL_LIK_KINDS(AGPL_LIK_CASE_)
#undef AGPL_LIK_CASE_
    default:
        return false;
    }
}

} // namespace agpl
