// agpl_logistic_noise.h -- the logistic-noise kind's rule over the noise's own measure (AGPL_LIK_LOGISTIC_NOISE, agpl.h), stated once
// for the two libraries that need it: libagpl_quantile.so (both tails and the density) and libagpl_likgrad.so (the expected
// log-likelihood and its derivative).  Device code, float64.
//
// With eps ~ Logistic(0, 1), g ~ N(m, R^2), m = (y - mu) / s, R = sqrt(var) / s, every expectation the kind takes of the logistic
// under q(f) is also an expectation of a Gaussian function under the logistic density sigma'(t) = sigma(t) sigma(-t):
//     E sigma(g)           = E_eps Phi(z),        z = (m - eps) / R           (P(Y <= y); the other tail is E_eps Phi(-z))
//     E sigma(g) sigma(-g) = E_eps phi(z) / R                                 (s p(y), and (e1 - e2) of the derivative)
//     E 2 log 2cosh(g / 2) = -m + 2 R E_eps G(z), G(z) = z Phi(z) + phi(z)    (twice by parts: (2 log 2cosh)'' = 2 sigma')
// The rules over N(m, R^2) (peak_integral, sigma_moments, logistic_expectations) place nodes kPoleCap apart over m +- 8 R and so
// stop at R = 64 .. 200; R = sqrt(var) / s is not bounded by the count kinds' s <= 50 (s = 1e-3 under sqrt(var) = 50: R = 5e4).
// Over eps the integrand is sigma'(t) times a function that varies on the scale R: the trapezoid rule centred on the mode 0 of
// sigma', spacing kLnStep = 1/2 (poles of sigma' at +- i pi: the error is 2 pi w / sinh(pi w) at w = 2 pi / kLnStep, 1.7e-15
// of the integral; the Gaussian factor adds exp(-2 pi^2 R^2 / kLnStep^2), nothing for R >= 1), out to |t| = kLnSpan = 50, where
// sigma' is exp(-50) = 2e-22: what is cut is below 4e-22 of mass, absolute, in any of the sums.  The sums are normalised by the
// rule's own weights.  It serves R >= kLnSwitch = 1; below, the rules over N(m, R^2) do, with nodes R / 4 <= 1/4 apart (32 a side):
// at the spacing pi / 4 that those rules take for R >= pi, the expected log-likelihood's gradient, which multiplies
// E sigma(g) sigma(-g) (a double pole at i pi) by 2 R^2, was 1.4e-9 off at R = 7.99 on the MI355X against a bar of 2.5e-11.
#pragma once
#include <math.h>

namespace agpl {

constexpr double kLnSwitch = 1.0; // R = sqrt(var) / s from which the rule over the noise's measure is taken
constexpr double kLnStep = 0.5;
constexpr int kLnHalf = 100;      // nodes on each side of 0: |t| <= 50

struct LnSums {
    double lo, hi, phi, g; // E Phi(z), E Phi(-z), E phi(z), E G(z) under eps ~ Logistic(0, 1); g only where asked for
};
// each tail is a sum of positive terms: the smaller of Phi(z), Phi(-z) is erfc(|z| / sqrt 2) / 2 and the larger what is left of 1
template <bool WITH_G>
__device__ inline LnSums ln_noise_rule(double m, double R) {
    const double iR = 1.0 / R;
    double w0 = 0.0, lo = 0.0, hi = 0.0, ph = 0.0, gs = 0.0;
    for (int j = -kLnHalf; j <= kLnHalf; ++j) {
        const double t = (double)j * kLnStep, e = exp(-fabs(t)), sp = 1.0 / (1.0 + e), w = e * sp * sp;
        const double z = (m - t) * iR, tail = 0.5 * erfc(fabs(z) * 0.70710678118654752440), rest = 1.0 - tail;
        const double pz = exp(-0.5 * z * z) * 0.39894228040143267794, Pz = z < 0.0 ? tail : rest;
        w0 += w;
        lo += w * Pz;
        hi += w * (z < 0.0 ? rest : tail);
        ph += w * pz;
        if (WITH_G) gs += w * (z * Pz + pz);
    }
    const double iw = 1.0 / w0;
    return LnSums{lo * iw, hi * iw, ph * iw, gs * iw};
}

} // namespace agpl
