// agpl_digamma.h -- psi(x) = d/dx log Gamma(x) for x > 0, stated ONCE for the device (agpl_likgrad.hip) and for the host (a plain
// C++ translation unit may include this file: tests/test_likgrad_reference_cpu.py compiles it against scipy.special.digamma).
// Upward recurrence psi(x) = psi(x + 1) - 1 / x until x >= 6, then the asymptotic series
//     psi(x) ~ log x - 1 / (2 x) - sum_k B_2k / (2 k x^2k),   k = 1 .. 10
// whose first omitted term is 2e-15 at x = 6 (psi(6) = 1.706).  No library digamma is called; log is the only library function.
// Relative error: a few ulp away from the root of psi at x = 1.4616 (where only the absolute error is small).  x <= 0 or NaN: NaN.
#pragma once
#include <math.h>

#if defined(__HIPCC__)
#define AGPL_HD __host__ __device__
#else
#define AGPL_HD
#endif

namespace agpl {

AGPL_HD inline double digamma(double x) {
    if (!(x > 0.0)) return NAN;
    double r = 0.0;
    while (x < 6.0) {
        r -= 1.0 / x;
        x += 1.0;
    }
    const double y = 1.0 / (x * x);
    // B_2k / (2 k), k = 10 .. 1 (Horner in y = x^-2)
    double p = -174611.0 / 6600.0;
    p = p * y + 43867.0 / 14364.0;
    p = p * y - 3617.0 / 8160.0;
    p = p * y + 1.0 / 12.0;
    p = p * y - 691.0 / 32760.0;
    p = p * y + 1.0 / 132.0;
    p = p * y - 1.0 / 240.0;
    p = p * y + 1.0 / 252.0;
    p = p * y - 1.0 / 120.0;
    p = p * y + 1.0 / 12.0;
    return r + (log(x) - 0.5 / x - p * y);
}

} // namespace agpl
