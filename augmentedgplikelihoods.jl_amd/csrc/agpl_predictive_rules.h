// agpl_predictive_rules.h -- the per-point quadrature rules of the predictive distribution of y, stated once for the two libraries
// that integrate p(y | f) or its distribution function over q(f) = N(mu, var): libagpl_predictive.so (agpl_predictive.hip) and
// libagpl_quantile.so (agpl_quantile.hip).  The rules' constants (kGrid, kSpan, kPoleCap, kMaxHalf, ...) are stated by
// agpl_predictive.hip, which includes this file after them; agpl_quantile.hip takes both by including agpl_predictive.hip with
// AGPL_PREDICTIVE_RULES_ONLY defined.  (The constants are not here because tests/test_predictive_domain_cpu.py and
// tests/seam_shapes.py read them out of agpl_predictive.hip by name; moving them means changing those tests.)  Device code, float64, no fused-multiply-add contraction (csrc/Makefile: NOFMA).
#ifndef AGPL_PREDICTIVE_RULES_H
#define AGPL_PREDICTIVE_RULES_H

namespace {

// sigma(f), sigma(-f), log sigma(f), log sigma(-f) without cancellation or overflow for any finite f
struct SigTerms {
    double sig, sgc, lsp, lsn;
};
__device__ __forceinline__ SigTerms sig_terms(double f) {
    const double e = exp(-fabs(f)), sp = 1.0 / (1.0 + e), l1p = log1p(e);
    SigTerms o;
    const bool pos = f >= 0.0;
    o.sig = pos ? sp : e * sp;
    o.sgc = pos ? e * sp : sp;
    o.lsp = pos ? -l1p : f - l1p;
    o.lsn = pos ? -f - l1p : -l1p;
    return o;
}

// lp(f) = A log sigma(f) + B log sigma(-f) - Lam sigma(f): Bernoulli (A, B = y, 1 - y), NegBinomial (y, r), Binomial (y, n - y), Poisson (A = y, Lam = lambda)
// up to the constant of y
struct CountLik {
    double A, B, Lam;
    __device__ __forceinline__ double lp(double f) const {
        const SigTerms t = sig_terms(f);
        return A * t.lsp + B * t.lsn - Lam * t.sig;
    }
    __device__ __forceinline__ void eval(double f, double &l, double &d1, double &d2) const {
        const SigTerms t = sig_terms(f);
        const double ssc = t.sig * t.sgc;
        l = A * t.lsp + B * t.lsn - Lam * t.sig;
        d1 = A * t.sgc - B * t.sig - Lam * ssc;
        d2 = -(A + B) * ssc - Lam * ssc * (1.0 - 2.0 * t.sig);
    }
    // Poisson: -Lam sigma(f) is convex for f > 0, so h may have a second maximum far from mu; it is then near the likelihood's own,
    // sigma(f) = A / Lam.  The other two are log-concave.
    __device__ __forceinline__ bool candidate(double &f) const {
        if (!(Lam > 0.0 && A > 0.0 && A < Lam)) return false;
        f = log(A / (Lam - A));
        return true;
    }
};

// lg(g) = -log(v) / 2 - d2 / (2 v), v = vf + (1 + exp(-g)) / lam: log N(y; mu_f, v(g)) up to -log(2 pi) / 2, f integrated out
struct HeteroLik {
    double vf, ilam, d2;
    __device__ __forceinline__ double lp(double g) const {
        const double v = vf + ilam + exp(-g) * ilam;
        return -0.5 * log(v) - 0.5 * d2 / v;
    }
    __device__ __forceinline__ void eval(double g, double &l, double &d1, double &dd) const {
        const double e = exp(-g) * ilam, v = vf + ilam + e; // v' = -e, v'' = e
        const double q = -0.5 * e / v, r = d2 / v - 1.0;
        l = -0.5 * log(v) - 0.5 * d2 / v;
        d1 = q * r;
        dd = (0.5 * e / v - 0.5 * e * e / (v * v)) * r + q * d2 * e / (v * v);
    }
    __device__ __forceinline__ bool candidate(double &) const { return false; }
};

// log int exp(lik.lp(f)) N(f; mu, var) df for var > 0.  h(f) = lp(f) - (f - mu)^2 / (2 var): maximum on the grid (moved, and doubled in
// width, while it lies on an edge), the likelihood's own candidate, safeguarded Newton steps between the best point's neighbours
// (bisection where a step leaves them or h is not concave; stopped when a step is kNewtonTol of the width), width
// w = min(s, (-h'')^-1/2), then the trapezoid rule centred there with spacing min(w / 2, s / 4, kPoleCap) over +- 8 s: fine enough
// for the peak and for the poles at distance pi from the real axis (the rule's error falls as exp(-2 pi a / spacing) for an
// integrand analytic in a strip of half-width a).  At s = 50, the largest of the supported domain, kPoleCap gives 800 points a
// side: kMaxHalf binds only through w, where the window is 512 widths.  The terms are scaled by the largest so far, so a centre
// beside the maximum cannot overflow the sum.
template <class Lik>
__device__ double peak_integral(const Lik &lik, double mu, double var) {
    const double s = sqrt(var), iv = 1.0 / var;
    double d = 2.0 * kSpan * s / (kGrid - 1);
    // (a maximum on the grid's edge -- a likelihood that pulls the mode more than 8 s from mu, s^2 (y + r) at most -- moves the grid
    // there, doubles its spacing and looks again: 8 s (2^32 - 1) at most)
    double best = -INFINITY, m = mu, c = mu;
    for (int rep = 0; rep < kRecentre; ++rep) {
        int kb = (kGrid - 1) / 2;
        for (int k = 0; k < kGrid; ++k) {
            const double f = c + (double)(k - (kGrid - 1) / 2) * d;
            const double h = lik.lp(f) - 0.5 * (f - mu) * (f - mu) * iv;
            if (h > best) {
                best = h;
                m = f;
                kb = k;
            }
        }
        if (kb != 0 && kb != kGrid - 1) break;
        c = m;
        d *= 2.0;
    }
    double l, d1, d2, lo = m - d, hi = m + d, fc;
    if (lik.candidate(fc) && lik.lp(fc) - 0.5 * (fc - mu) * (fc - mu) * iv > best) {
        // at the candidate lp' = 0, so h' = (mu - fc) / var points to mu: the maximum lies between the candidate and the first point
        // towards mu where h' has changed sign (steps of d, doubled; h' has changed at mu at the latest for this likelihood)
        const double sgn = mu > fc ? 1.0 : -1.0;
        double step = d, t = fc;
        for (int it = 0; it < kBracket; ++it) {
            t = fc + sgn * step;
            lik.eval(t, l, d1, d2);
            if (sgn * (d1 - (t - mu) * iv) <= 0.0) break;
            step *= 2.0;
        }
        m = fc;
        lo = fmin(fc, t);
        hi = fmax(fc, t);
    }
    for (int it = 0; it < kNewton; ++it) {
        lik.eval(m, l, d1, d2);
        const double h1 = d1 - (m - mu) * iv, h2 = d2 - iv;
        if (h1 == 0.0) break;
        if (h1 > 0.0)
            lo = m;
        else
            hi = m;
        double t = h2 < 0.0 ? m - h1 / h2 : lo;
        if (!(lo < t && t < hi)) t = 0.5 * (lo + hi);
        const bool done = h2 < 0.0 && fabs(t - m) * sqrt(-h2) <= kNewtonTol;
        m = t;
        if (done) break;
    }
    lik.eval(m, l, d1, d2);
    const double h2 = d2 - iv;
    const double w = h2 >= 0.0 ? s : fmin(s, 1.0 / sqrt(-h2));
    const double hm = l - 0.5 * (m - mu) * (m - mu) * iv;
    const double dl = fmin(fmin(0.5 * w, 0.25 * s), kPoleCap);
    const int nh = (int)fmin(ceil(kSpan * s / dl), (double)kMaxHalf);
    double mx = hm, acc = 0.0;
    for (int j = -nh; j <= nh; ++j) {
        const double f = m + (double)j * dl;
        const double e = lik.lp(f) - 0.5 * (f - mu) * (f - mu) * iv;
        if (e > mx) {
            acc = acc * exp(mx - e) + 1.0;
            mx = e;
        } else {
            acc += exp(e - mx);
        }
    }
    return mx + log(acc) + log(dl) - log(s) - kLogSqrt2Pi;
}

// E sigma(f), E sigma(f)^2 under N(mu, var): the trapezoid rule over mu +- 8 s with the seed grid's spacing s / 4 (32 points a side)
// while that is at most kPoleCap (s <= 2), else ceil(8 s / kPoleCap) points a side (at most kMaxHalf); normalised by its own weights
__device__ void sigma_moments(double mu, double var, double &e1, double &e2) {
    const double s = sqrt(var);
    const int nh = (int)fmin(fmax((double)((kGrid - 1) / 2), ceil(kSpan * s / kPoleCap)), (double)kMaxHalf); // (kMaxHalf: s > 64)
    const double dx = kSpan / (double)nh;
    double a0 = 0.0, a1 = 0.0, a2 = 0.0;
    for (int k = -nh; k <= nh; ++k) {
        const double x = (double)k * dx;
        const double wt = exp(-0.5 * x * x), sg = sig_terms(mu + s * x).sig;
        a0 += wt;
        a1 += wt * sg;
        a2 += wt * sg * sg;
    }
    e1 = a1 / a0;
    e2 = a2 / a0;
}

// Student-t(nu, sg) observation under q(f) = N(mu, var): p(y) = E_x N(y; mu, var + c / x), x ~ Gamma(a, 1), a = nu / 2,
// c = nu sg^2 / 2 (the scale mixture of the augmentation, studentt.jl:85-91), in t = log x:
// g(t) = a t - e^t - log(v) / 2 - dd / (2 v), v = var + c e^-t, and its first two derivatives
struct StLik {
    double a, c, var, dd;
    __device__ __forceinline__ void eval(double t, double &g, double &g1, double &g2) const {
        const double x = exp(t), u = c / x, v = var + u;
        g = a * t - x - 0.5 * log(v) - 0.5 * dd / v;
        g1 = a - x + 0.5 * u / v - 0.5 * dd * u / (v * v);
        g2 = -x - 0.5 * u * var / (v * v) + 0.5 * dd * u * (var - u) / (v * v * v);
    }
    __device__ __forceinline__ double lp(double t) const {
        const double x = exp(t), v = var + c / x;
        return a * t - x - 0.5 * log(v) - 0.5 * dd / v;
    }
    __device__ double newton(double t) const {
        double g, g1, g2;
        for (int it = 0; it < kStNewton; ++it) {
            eval(t, g, g1, g2);
            if (g2 >= 0.0) break;
            t += fmin(fmax(-g1 / g2, -kStStep), kStStep);
        }
        return t;
    }
};

// The Gamma density in t has width a^-1/2 for large a and a left tail exp(a t) for small a, and the Gaussian factor moves the peak
// by up to log(1 + dd / 2c): no fixed range and point count serves nu from 0.01 to 1e6.  So: Newton from two starts -- the Gamma
// density's own mode log a, and log((a + 1/2) / (1 + dd / 2c)), the mode where c / x dominates var -- the higher result is the
// centre, spacing min(w / 2, kPoleCap) with w = (-g'')^-1/2 there (for a Gaussian peak the rule's error is exp(-2 pi^2 w^2 / h^2)
// = exp(-79); for the Gamma density it is |Gamma(a + 2 pi i / h)| / Gamma(a) <= exp(-pi^2 / h) = 3e-9 at h = 1/2), and the rule
// marches out on each side until a term falls below exp(-kStDrop) of the largest so far (the tails fall at least as exp((a + 1/2) t)
// and exp(-e^t), so what is cut is below exp(-30) / ((a + 1/2) h) of the sum).  Where the other start ended on a second maximum within
// exp(-kStDrop) of the first (possible for sg^2 < var / 2), the march does not stop before it has passed it.
__device__ double studentt_logp(double nu, double sg, double y, double mu, double var) {
    const double a = 0.5 * nu, c = 0.5 * nu * sg * sg, dd = (y - mu) * (y - mu);
    if (var == 0.0) {
        const double z = (y - mu) / sg;
        return lgamma(0.5 * (nu + 1.0)) - lgamma(a) - 0.5 * log(nu * agpl::kPi) - log(sg) - 0.5 * (nu + 1.0) * log1p(z * z / nu);
    }
    const StLik lik{a, c, var, dd};
    double ta = lik.newton(log(a)), tb = lik.newton(log((a + 0.5) / (1.0 + 0.5 * dd / c)));
    double ga, gb, g1, ga2, gb2;
    lik.eval(ta, ga, g1, ga2);
    lik.eval(tb, gb, g1, gb2);
    if (gb > ga) {
        double t = ta;
        ta = tb, tb = t;
        t = ga, ga = gb, gb = t;
        ga2 = gb2;
    }
    const double w = ga2 < 0.0 ? 1.0 / sqrt(-ga2) : 1.0, h = fmin(0.5 * w, kPoleCap);
    const bool other = gb > ga - kStDrop;
    double mx = ga, sum = 1.0;
    for (int side = 0; side < 2; ++side) {
        const double sgn = side == 0 ? 1.0 : -1.0;
        for (int j = 1; j <= kStMaxHalf; ++j) {
            const double t = ta + sgn * (double)j * h, li = lik.lp(t);
            if (li > mx) {
                sum = sum * exp(mx - li) + 1.0;
                mx = li;
            } else {
                sum += exp(li - mx);
            }
            if (li < mx - kStDrop && !(other && sgn * (tb - t) > 0.0)) break;
        }
    }
    return mx + log(sum) + log(h) - lgamma(a) - kLogSqrt2Pi;
}

// Laplace(beta) observation: (1 / 4 beta) [exp(e0 - d / beta) erfc(z1) + exp(e0 + d / beta) erfc(z2)], e0 = var / (2 beta^2),
// z = (s / beta -+ d / s) / sqrt 2; for z > 0 in the scaled form exp(-d^2 / 2 var) erfcx(z), which cannot overflow
__device__ double laplace_logp(double beta, double y, double mu, double var) {
    const double d = y - mu;
    if (var == 0.0) return -fabs(d) / beta - log(2.0 * beta);
    const double s = sqrt(var), q = 0.5 * d * d / var, e0 = 0.5 * var / (beta * beta);
    const double z1 = (s / beta - d / s) * agpl::kSqrtHalf, z2 = (s / beta + d / s) * agpl::kSqrtHalf;
    const double t1 = z1 > 0.0 ? -q + log(erfcx(z1)) : e0 - d / beta + log(erfc(z1));
    const double t2 = z2 > 0.0 ? -q + log(erfcx(z2)) : e0 + d / beta + log(erfc(z2));
    const double hi = fmax(t1, t2), lo = fmin(t1, t2);
    return hi + log1p(exp(lo - hi)) - log(4.0 * beta);
}

// Asymmetric Laplace(sigma, tau) observation (agpl.h), a = tau / sigma, b = (1 - tau) / sigma:
// (tau (1 - tau) / 2 sigma) [exp(ea - a d) erfc(z1) + exp(eb + b d) erfc(z2)], ea = a^2 var / 2, eb = b^2 var / 2,
// z1 = (a s - d / s) / sqrt 2, z2 = (b s + d / s) / sqrt 2: laplace_logp's two terms with a rate each (1 / beta = a = b at tau = 1/2)
__device__ double asymlaplace_logp(double sigma, double tau, double y, double mu, double var) {
    const double d = y - mu, a = tau / sigma, b = (1.0 - tau) / sigma, lc = log(tau * (1.0 - tau) / sigma);
    if (var == 0.0) return lc - (d < 0.0 ? -b * d : a * d);
    const double s = sqrt(var), q = 0.5 * d * d / var, ea = 0.5 * var * a * a, eb = 0.5 * var * b * b;
    const double z1 = (s * a - d / s) * agpl::kSqrtHalf, z2 = (s * b + d / s) * agpl::kSqrtHalf;
    const double t1 = z1 > 0.0 ? -q + log(erfcx(z1)) : ea - d * a + log(erfc(z1));
    const double t2 = z2 > 0.0 ? -q + log(erfcx(z2)) : eb + d * b + log(erfc(z2));
    const double hi = fmax(t1, t2), lo = fmin(t1, t2);
    return hi + log1p(exp(lo - hi)) + lc - agpl::kLogTwo;
}

// Logistic noise of scale sc (agpl.h): p(y) = E sigma(g) sigma(-g) / sc, g ~ N(m, R^2), m = (y - mu) / sc, R^2 = var / sc^2 -- the count
// rule at the exponent pair (1, 1).  The peak of the integrand is at most the logistic density's own width wide, however large R
// is, so peak_integral's window (512 widths where kMaxHalf binds) holds it: DESIGN.md 4.31.  Not formed as e1 - e2 of
// sigma_moments, which cancels in the tails.
// Below R^2 = kLnNarrowVar the rule is the second-order expansion instead, log E exp(lp(g)) = lp(m) + R^2 (lp'' + lp'^2) / 2 + O(R^4)
// (below 1e-12: lp varies on the scale 1).  peak_integral places its nodes R / 4 apart about m, and |m| reaches 91 here (50 predictive
// standard deviations), where a node is rounded to 1.4e-14: at R = 1e-11 (sqrt(var) = 1e-8 under s = 1e3) that is 6e-3 of the spacing
// and cost 1.4e-4 in log p on the MI355X; at R = 1e-3 it is 6e-11 of it.
constexpr double kLnNarrowVar = 1e-6;
template <class Lik>
__device__ __forceinline__ double narrow_integral(const Lik &lik, double m, double R2) {
    double l, d1, d2;
    lik.eval(m, l, d1, d2);
    return l + 0.5 * R2 * (d2 + d1 * d1);
}
// log E exp(lik.lp(g)), g ~ N(m, R2), for the logistic-noise kind's three exponent pairs, R2 > 0
__device__ double logistic_noise_integral(const CountLik &lik, double m, double R2) {
    return R2 < kLnNarrowVar ? narrow_integral(lik, m, R2) : peak_integral(lik, m, R2);
}
__device__ double logistic_noise_logp(double sc, double y, double mu, double var) {
    if (!isfinite(y)) return (isnan(y) || var > 0.0) ? NAN : -INFINITY; // (what laplace_logp's arithmetic gives: no rule is run at m = +-inf)
    const CountLik lik{1.0, 1.0, 0.0};
    const double m = (y - mu) / sc;
    return (var == 0.0 ? lik.lp(m) : logistic_noise_integral(lik, m, var / (sc * sc))) - log(sc);
}

__device__ __forceinline__ bool bad_marginal(double mu, double var) { return !(isfinite(mu) && isfinite(var) && var >= 0.0); }

} // namespace
#endif // AGPL_PREDICTIVE_RULES_H
