// agpl_quantile.hip -- libagpl_quantile.so (include/agpl_quantile.h): P(Y <= y), P(Y > y) and the quantiles of the predictive
// p(y) = int p(y | f) q(f) df per point.  float64, one lane per point, no reductions, no allocation; the rules, the domain and the
// measured errors are in DESIGN.md 4.25.  The distribution function is the expectation that agpl_predictive.hip takes of the
// density, with F(y | f) in place of p(y | f): the rules over q(f) and their constants are that file's (agpl_predictive_rules.h),
// not restated here.  Compiled without fused-multiply-add contraction, like agpl_predictive.hip.
#include <math.h>

#include "../../include/agpl_quantile.h"
#define AGPL_PREDICTIVE_RULES_ONLY
#include "agpl_predictive.hip"
#include "agpl_logistic_noise.h"

namespace {

constexpr int kQtBlocks = 65536;   // workgroups of one launch, at most (the lanes stride over the points)
constexpr int kQtMaxProbs = 16;    // probs of one agpl_predictive_quantile call, at most
constexpr int kQtNodes = 2048;     // Student-t: nodes of the rule in log w, at most (two tables of doubles in the workgroup's LDS)
constexpr double kQtMinNu = 0.2;   // Student-t: below it the left tail of the rule does not fit kQtNodes: refused
constexpr double kQtDrop = 50.0;   // Student-t: the rule ends where the Gamma weight is exp(-50) of its largest
constexpr double kQtStCap = 0.25;  // Student-t: largest spacing in log w (|Gamma(a + 2 pi i / h)| / Gamma(a) <= exp(-pi^2 / h) = 7e-18)
constexpr double kQtSpan = 10.0;   // heteroscedastic: the rule over g covers mu_g +- 10 s_g (the mass beyond is 1.5e-23: a tail of
                                   // 1e-12 that lives at g < mu_g - 8 s_g keeps four digits)
constexpr int kQtMinHalf = 40;     // heteroscedastic: points a side at least (spacing s_g / 4)
constexpr int kQtDouble = 1100;    // doublings of the bracket, at most (the last reach +-inf, where the tails are 0 and 1)
constexpr int kQtSteps = 200;      // Newton / bisection steps of one quantile, at most
constexpr double kQtTol = 1e-10;   // a quantile is done at |F - p| <= kQtTol (or at a two-ulp bracket)
constexpr double kInvSqrt2Pi = 0.39894228040143267794;

// ---- Student-t: the Gamma scale mixture in tau = log(w / mode) -------------------------------------------------------------------
// F(y) = E_w Phi((y - mu) / sqrt(var + sg^2 / w)), w ~ Gamma(a, rate a), a = nu / 2.  In tau = log w (the mode of the density of
// log w is w = 1) the weight is exp(-a (e^tau - 1 - tau)) / norm: width a^-1/2 for large a, a left tail exp(a tau) for small a.
// Nodes tau_j = (j - nl) h, j < cnt, h = min(a^-1/2 / 2, kQtStCap), out to where the weight is exp(-kQtDrop); they depend on
// (nu, sg) alone, so the host marches them once per call, sums the weights (norm) and every workgroup forms the two tables
// weight_j, sg^2 / w_j in LDS once.  Phi(d / sqrt(var + sg^2 e^-tau)) is analytic and bounded for |Im tau| < pi / 2 (Re z^2 > 0
// there), so the trapezoid rule's error is exp(-2 pi (pi / 2) / h) <= 7e-18 of the bound.
struct StRule {
    double a, h, lognorm, sg2;
    int nl, cnt;
};

StRule st_rule(double nu, double sg) {
    StRule r;
    r.a = 0.5 * nu;
    r.sg2 = sg * sg;
    r.h = fmin(0.5 / sqrt(r.a), kQtStCap);
    int nr = 0, nl = 0;
    while (nr < kQtNodes / 2 && r.a * (expm1((nr + 1) * r.h) - (nr + 1) * r.h) <= kQtDrop) ++nr;
    while (nl < kQtNodes - 1 - nr && r.a * (expm1(-(nl + 1) * r.h) + (nl + 1) * r.h) <= kQtDrop) ++nl;
    r.nl = nl;
    r.cnt = nl + nr + 1;
    double sum = 0.0;
    for (int j = 0; j < r.cnt; ++j) {
        const double tau = (double)(j - nl) * r.h;
        sum += exp(-r.a * (expm1(tau) - tau));
    }
    r.lognorm = log(sum);
    return r;
}

__device__ void st_tables(const StRule &r, double *__restrict__ tw, double *__restrict__ tu) {
    for (int j = threadIdx.x; j < r.cnt; j += kBlock) {
        const double tau = (double)(j - r.nl) * r.h;
        tw[j] = exp(-r.a * (expm1(tau) - tau) - r.lognorm);
        tu[j] = r.sg2 * exp(-tau);
    }
    __syncthreads();
}

// Each evaluator gives the tail on the side of its own location from positive terms (0.5 erfc(|z|)), and the other tail as what
// is left of the rule's weights: never 1 - (a number near 1) for the tail that is small.
struct StEval {
    const double *tw, *tu;
    int cnt;
    double mu, var;
    template <bool PDF>
    __device__ void eval(double y, double &cdf, double &sf, double &pdf) const {
        const double d = y - mu, ad = fabs(d) * agpl::kSqrtHalf;
        double w0 = 0.0, t = 0.0, p = 0.0;
        for (int j = 0; j < cnt; ++j) {
            const double w = tw[j], r = 1.0 / sqrt(var + tu[j]), z = ad * r;
            w0 += w;
            t += w * (0.5 * erfc(z));
            if (PDF) p += w * (exp(-z * z) * r);
        }
        cdf = d < 0.0 ? t : w0 - t;
        sf = d < 0.0 ? w0 - t : t;
        pdf = p * kInvSqrt2Pi;
    }
};

// Laplace(beta): F = Phi(d / s) - exp(e0 - d / beta) Phi(d / s - s / beta) / 2 + exp(e0 + d / beta) Phi(-d / s - s / beta) / 2,
// e0 = s^2 / (2 beta^2).  With z0 = -d / (s sqrt 2), z1, z2 = (s / beta -+ d / s) / sqrt 2 of laplace_logp and q = d^2 / (2 s^2),
// exp(e0 -+ d / beta) erfc(z) = exp(-q) erfcx(z), so for d <= 0 (z0 >= 0, z1 > 0)
//     F = exp(-q) (erfcx(z0) / 2 - erfcx(z1) / 4) + [ z2 > 0: exp(-q) erfcx(z2) / 4;  else exp(e0 + d / beta) erfc(z2) / 4 ]
// where erfcx(z0) > erfcx(z1) and, for z2 <= 0, e0 + d / beta <= -e0: nothing overflows and nothing cancels.  The predictive is
// symmetric about mu: the other tail is the mirror image.
struct LapEval {
    double beta, mu, var;
    __device__ double lower_tail(double d) const { // d <= 0
        if (var == 0.0) return 0.5 * exp(d / beta);
        const double s = sqrt(var), q = 0.5 * d * d / var, e0 = 0.5 * var / (beta * beta), eq = exp(-q);
        const double z0 = -d / s * agpl::kSqrtHalf, z1 = (s / beta - d / s) * agpl::kSqrtHalf, z2 = (s / beta + d / s) * agpl::kSqrtHalf;
        const double third = z2 > 0.0 ? 0.25 * eq * erfcx(z2) : 0.25 * exp(e0 + d / beta) * erfc(z2);
        return eq * (0.5 * erfcx(z0) - 0.25 * erfcx(z1)) + third;
    }
    template <bool PDF>
    __device__ void eval(double y, double &cdf, double &sf, double &pdf) const {
        const double d = y - mu, t = lower_tail(-fabs(d));
        cdf = d < 0.0 ? t : 1.0 - t;
        sf = d < 0.0 ? 1.0 - t : t;
        pdf = PDF ? exp(laplace_logp(beta, y, mu, var)) : 0.0;
    }
};

// Asymmetric Laplace(sigma, tau), a = tau / sigma, b = (1 - tau) / sigma, ea = a^2 s^2 / 2, eb = b^2 s^2 / 2:
//     F = Phi(d / s) - (1 - tau) exp(ea - a d) Phi(d / s - a s) + tau exp(eb + b d) Phi(-d / s - b s)
// The predictive is not symmetric, so each tail is formed as such, on its own side of mu: with the rearrangement of
// LapEval::lower_tail, for t <= 0 the distance to mu on the tail's side,
//     tail(t; r1, w1, r2, w2) = exp(-q) (erfcx(z0) / 2 - w1 erfcx(z1) / 2) + [ z2 > 0: w2 exp(-q) erfcx(z2) / 2;  else w2 exp(e2 + r2 t) erfc(z2) / 2 ]
// z0 = -t / (s sqrt 2), z1 = (r1 s - t / s) / sqrt 2 > z0, z2 = (r2 s + t / s) / sqrt 2, e2 = r2^2 s^2 / 2 (e2 + r2 t <= -e2 for z2 <= 0).
// P(Y <= y) = tail(d; a, 1 - tau, b, tau) for d <= 0 and P(Y > y) = tail(-d; b, tau, a, 1 - tau) for d >= 0: w1 < 1 and
// erfcx(z0) > erfcx(z1), so nothing overflows and nothing cancels.  The other tail is what is left of 1.
struct AldEval {
    double sigma, tau, mu, var;
    __device__ double tail(double t, double r1, double w1, double r2, double w2) const { // t <= 0
        if (var == 0.0) return w2 * exp(r2 * t);
        const double s = sqrt(var), q = 0.5 * t * t / var, e2 = 0.5 * var * r2 * r2, eq = exp(-q);
        const double z0 = -t / s * agpl::kSqrtHalf, z1 = (s * r1 - t / s) * agpl::kSqrtHalf, z2 = (s * r2 + t / s) * agpl::kSqrtHalf;
        const double third = z2 > 0.0 ? 0.5 * w2 * eq * erfcx(z2) : 0.5 * w2 * exp(e2 + r2 * t) * erfc(z2);
        return eq * (0.5 * erfcx(z0) - 0.5 * w1 * erfcx(z1)) + third;
    }
    template <bool PDF>
    __device__ void eval(double y, double &cdf, double &sf, double &pdf) const {
        const double d = y - mu, a = tau / sigma, b = (1.0 - tau) / sigma;
        const double t = d < 0.0 ? tail(d, a, 1.0 - tau, b, tau) : tail(-d, b, tau, a, 1.0 - tau);
        cdf = d < 0.0 ? t : 1.0 - t;
        sf = d < 0.0 ? 1.0 - t : t;
        pdf = PDF ? exp(asymlaplace_logp(sigma, tau, y, mu, var)) : 0.0;
    }
};

// Logistic noise of scale sc (agpl.h): with g ~ N(m, R^2), m = (y - mu) / sc, R = sqrt(var) / sc, P(Y <= y) = E sigma(g) and
// P(Y > y) = E sigma(-g), each formed as such.  R < kLnSwitch: the logarithm of each from peak_integral at the exponent pairs (1, 0)
// and (0, 1), whose window m +- 8 R holds all of the integrand there (logistic_noise_integral: the expansion below R^2 = kLnNarrowVar).
// R >= kLnSwitch: the rule over the noise's own measure
// (agpl_logistic_noise.h), both tails and the density from one pass over its nodes.  var = 0 is the logistic itself.
struct LnEval {
    double sc, mu, var;
    template <bool PDF>
    __device__ void eval(double y, double &cdf, double &sf, double &pdf) const {
        const double m = (y - mu) / sc;
        if (var == 0.0) {
            const SigTerms t = sig_terms(m);
            cdf = t.sig, sf = t.sgc;
            pdf = PDF ? t.sig * t.sgc / sc : 0.0;
            return;
        }
        const double R = sqrt(var) / sc;
        if (R >= agpl::kLnSwitch) {
            const agpl::LnSums r = agpl::ln_noise_rule<false>(m, R);
            cdf = r.lo, sf = r.hi;
            pdf = r.phi / (R * sc);
        } else {
            const double R2 = var / (sc * sc);
            cdf = fmin(exp(logistic_noise_integral(CountLik{1.0, 0.0, 0.0}, m, R2)), 1.0);
            sf = fmin(exp(logistic_noise_integral(CountLik{0.0, 1.0, 0.0}, m, R2)), 1.0);
            pdf = PDF ? exp(logistic_noise_logp(sc, y, mu, var)) : 0.0;
        }
    }
};

// Heteroscedastic Gaussian: F = E_g Phi((y - mu_f) / sqrt(var_f + (1 + exp(-g)) / lambda)), the trapezoid rule over
// g = mu_g + s_g x, |x| <= kQtSpan, spaced min(s_g / 4, kPoleCap) (v(g) = 0 lies at distance pi from the real axis), normalised by
// its own weights; var_g = 0 is the one node mu_g.
struct HetEval {
    double mf, vf, mg, sg, ilam, dx;
    int nh;
    __device__ HetEval(double mf_, double vf_, double mg_, double vg_, double lam) : mf(mf_), vf(vf_), mg(mg_), sg(sqrt(vg_)), ilam(1.0 / lam) {
        nh = vg_ == 0.0 ? 0 : (int)fmin(fmax((double)kQtMinHalf, ceil(kQtSpan * sg / kPoleCap)), (double)kMaxHalf);
        dx = nh ? kQtSpan / (double)nh : 0.0;
    }
    template <bool PDF>
    __device__ void eval(double y, double &cdf, double &sf, double &pdf) const {
        const double d = y - mf, ad = fabs(d) * agpl::kSqrtHalf;
        double w0 = 0.0, t = 0.0, p = 0.0;
        for (int k = -nh; k <= nh; ++k) {
            const double x = (double)k * dx, w = exp(-0.5 * x * x);
            const double v = vf + ilam + exp(-(mg + sg * x)) * ilam, r = 1.0 / sqrt(v), z = ad * r;
            w0 += w;
            t += w * (0.5 * erfc(z));
            if (PDF) p += w * (exp(-z * z) * r);
        }
        t /= w0;
        cdf = d < 0.0 ? t : 1.0 - t;
        sf = d < 0.0 ? 1.0 - t : t;
        pdf = p / w0 * kInvSqrt2Pi;
    }
};

// ---- the count likelihoods --------------------------------------------------------------------------------------------------------
// Given f, F(y | f) = Q(y + 1, lambda sigma(f)) (Poisson) and I_{sigma(-f)}(r, y + 1) (NegBinomial).  Their derivative in f is minus
//     k_y(f) = Pois(y; lambda sigma) lambda sigma sigma(-f)       and       sigma^(y+1) sigma(-f)^r / B(r, y + 1),
// exp(CountLik{y + 1, 1, lambda}.lp + c0) and exp(CountLik{y + 1, r, 0}.lp + c0), so by parts, the boundary terms being
// Q(y + 1, lambda) and 0 for the lower tail and 0 for the upper,
//     P(Y <= y) = [Q(y + 1, lambda)] + int Phi((f - mu) / s) k_y(f) df,          P(Y > y) = int Phi((mu - f) / s) k_y(f) df:
// both tails are sums of positive terms, and the integrand needs the mass function only.  k_y is unimodal, its maximum the root of
// Lam sig^2 - (A + B + Lam) sig + A = 0.  The integral is taken by composite 16-point Gauss-Legendre panels (no periodicity is
// needed where panels of different widths meet): from the maximum out to where k_y has fallen by exp(-kQtCountDrop), panels of half
// the peak's width (-h'')^-1/2, growing to a tenth of the distance from the maximum (at most 1 where the logistic still has
// structure, |f| < 50; beyond, k_y is a pure exponential); inside mu +- 10 s, where Phi steps, no panel is wider than s, so
// s = 1e-6 costs twenty panels more.  var = 0 is F(y | mu) itself: the regularised incomplete gamma (series for x < a + 1, modified
// Lentz continued fraction otherwise) and the incomplete beta by its continued fraction, each giving the smaller of the two tails.
constexpr int kQtCfIter = 20000;        // terms of a series or continued fraction, at most (a few sqrt(count cap))
constexpr double kQtCountDrop = 60.0;   // the panels end where k_y is exp(-60) of its maximum
constexpr int kQtPanels = 4096;         // panels of one integral, at most
constexpr double kQtInner = 10.0;       // panels within mu +- 10 s are at most s wide
constexpr double kQtTiny = 1e-300;
__constant__ double kGlX[8] = {0.095012509837637454, 0.28160355077925892, 0.45801677765722737, 0.61787624440264377,
                               0.755404408355003,    0.86563120238783176, 0.9445750230732326,  0.98940093499164994};
__constant__ double kGlW[8] = {0.18945061045506859, 0.18260341504492361, 0.16915651939500262,  0.14959598881657676,
                               0.12462897125553403, 0.095158511682492591, 0.062253523938647706, 0.027152459411754037};

// P(a, x), Q(a, x), lx = log x
__device__ void gamma_pq(double a, double x, double lx, double &P, double &Q) {
    if (!(x > 0.0)) {
        P = 0.0, Q = 1.0;
        return;
    }
    const double pre = exp(a * lx - x - lgamma(a));
    if (x < a + 1.0) {
        double ap = a, del = 1.0 / a, sum = del;
        for (int n = 0; n < kQtCfIter; ++n) {
            ap += 1.0;
            del *= x / ap;
            sum += del;
            if (del < sum * 1e-17) break;
        }
        P = pre * sum;
        Q = 1.0 - P;
    } else {
        double b = x + 1.0 - a, c = 1.0 / kQtTiny, d = 1.0 / b, h = d;
        for (int i = 1; i <= kQtCfIter; ++i) {
            const double an = -(double)i * ((double)i - a);
            b += 2.0;
            d = an * d + b;
            if (fabs(d) < kQtTiny) d = kQtTiny;
            c = b + an / c;
            if (fabs(c) < kQtTiny) c = kQtTiny;
            d = 1.0 / d;
            const double del = d * c;
            h *= del;
            if (fabs(del - 1.0) < 1e-16) break;
        }
        Q = pre * h;
        P = 1.0 - Q;
    }
}

__device__ double beta_cf(double a, double b, double x) {
    const double qab = a + b, qap = a + 1.0, qam = a - 1.0;
    double c = 1.0, d = 1.0 - qab * x / qap;
    if (fabs(d) < kQtTiny) d = kQtTiny;
    d = 1.0 / d;
    double h = d;
    for (int m = 1; m <= kQtCfIter; ++m) {
        const double m2 = 2.0 * m;
        double aa = m * (b - m) * x / ((qam + m2) * (a + m2));
        d = 1.0 + aa * d;
        if (fabs(d) < kQtTiny) d = kQtTiny;
        c = 1.0 + aa / c;
        if (fabs(c) < kQtTiny) c = kQtTiny;
        d = 1.0 / d;
        h *= d * c;
        aa = -(a + m) * (qab + m) * x / ((a + m2) * (qap + m2));
        d = 1.0 + aa * d;
        if (fabs(d) < kQtTiny) d = kQtTiny;
        c = 1.0 + aa / c;
        if (fabs(c) < kQtTiny) c = kQtTiny;
        d = 1.0 / d;
        const double del = d * c;
        h *= del;
        if (fabs(del - 1.0) < 1e-16) break;
    }
    return h;
}

// I = I_x(a, b), Ic = 1 - I; xc = 1 - x and the two logarithms come from sig_terms
__device__ void beta_both(double a, double b, double x, double xc, double lx, double lxc, double &I, double &Ic) {
    const double pre = exp(lgamma(a + b) - lgamma(a) - lgamma(b) + a * lx + b * lxc);
    if (x < (a + 1.0) / (a + b + 2.0)) {
        I = pre * beta_cf(a, b, x) / a;
        Ic = 1.0 - I;
    } else {
        Ic = pre * beta_cf(b, a, xc) / b;
        I = 1.0 - Ic;
    }
}

struct CountEval {
    bool pois;
    double p0, mu, var; // p0: lambda or r
    __device__ void eval(double y, double &cdf, double &sf) const {
        if (y < 0.0) {
            cdf = 0.0, sf = 1.0;
            return;
        }
        if (var == 0.0) {
            const SigTerms t = sig_terms(mu);
            if (pois)
                gamma_pq(y + 1.0, p0 * t.sig, log(p0) + t.lsp, sf, cdf);
            else
                beta_both(p0, y + 1.0, t.sgc, t.sig, t.lsn, t.lsp, cdf, sf);
            return;
        }
        const double A = y + 1.0, B = pois ? 1.0 : p0, L = pois ? p0 : 0.0;
        const CountLik lik{A, B, L};
        const double c0 = pois ? A * log(p0) - lgamma(A) : lgamma(A + p0) - lgamma(A) - lgamma(p0);
        const double S = A + B + L, sg = 2.0 * A / (S + sqrt(S * S - 4.0 * L * A)), fs = log(sg) - log1p(-sg);
        double l, d1, d2;
        lik.eval(fs, l, d1, d2);
        const double w = d2 < 0.0 ? fmin(1.0 / sqrt(-d2), 1.0) : 1.0, H = 0.5 * w;
        double fL = fs - w, fR = fs + w, step = w;
        for (int it = 0; it < 64; ++it) {
            fL = fs - step;
            if (lik.lp(fL) < l - kQtCountDrop) break;
            step *= 2.0;
        }
        step = w;
        for (int it = 0; it < 64; ++it) {
            fR = fs + step;
            if (lik.lp(fR) < l - kQtCountDrop) break;
            step *= 2.0;
        }
        const double s = sqrt(var), is = 1.0 / s, inLo = mu - kQtInner * s, inHi = mu + kQtInner * s;
        double f = fL, jp = 0.0, jm = 0.0;
        for (int pn = 0; pn < kQtPanels && f < fR; ++pn) {
            double Hp = fmax(H, 0.1 * fabs(f - fs));
            if (fabs(f) < 50.0) Hp = fmin(Hp, 1.0);
            if (f < inLo) {
                if (f + Hp > inLo) Hp = inLo - f;
            } else if (f < inHi) {
                Hp = fmin(Hp, s);
                if (f + Hp > inHi) Hp = inHi - f;
            }
            Hp = fmin(Hp, fR - f);
            if (!(f + Hp > f)) {
                f = nextafter(f, INFINITY);
                continue;
            }
            const double c = f + 0.5 * Hp, hh = 0.5 * Hp;
            double ap = 0.0, am = 0.0;
            for (int q = 0; q < 16; ++q) {
                const double ff = q < 8 ? c - hh * kGlX[q] : c + hh * kGlX[q - 8], wq = kGlW[q & 7];
                const double e = wq * exp(lik.lp(ff) + c0), z = (ff - mu) * is, ts = 0.5 * erfc(fabs(z) * agpl::kSqrtHalf);
                ap += e * (z >= 0.0 ? 1.0 - ts : ts);
                am += e * (z >= 0.0 ? ts : 1.0 - ts);
            }
            jp += hh * ap;
            jm += hh * am;
            f += Hp;
        }
        double P = 0.0, Q = 0.0;
        if (pois) gamma_pq(A, p0, log(p0), P, Q);
        cdf = Q + jp;
        sf = jm;
    }
};

// the smallest integer y with F(y) >= p, on the tail that p is in: doubling from 0, then integer bisection
__device__ double count_quantile(const CountEval &ev, double p) {
    if (!(p > 0.0 && p < 1.0)) return NAN;
    const bool lower = p <= 0.5;
    double c, s, lo = -1.0, hi = 0.0;
    for (int it = 0; it < 33; ++it) {
        ev.eval(hi, c, s);
        if (lower ? c >= p : s <= 1.0 - p) break;
        lo = hi;
        hi = hi == 0.0 ? 1.0 : 2.0 * hi;
    }
    while (hi - lo > 1.0) {
        const double mid = floor(0.5 * (lo + hi));
        ev.eval(mid, c, s);
        if (lower ? c >= p : s <= 1.0 - p)
            hi = mid;
        else
            lo = mid;
    }
    return hi;
}

// Binomial(n, sigma(f)): given f, F(y | f) = I_{sigma(-f)}(n - y, y + 1) for 0 <= y < n -- the negative binomial's distribution function
// at the same y with r = n - y, so both tails take that route unchanged; P(Y <= y) = 1 and P(Y > y) = 0 exactly for y >= n.
struct BinomialEval {
    double nt, mu, var;
    __device__ void eval(double y, double &cdf, double &sf) const {
        if (y >= nt)
            cdf = 1.0, sf = 0.0;
        else {
            CountEval{false, nt - y, mu, var}.eval(y, cdf, sf); // (y < 0: 0 and 1)
            // a tail that is 1 to rounding comes out of the panels' sum as 1 + a few ulp: a probability is at most 1
            cdf = fmin(cdf, 1.0), sf = fmin(sf, 1.0);
        }
    }
};
// the smallest integer y with F(y) >= p, on the tail that p is in: integer bisection of [0, n] (F(n) = 1)
__device__ double binomial_quantile(const BinomialEval &ev, double p) {
    if (!(p > 0.0 && p < 1.0)) return NAN;
    const bool lower = p <= 0.5;
    double c, s, lo = -1.0, hi = ev.nt;
    while (hi - lo > 1.0) {
        const double mid = floor(0.5 * (lo + hi));
        ev.eval(mid, c, s);
        if (lower ? c >= p : s <= 1.0 - p)
            hi = mid;
        else
            lo = mid;
    }
    return hi;
}

// inf { y : F(y) >= p } of a continuous predictive.  The residual is taken on the tail that p is in (cdf - p for p <= 1/2,
// (1 - p) - sf above) and increases in y.  The bracket grows by doubling from loc on the side the residual points to; then Newton
// steps on the logarithm of the tail (a power-law tail is nearly linear in it), bisection where a step leaves the bracket.
template <class E>
__device__ double solve_quantile(const E &ev, double p, double loc, double sc) {
    if (!(p > 0.0 && p < 1.0)) return NAN;
    const bool lower = p <= 0.5;
    const double tgt = lower ? p : 1.0 - p;
    double c, s, dens, y = loc;
    ev.template eval<true>(y, c, s, dens);
    double g = lower ? c : s, r = lower ? g - tgt : tgt - g;
    if (r == 0.0) return y;
    double lo = y, hi = y, step = r < 0.0 ? sc : -sc;
    for (int it = 0; it < kQtDouble; ++it) {
        const bool up = step > 0.0;
        y = loc + step;
        ev.template eval<true>(y, c, s, dens);
        g = lower ? c : s;
        r = lower ? g - tgt : tgt - g;
        if (up ? r >= 0.0 : r <= 0.0) {
            (up ? hi : lo) = y;
            break;
        }
        (up ? lo : hi) = y;
        step *= 2.0;
    }
    for (int it = 0; it < kQtSteps; ++it) {
        if (fabs(r) <= kQtTol) break;
        if (r < 0.0)
            lo = y;
        else
            hi = y;
        if (hi <= nextafter(nextafter(lo, INFINITY), INFINITY)) break;
        double t = g > 0.0 && dens > 0.0 ? y - (lower ? 1.0 : -1.0) * g * log(g / tgt) / dens : NAN;
        if (!(lo < t && t < hi)) t = lo + 0.5 * (hi - lo);
        y = t;
        ev.template eval<true>(y, c, s, dens);
        g = lower ? c : s;
        r = lower ? g - tgt : tgt - g;
    }
    return y;
}

__device__ __forceinline__ void point_of(int kind, const double *__restrict__ mu, const double *__restrict__ var, int64_t i, double &m,
                                         double &v, double &mg, double &vg, bool &bad) {
    mg = vg = 0.0;
    if (kind == AGPL_LIK_HETEROGAUSS) {
        m = mu[2 * i], v = var[2 * i], mg = mu[2 * i + 1], vg = var[2 * i + 1];
        bad = bad_marginal(m, v) || bad_marginal(mg, vg);
    } else {
        m = mu[i], v = var[i];
        bad = bad_marginal(m, v);
    }
}

// E sigma(f) at (mu, var): the predictive's rule, the logistic itself at var = 0
__device__ double mean_sigma(double mu, double var) {
    if (var == 0.0) return sig_terms(mu).sig;
    double e1, e2;
    sigma_moments(mu, var, e1, e2);
    return e1;
}

template <class E>
__device__ void cdf_at(const E &ev, double y, double &c, double &s) {
    double dens;
    if (isnan(y))
        c = s = NAN;
    else if (isinf(y))
        c = y > 0.0 ? 1.0 : 0.0, s = 1.0 - c;
    else
        ev.template eval<false>(y, c, s, dens);
}

template <int KIND>
__global__ __launch_bounds__(kBlock) void cdf_kernel(double p0, StRule rule, int64_t n, const double *__restrict__ mu,
                                                     const double *__restrict__ var, const void *__restrict__ yv,
                                                     double *__restrict__ cdf_out, double *__restrict__ sf_out) {
    const double *tw = nullptr, *tu = nullptr;
    if constexpr (KIND == AGPL_LIK_STUDENTT) {
        __shared__ double stw[kQtNodes], stu[kQtNodes];
        st_tables(rule, stw, stu);
        tw = stw, tu = stu;
    }
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (int64_t)gridDim.x * kBlock) {
        double m, v, mg, vg, c = NAN, s = NAN;
        bool bad;
        point_of(KIND, mu, var, i, m, v, mg, vg, bad);
        if (!bad) {
            if constexpr (KIND == AGPL_LIK_BERNOULLI_LOGISTIC) {
                const bool one = ((const uint8_t *)yv)[i] != 0;
                c = one ? 1.0 : mean_sigma(-m, v);
                s = one ? 0.0 : mean_sigma(m, v);
            } else if constexpr (KIND == AGPL_LIK_POISSON || KIND == AGPL_LIK_NEGBINOMIAL) {
                CountEval{KIND == AGPL_LIK_POISSON, p0, m, v}.eval((double)((const int32_t *)yv)[i], c, s);
            } else if constexpr (KIND == AGPL_LIK_BINOMIAL) {
                BinomialEval{p0, m, v}.eval((double)((const int32_t *)yv)[i], c, s);
            } else if constexpr (KIND == AGPL_LIK_BINOMIAL_N) { // the point's own trials: y [N][2], NaN outside 1 <= n < 2^22
                const double nt = agpl::binomial_trials<double>((double)((const int32_t *)yv)[2 * i + 1]);
                if (nt == nt) BinomialEval{nt, m, v}.eval((double)((const int32_t *)yv)[2 * i], c, s);
            } else {
                const double y = ((const double *)yv)[i];
                if constexpr (KIND == AGPL_LIK_STUDENTT)
                    cdf_at(StEval{tw, tu, rule.cnt, m, v}, y, c, s);
                else if constexpr (KIND == AGPL_LIK_LAPLACE)
                    cdf_at(LapEval{p0, m, v}, y, c, s);
                else if constexpr (KIND == AGPL_LIK_ASYMLAPLACE)
                    cdf_at(AldEval{p0, rule.a, m, v}, y, c, s); // (tau: check_call)
                else if constexpr (KIND == AGPL_LIK_LOGISTIC_NOISE)
                    cdf_at(LnEval{p0, m, v}, y, c, s);
                else
                    cdf_at(HetEval(m, v, mg, vg, p0), y, c, s);
            }
        }
        if (cdf_out) cdf_out[i] = c;
        if (sf_out) sf_out[i] = s;
    }
}

template <int KIND>
__global__ __launch_bounds__(kBlock) void quantile_kernel(double p0, double p1, StRule rule, int64_t n, const double *__restrict__ mu,
                                                          const double *__restrict__ var, int nq, const double *__restrict__ probs,
                                                          double *__restrict__ q_out) {
    const double *tw = nullptr, *tu = nullptr;
    if constexpr (KIND == AGPL_LIK_STUDENTT) {
        __shared__ double stw[kQtNodes], stu[kQtNodes];
        st_tables(rule, stw, stu);
        tw = stw, tu = stu;
    }
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (int64_t)gridDim.x * kBlock) {
        double m, v, mg, vg;
        bool bad;
        point_of(KIND, mu, var, i, m, v, mg, vg, bad);
        double c0 = 0.0; // Bernoulli: cdf(0), once per point
        if (KIND == AGPL_LIK_BERNOULLI_LOGISTIC && !bad) c0 = mean_sigma(-m, v);
        for (int j = 0; j < nq; ++j) {
            const double p = probs[j];
            double q = NAN;
            if (!bad) {
                if constexpr (KIND == AGPL_LIK_BERNOULLI_LOGISTIC)
                    q = p > 0.0 && p < 1.0 ? (p <= c0 ? 0.0 : 1.0) : NAN;
                else if constexpr (KIND == AGPL_LIK_POISSON || KIND == AGPL_LIK_NEGBINOMIAL)
                    q = count_quantile(CountEval{KIND == AGPL_LIK_POISSON, p0, m, v}, p);
                else if constexpr (KIND == AGPL_LIK_BINOMIAL)
                    q = binomial_quantile(BinomialEval{p0, m, v}, p);
                else if constexpr (KIND == AGPL_LIK_STUDENTT)
                    q = solve_quantile(StEval{tw, tu, rule.cnt, m, v}, p, m, sqrt(v + p1 * p1));
                else if constexpr (KIND == AGPL_LIK_LAPLACE)
                    q = solve_quantile(LapEval{p0, m, v}, p, m, sqrt(v + 2.0 * p0 * p0));
                else if constexpr (KIND == AGPL_LIK_ASYMLAPLACE) // (the scale: the predictive's standard deviation, as above)
                    q = solve_quantile(AldEval{p0, p1, m, v}, p, m,
                                       sqrt(v + p0 * p0 * (1.0 - 2.0 * p1 + 2.0 * p1 * p1) / (p1 * (1.0 - p1) * p1 * (1.0 - p1))));
                else if constexpr (KIND == AGPL_LIK_LOGISTIC_NOISE)
                    q = solve_quantile(LnEval{p0, m, v}, p, m, sqrt(v + p0 * p0 * (agpl::kPi * agpl::kPi / 3.0)));
                else
                    q = solve_quantile(HetEval(m, v, mg, vg, p0), p, m, sqrt(v + (1.0 + exp(-mg + 0.5 * vg)) / p0));
            }
            q_out[i * nq + j] = q;
        }
    }
}

// the checks that both entry points share; *rule is filled for the Student-t kind
int32_t check_call(agpl_ctx *ctx, const agpl_lik_desc *lik, int64_t n, StRule *rule) {
    AGPL_LIK_CHECK(ctx, lik);
    if (lik_is_categorical(lik->kind))
        AGPL_FAIL(ctx, AGPL_ERR_INVALID_ARGUMENT, "the classes of a categorical likelihood have no order: no distribution function");
    if (n < 0) AGPL_FAIL(ctx, AGPL_ERR_INVALID_ARGUMENT, "n = %lld < 0", (long long)n);
    const double p0 = lik->p[0], p1 = lik->p[1];
    if (lik->kind == AGPL_LIK_STUDENTT && p0 < kQtMinNu)
        AGPL_FAIL(ctx, AGPL_ERR_INVALID_ARGUMENT, "StudentT nu = %g: the rule's %d nodes hold nu >= %g", p0, kQtNodes, kQtMinNu);
    *rule = lik->kind == AGPL_LIK_STUDENTT ? st_rule(p0, p1) : StRule{};
    if (lik->kind == AGPL_LIK_ASYMLAPLACE) rule->a = p1; // cdf_kernel takes p0 alone: tau rides the first slot of the rule, which only Student-t reads
    return AGPL_OK;
}

unsigned blocks_for(int64_t n) {
    const int64_t want = agpl_cdiv(n, kBlock);
    return (unsigned)(want < kQtBlocks ? want : kQtBlocks);
}

} // namespace

extern "C" AGPL_API int32_t agpl_predictive_cdf(agpl_ctx *ctx, const agpl_lik_desc *lik, int64_t n, const double *mu, const double *var,
                                                const void *y, double *cdf_out, double *sf_out) {
    if (!ctx) return AGPL_ERR_INVALID_ARGUMENT;
    StRule rule;
    const int32_t rc = check_call(ctx, lik, n, &rule);
    if (rc != AGPL_OK) return rc;
    if (!cdf_out && !sf_out) AGPL_FAIL(ctx, AGPL_ERR_INVALID_ARGUMENT, "cdf_out and sf_out are both null");
    if (n == 0) return AGPL_OK;
    if (!mu || !var || !y) AGPL_FAIL(ctx, AGPL_ERR_INVALID_ARGUMENT, "null mu / var / y");
    const double p0 = lik->p[0];
    const bool launched = agpl::lik_switch(lik->kind, [&](auto K) {
        constexpr bool taken = !lik_is_categorical(K()); // (the categorical kinds: refused by check_call)
        if constexpr (taken) cdf_kernel<K()><<<blocks_for(n), kBlock, 0, ctx->stream>>>(p0, rule, n, mu, var, y, cdf_out, sf_out);
        return taken;
    });
    if (!launched) AGPL_FAIL(ctx, AGPL_ERR_INVALID_ARGUMENT, "agpl_predictive_cdf: no kernel for likelihood kind %d", lik->kind);
    AGPL_LAUNCH_CHECK(ctx);
    return AGPL_OK;
}

extern "C" AGPL_API int32_t agpl_predictive_quantile(agpl_ctx *ctx, const agpl_lik_desc *lik, int64_t n, const double *mu,
                                                     const double *var, int32_t nq, const double *probs, double *q_out) {
    if (!ctx) return AGPL_ERR_INVALID_ARGUMENT;
    StRule rule;
    const int32_t rc = check_call(ctx, lik, n, &rule);
    if (rc != AGPL_OK) return rc;
    if (lik->kind == AGPL_LIK_BINOMIAL_N)
        AGPL_FAIL(ctx, AGPL_ERR_INVALID_ARGUMENT,
                  "the per-point Binomial's quantiles need the trials n_i, which agpl_predictive_quantile has no argument for: "
                  "bisect agpl_predictive_cdf, or call with AGPL_LIK_BINOMIAL per group of equal n");
    if (nq < 1 || nq > kQtMaxProbs) AGPL_FAIL(ctx, AGPL_ERR_INVALID_ARGUMENT, "nq = %d: a call takes 1 .. %d probs", nq, kQtMaxProbs);
    if (n == 0) return AGPL_OK;
    if (!mu || !var || !probs || !q_out) AGPL_FAIL(ctx, AGPL_ERR_INVALID_ARGUMENT, "null mu / var / probs / q_out");
    const double p0 = lik->p[0], p1 = lik->p[1];
    const bool launched = agpl::lik_switch(lik->kind, [&](auto K) {
        constexpr bool taken = !lik_is_categorical(K()) && K() != AGPL_LIK_BINOMIAL_N; // (refused by check_call, and above)
        if constexpr (taken) quantile_kernel<K()><<<blocks_for(n), kBlock, 0, ctx->stream>>>(p0, p1, rule, n, mu, var, nq, probs, q_out);
        return taken;
    });
    if (!launched) AGPL_FAIL(ctx, AGPL_ERR_INVALID_ARGUMENT, "agpl_predictive_quantile: no kernel for likelihood kind %d", lik->kind);
    AGPL_LAUNCH_CHECK(ctx);
    return AGPL_OK;
}
