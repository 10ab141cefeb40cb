// agpl_likgrad.hip -- libagpl_likgrad.so (include/agpl_likgrad.h): E_{q(f)} log p(y | f; theta) per point, its derivatives for the
// logarithms of the likelihood's parameters, and their deterministic sums.  float64, one lane per point; the rules and their
// measured errors are in DESIGN.md 4.21.  Compiled without fused-multiply-add contraction, like agpl_predictive.hip.
#include <math.h>

#include "../../include/agpl_likgrad.h"
#include "agpl_common.h"
#include "agpl_digamma.h"
#include "agpl_logistic_noise.h"
#include "agpl_random.h"

namespace {

constexpr int kBlock = 512;     // lanes per workgroup
constexpr int kMaxBlocks = 256; // workgroups of one launch: 1 + P <= 3 partial sums each in ctx->elbo_part (1024 doubles)
constexpr int kMaxTerms = 3;    // ell and at most two derivatives
constexpr int kMaxHalf = 2048;  // nodes on each side of mu in a trapezoid rule, at most
constexpr double kSpan = 8.0;
constexpr double kSinhStep = 0.19634954084936207; // pi / 16: the largest spacing in x of the Student-t rule above the node limit
constexpr double kSinhDensity = 0.5;              // its spacing is kSinhDensity / (|y - mu| / s + kSinhPad) where that is smaller
constexpr double kSinhPad = 4.0;
constexpr int kSinhMax = 1024;                    // its intervals, at most
constexpr double kLn2 = 0.69314718055994530942;
constexpr double kLogSqrt2Pi = 0.91893853320467274178;
constexpr double kSqrt2OverPi = 0.79788456080286535588;

static_assert(kMaxBlocks * kMaxTerms <= 1024, "the partial sums must fit the context's 1024 doubles");

// The trapezoid rule over mu +- 8 s for an integrand whose nearest complex singularity lies `a` from the real axis: spacing
// min(s / 4, a / 4) (the error falls as exp(-2 pi a / spacing); s / 4 integrates the Gaussian weight itself to rounding), nh
// nodes on each side of mu; beyond kMaxHalf nodes the spacing widens to 8 s / kMaxHalf (include/agpl_likgrad.h says so).
struct Rule {
    double h;
    int nh;
};
__device__ __forceinline__ Rule make_rule(double s, double a) {
    Rule r;
    r.h = 0.25 * fmin(s, a);
    const double want = ceil(kSpan * s / r.h);
    if (want > (double)kMaxHalf) {
        r.nh = kMaxHalf;
        r.h = kSpan * s / (double)kMaxHalf;
    } else {
        r.nh = (int)want;
    }
    return r;
}
// whether make_rule(s, a) widens the spacing (the same expression, so the same decision).  The logistic terms never get there on
// the supported domain (s / pi <= 16); the Student-t terms then take the sinh rule below.
__device__ __forceinline__ bool rule_is_capped(double s, double a) { return ceil(kSpan * s / (0.25 * fmin(s, a))) > (double)kMaxHalf; }

// E log sigma(f), E log sigma(-f), E sigma(f) under N(mu, var); var = 0: the values at mu
struct LogisticE {
    double lsp, lsn, sig;
};
__device__ __forceinline__ LogisticE logistic_at(double f) {
    const double e = exp(-fabs(f)), sp = 1.0 / (1.0 + e), l1p = log1p(e);
    LogisticE o;
    const bool pos = f >= 0.0;
    o.sig = pos ? sp : e * sp;
    o.lsp = pos ? -l1p : f - l1p;
    o.lsn = pos ? -f - l1p : -l1p;
    return o;
}
__device__ LogisticE logistic_expectations(double mu, double var) {
    if (var == 0.0) return logistic_at(mu);
    const double s = sqrt(var);
    const Rule r = make_rule(s, agpl::kPi);
    const double hs = r.h / s;
    double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
    for (int j = -r.nh; j <= r.nh; ++j) {
        const double x = (double)j * hs, w = exp(-0.5 * x * x);
        const LogisticE t = logistic_at(mu + (double)j * r.h);
        a0 += w;
        a1 += w * t.lsp;
        a2 += w * t.lsn;
        a3 += w * t.sig;
    }
    LogisticE o;
    o.lsp = a1 / a0;
    o.lsn = a2 / a0;
    o.sig = a3 / a0;
    return o;
}

// Logistic noise (agpl.h) at the standardised residual m = (y - mu) / s and spread R^2 = var / s^2, g ~ N(m, R^2):
//     lse = E[log sigma(g) + log sigma(-g)],  dls = E[g tanh(g / 2)] = m (2 e1 - 1) + 2 R^2 (e1 - e2)  (Stein's lemma),
// e1 = E sigma(g), e2 = E sigma(g)^2.  Below R = kLnSwitch = 1 the rule of logistic_expectations (the same nodes and weights, R / 4 apart, with
// sigma(g) sigma(-g) beside its three sums); from there the rule over the noise's own measure (agpl_logistic_noise.h), taken at
// -|m| (both results are even in m), where lse = -(|m| + 2 R E G(z)) is a sum of terms of one sign.
struct LogisticNoiseE {
    double lse, dls;
};
__device__ LogisticNoiseE logistic_noise_expectations(double m, double R2) {
    const double am = fabs(m);
    if (R2 == 0.0) {
        const double e = exp(-am), l1p = log1p(e);
        return LogisticNoiseE{-am - 2.0 * l1p, am * ((1.0 - e) / (1.0 + e))};
    }
    const double R = sqrt(R2);
    if (R >= agpl::kLnSwitch) {
        const agpl::LnSums r = agpl::ln_noise_rule<true>(-am, R);
        return LogisticNoiseE{-(am + 2.0 * R * r.g), am * (r.hi - r.lo) + 2.0 * R * r.phi};
    }
    const Rule r = make_rule(R, agpl::kPi);
    const double hs = r.h / R;
    double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
    for (int j = -r.nh; j <= r.nh; ++j) {
        const double x = (double)j * hs, w = exp(-0.5 * x * x);
        const double f = m + (double)j * r.h, af = fabs(f), e = exp(-af), sp = 1.0 / (1.0 + e);
        a0 += w;
        a1 += w * (-af - 2.0 * log1p(e));
        a2 += w * copysign((1.0 - e) * sp, f); // tanh(f / 2) = 2 sigma(f) - 1
        a3 += w * (e * sp * sp);               // sigma(f) sigma(-f)
    }
    return LogisticNoiseE{a1 / a0, m * (a2 / a0) + 2.0 * R2 * (a3 / a0)};
}

// The Student-t terms above the node limit (s / a > 64), where the widened spacing would not resolve the peak of width a at f = y,
// with that peak inside mu +- 8 s: the rule runs in x, y - f = a sinh x.  Then log1p(u) = 2 log cosh x and u / (1 + u) = tanh^2 x
// (singular at x = +- i pi / 2 whatever s / a is), the weight is N(a sinh x; d, s^2) cosh x, the nodes are x = j hx between
// asinh((d -+ 8 s) / a), and the sums are normalised by the rule's own weights.  The weight varies in x on the scale
// 1 / |d / s - z| at z standard deviations from mu, hence the spacing min(pi / 16, 1 / (2 (|d| / s + 4))): at most 24 ln(32 s / a)
// nodes, a few hundred.  Not inlined, so that the loop below the limit stays the code it was, and its two results returned by value:
// by reference they would have to live in memory, 32 bytes of scratch per lane.
struct StudentTE {
    double elog, efrac;
};
__device__ __noinline__ StudentTE studentt_sinh_rule(double a, double d, double s) {
    const double ia = 1.0 / a, is = 1.0 / s;
    double hx = fmin(kSinhStep, kSinhDensity / (fabs(d) * is + kSinhPad));
    const double xlo = asinh((d - kSpan * s) * ia), xhi = asinh((d + kSpan * s) * ia);
    if (xhi - xlo > hx * (double)kSinhMax) hx = (xhi - xlo) / (double)kSinhMax;
    if (!isfinite(hx)) return StudentTE{NAN, NAN}; // 16 s / a overflows (a denormal a): no rule, and no undefined cast below
    const int jhi = (int)floor(xhi / hx);
    double a0 = 0.0, a1 = 0.0, a3 = 0.0;
    for (int j = (int)ceil(xlo / hx); j <= jhi; ++j) {
        const double x = (double)j * hx, ax = fabs(x), e = exp(ax), ie = 1.0 / e;
        const double sh = copysign(0.5 * (e - ie), x), ch = 0.5 * (e + ie);
        const double q = (d - a * sh) * is, w = exp(-0.5 * q * q) * ch, th = sh / ch;
        a0 += w;
        a1 += w * (2.0 * (ax + log1p(ie * ie) - kLn2));
        a3 += w * (th * th);
    }
    StudentTE o;
    o.elog = a1 / a0;
    o.efrac = a3 / a0;
    return o;
}

// E log1p(u), E u / (1 + u), u = (y - f)^2 / (nu sg^2), under N(mu, var): singularities at f = y +- i sg sqrt(nu) = y +- i a.
// Above the node limit the sinh rule serves where the peak lies inside mu +- 8 s; where it lies outside, it carries a weight below
// exp(-32) and the widened trapezoid rule is exact to rounding.  Where 16 s / a overflows (far outside the supported domain) the
// sinh rule's end points are not finite and it gives NaN.
__device__ void studentt_expectations(double nu, double sg, double y, double mu, double var, double &elog, double &efrac) {
    const double a2 = nu * sg * sg, d = y - mu;
    if (var == 0.0) {
        const double u = d * d / a2;
        elog = log1p(u);
        efrac = u / (1.0 + u);
        return;
    }
    const double s = sqrt(var);
    if (rule_is_capped(s, sqrt(a2)) && fabs(d) < kSpan * s) {
        const StudentTE e = studentt_sinh_rule(sqrt(a2), d, s);
        elog = e.elog;
        efrac = e.efrac;
        return;
    }
    const Rule r = make_rule(s, sqrt(a2));
    const double hs = r.h / s, ia2 = 1.0 / a2;
    double a0 = 0.0, a1 = 0.0, a3 = 0.0;
    for (int j = -r.nh; j <= r.nh; ++j) {
        const double x = (double)j * hs, w = exp(-0.5 * x * x);
        const double t = d - (double)j * r.h, u = t * t * ia2;
        a0 += w;
        a1 += w * log1p(u);
        a3 += w * (u / (1.0 + u));
    }
    elog = a1 / a0;
    efrac = a3 / a0;
}

// E|y - f| under N(mu, var), d = y - mu
__device__ __forceinline__ double expected_abs(double d, double var) {
    if (var == 0.0) return fabs(d);
    const double s = sqrt(var);
    return s * kSqrt2OverPi * exp(-0.5 * d * d / var) + d * erf(d / s * agpl::kSqrtHalf);
}

__device__ __forceinline__ bool bad_marginal(double mu, double var) { return !(isfinite(mu) && isfinite(var) && var >= 0.0); }

// the sums of this workgroup's per-lane values in a fixed order -> part[t * gridDim.x + blockIdx.x], t = 0 .. NT - 1
template <int NT>
__device__ void block_sums(const double (&v)[kMaxTerms], double *__restrict__ part) {
    __shared__ double red[kMaxTerms][kBlock];
    for (int t = 0; t < NT; ++t) red[t][threadIdx.x] = v[t];
    __syncthreads();
    for (int st = kBlock / 2; st > 0; st >>= 1) {
        if ((int)threadIdx.x < st)
            for (int t = 0; t < NT; ++t) red[t][threadIdx.x] += red[t][threadIdx.x + st];
        __syncthreads();
    }
    if ((int)threadIdx.x < NT) part[(int)threadIdx.x * (int)gridDim.x + (int)blockIdx.x] = red[threadIdx.x][0];
}

template <int KIND>
__global__ __launch_bounds__(kBlock) void expected_loglik_kernel(double p0, double p1, int64_t n, const double *__restrict__ mu,
                                                                 const double *__restrict__ var, const void *__restrict__ yv,
                                                                 double *__restrict__ ell_out, double *__restrict__ dell_out,
                                                                 double *__restrict__ part) {
    constexpr int P = agpl_lik_nparams(KIND);
    // constants of the kind (functions of the parameters alone)
    double c0 = 0.0, c1 = 0.0;
    if (KIND == AGPL_LIK_NEGBINOMIAL) {
        c0 = lgamma(p0);
        c1 = agpl::digamma(p0);
    } else if (KIND == AGPL_LIK_STUDENTT) {
        c0 = lgamma(0.5 * (p0 + 1.0)) - lgamma(0.5 * p0) - 0.5 * log(p0 * agpl::kPi) - log(p1);
        c1 = 0.5 * agpl::digamma(0.5 * (p0 + 1.0)) - 0.5 * agpl::digamma(0.5 * p0) - 0.5 / p0;
    } else if (KIND == AGPL_LIK_POISSON) {
        c0 = log(p0);
    } else if (KIND == AGPL_LIK_LAPLACE) {
        c0 = log(2.0 * p0);
    } else if (KIND == AGPL_LIK_ASYMLAPLACE) { // p0 = sigma, p1 = tau
        c0 = log(p1 * (1.0 - p1) / p0);
        c1 = (p1 - 0.5) / p0;
    } else if (KIND == AGPL_LIK_LOGISTIC_NOISE) {
        c0 = log(p0);
    } else if (KIND == AGPL_LIK_HETEROGAUSS) {
        c0 = 0.5 * log(p0) - kLogSqrt2Pi;
    }
    double sums[kMaxTerms] = {0.0, 0.0, 0.0}; // this lane's ell and derivatives, points in ascending order
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (int64_t)gridDim.x * kBlock) {
        double m, v, mg = 0.0, vg = 0.0;
        bool bad;
        if (KIND == AGPL_LIK_HETEROGAUSS) {
            m = mu[2 * i], v = var[2 * i], mg = mu[2 * i + 1], vg = var[2 * i + 1];
            bad = bad_marginal(m, v) || bad_marginal(mg, vg);
        } else {
            m = mu[i], v = var[i];
            bad = bad_marginal(m, v);
        }
        double ell = NAN, d0 = NAN, d1 = NAN;
        if (!bad) {
            if (KIND == AGPL_LIK_BERNOULLI_LOGISTIC) {
                const LogisticE e = logistic_expectations(m, v);
                ell = ((const uint8_t *)yv)[i] ? e.lsp : e.lsn;
            } else if (KIND == AGPL_LIK_NEGBINOMIAL) {
                const double y = (double)((const int32_t *)yv)[i];
                if (y < 0.0) {
                    ell = -INFINITY;
                } else {
                    const LogisticE e = logistic_expectations(m, v);
                    ell = lgamma(y + p0) - lgamma(y + 1.0) - c0 + y * e.lsp + p0 * e.lsn;
                    d0 = p0 * (agpl::digamma(y + p0) - c1 + e.lsn);
                }
            } else if (KIND == AGPL_LIK_BINOMIAL || KIND == AGPL_LIK_BINOMIAL_N) { // log C(n, y) + y E log sigma(f) + (n - y) E log sigma(-f)
                // n = p0 for kind 8; the point's own trials (y [N][2], column 1; NaN outside 1 <= n < 2^22) for kind 11
                const int32_t *yi = (const int32_t *)yv;
                const double y = (double)(KIND == AGPL_LIK_BINOMIAL ? yi[i] : yi[2 * i]);
                const double nt = KIND == AGPL_LIK_BINOMIAL ? p0 : agpl::binomial_trials<double>((double)yi[2 * i + 1]);
                if (KIND == AGPL_LIK_BINOMIAL_N && nt != nt) {
                    ell = NAN;
                } else if (y < 0.0 || y > nt) {
                    ell = -INFINITY;
                } else {
                    const LogisticE e = logistic_expectations(m, v);
                    ell = lgamma(nt + 1.0) - lgamma(y + 1.0) - lgamma(nt - y + 1.0) + y * e.lsp + (nt - y) * e.lsn;
                }
            } else if (KIND == AGPL_LIK_POISSON) {
                const double y = (double)((const int32_t *)yv)[i];
                if (y < 0.0) {
                    ell = -INFINITY;
                } else {
                    const LogisticE e = logistic_expectations(m, v);
                    ell = y * (c0 + e.lsp) - p0 * e.sig - lgamma(y + 1.0);
                    d0 = y - p0 * e.sig;
                }
            } else if (KIND == AGPL_LIK_STUDENTT) {
                double elog, efrac;
                studentt_expectations(p0, p1, ((const double *)yv)[i], m, v, elog, efrac);
                ell = c0 - 0.5 * (p0 + 1.0) * elog;
                d0 = p0 * (c1 - 0.5 * elog + 0.5 * (p0 + 1.0) * efrac / p0);
                d1 = -1.0 + (p0 + 1.0) * efrac;
            } else if (KIND == AGPL_LIK_LAPLACE) {
                // y = +-inf gives ea = +inf, so ell = -inf, and 0 * ea = NaN makes the derivative NaN; y = NaN gives NaN in both.  No
                // branch and no select: this kernel sits at the 80 registers of six waves per SIMD.
                const double ea = expected_abs(((const double *)yv)[i] - m, v) / p0;
                ell = -ea - c0;
                d0 = -1.0 + ea + 0.0 * ea;
            } else if (KIND == AGPL_LIK_ASYMLAPLACE) { // E of the pinball loss = E|y - f| / (2 sigma) + (tau - 1/2) (y - mu) / sigma
                const double d = ((const double *)yv)[i] - m;
                const double ea = expected_abs(d, v) / (2.0 * p0), lin = c1 * d;
                ell = c0 - ea - lin;
                d0 = -1.0 + ea + lin;
            } else if (KIND == AGPL_LIK_LOGISTIC_NOISE) { // p0 = the scale s: -log s + E log sigma(g) + E log sigma(-g)
                const LogisticNoiseE e = logistic_noise_expectations((((const double *)yv)[i] - m) / p0, v / (p0 * p0));
                ell = e.lse - c0;
                d0 = -1.0 + e.dls;
            } else {
                const double d = ((const double *)yv)[i] - m;
                const LogisticE e = logistic_expectations(mg, vg);
                const double q = 0.5 * p0 * e.sig * (d * d + v);
                ell = c0 + 0.5 * e.lsp - q;
                d0 = 0.5 - q;
            }
            if (KIND == AGPL_LIK_STUDENTT || KIND == AGPL_LIK_HETEROGAUSS || KIND == AGPL_LIK_ASYMLAPLACE ||
                KIND == AGPL_LIK_LOGISTIC_NOISE) {
                // a non-finite real y, after the fact (the rules above are bounded whatever y is; the asymmetric Laplace kind's two
                // terms are infinities of either sign, and this is what the Laplace kind gives): the convention of a count y < 0
                const double y = ((const double *)yv)[i];
                if (!isfinite(y)) {
                    ell = isnan(y) ? NAN : -INFINITY;
                    d0 = d1 = NAN;
                }
            }
        }
        if (ell_out) ell_out[i] = ell;
        sums[0] += ell;
        if (P >= 1) {
            if (dell_out) dell_out[i * P] = d0;
            sums[1] += d0;
        }
        if (P >= 2) {
            if (dell_out) dell_out[i * P + 1] = d1;
            sums[2] += d1;
        }
    }
    if (part) block_sums<1 + P>(sums, part);
}

// second level: workgroup t sums part[t * nblk ..] in a fixed order -> ell_sum (t = 0) or grad_sum[t - 1]; a NULL output is skipped
__global__ __launch_bounds__(kMaxBlocks) void likgrad_sum_kernel(const double *__restrict__ part, int nblk, double *__restrict__ ell_sum,
                                                                 double *__restrict__ grad_sum) {
    __shared__ double red[kMaxBlocks];
    const int t = blockIdx.x;
    red[threadIdx.x] = (int)threadIdx.x < nblk ? part[t * nblk + (int)threadIdx.x] : 0.0;
    __syncthreads();
    for (int st = kMaxBlocks / 2; st > 0; st >>= 1) {
        if ((int)threadIdx.x < st) red[threadIdx.x] += red[threadIdx.x + st];
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        if (t == 0) {
            if (ell_sum) *ell_sum = red[0];
        } else if (grad_sum) {
            grad_sum[t - 1] = red[0];
        }
    }
}

} // namespace

extern "C" AGPL_API int32_t agpl_expected_loglik(agpl_ctx *ctx, const agpl_lik_desc *lik, int64_t n, const double *mu, const double *var,
                                                 const void *y, double *ell_out, double *dell_out, double *ell_sum, double *grad_sum) {
    if (!ctx) return AGPL_ERR_INVALID_ARGUMENT;
    AGPL_LIK_CHECK(ctx, lik);
    if (lik_is_categorical(lik->kind))
        AGPL_FAIL(ctx, AGPL_ERR_INVALID_ARGUMENT, "agpl_expected_loglik does not take the categorical kinds (their expectation couples the latents)");
    if (n < 0) AGPL_FAIL(ctx, AGPL_ERR_INVALID_ARGUMENT, "n = %lld < 0", (long long)n);
    const double p0 = lik->p[0], p1 = lik->p[1];
    if (lik->kind == AGPL_LIK_BERNOULLI_LOGISTIC && (dell_out || grad_sum))
        AGPL_FAIL(ctx, AGPL_ERR_INVALID_ARGUMENT, "the Bernoulli likelihood has no parameter: dell_out / grad_sum must be NULL");
    if ((lik->kind == AGPL_LIK_BINOMIAL || lik->kind == AGPL_LIK_BINOMIAL_N) && (dell_out || grad_sum))
        AGPL_FAIL(ctx, AGPL_ERR_INVALID_ARGUMENT, "the Binomial likelihood has no learnable parameter: dell_out / grad_sum must be NULL");
    const int P = agpl_lik_nparams(lik->kind);
    if (n == 0) {
        if (ell_sum) AGPL_HIP(ctx, hipMemsetAsync(ell_sum, 0, sizeof(double), ctx->stream));
        if (grad_sum) AGPL_HIP(ctx, hipMemsetAsync(grad_sum, 0, sizeof(double) * P, ctx->stream));
        return AGPL_OK;
    }
    if (!mu || !var || !y) AGPL_FAIL(ctx, AGPL_ERR_INVALID_ARGUMENT, "null mu / var / y");
    if (!ell_out && !dell_out && !ell_sum && !grad_sum) return AGPL_OK;
    double *part = nullptr;
    if (ell_sum || grad_sum) {
        if (!ctx->elbo_part) AGPL_HIP(ctx, hipMalloc((void **)&ctx->elbo_part, sizeof(double) * 1024));
        part = ctx->elbo_part;
    }
    const int64_t want = agpl_cdiv(n, kBlock);
    const int nblk = (int)(want < kMaxBlocks ? want : kMaxBlocks);
    const bool launched = agpl::lik_switch(lik->kind, [&](auto K) {
        constexpr bool taken = !lik_is_categorical(K()); // (the categorical kinds: refused above)
        if constexpr (taken) expected_loglik_kernel<K()><<<(unsigned)nblk, kBlock, 0, ctx->stream>>>(p0, p1, n, mu, var, y, ell_out, dell_out, part);
        return taken;
    });
    if (!launched) AGPL_FAIL(ctx, AGPL_ERR_INVALID_ARGUMENT, "agpl_expected_loglik: no kernel for likelihood kind %d", lik->kind);
    AGPL_LAUNCH_CHECK(ctx);
    if (part) {
        likgrad_sum_kernel<<<(unsigned)(1 + P), kMaxBlocks, 0, ctx->stream>>>(part, nblk, ell_sum, grad_sum);
        AGPL_LAUNCH_CHECK(ctx);
    }
    return AGPL_OK;
}
