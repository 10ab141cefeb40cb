// agpl_operators.hip -- everything deterministic per point: aux_posterior!, (expected_)auglik_{potential,precision}, the ELBO
// N-reductions, and the sweep's fused per-point kernel.  HBM-bound streaming kernels; the per-likelihood formulas are those of
// agpl_lik_rules.h, fed from arrays here and from registers in the fused kernel.  The kernels that draw live in agpl_sampler.hip.
#include <math.h>
#include <cstdlib>

#include "agpl_internal.h"
#include "agpl_lik_rules.h"

using namespace agpl;

namespace {

// ------------------------------------------------------------------------------------------------
// The three operators over arrays: the rules of agpl_lik_rules.h, one point per thread.  mu, var, f: [N][L]; the auxiliary arrays
// (out1 .. out3 = q1, q2, psi; omega, n): [N][La], La auxiliary variables per point; beta, gamma: [L][N].
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ int aux_per_point(const agpl_lik_dev &lik) { return lik.kind == AGPL_LIK_HETEROGAUSS ? 1 : lik.nlatent; }

template <typename T>
__global__ __launch_bounds__(kBlock) void aux_posterior_kernel(agpl_lik_dev lik_arg, int64_t n, const void *yv,
                                                               const T *__restrict__ mu,
                                                               const T *__restrict__ var, T *__restrict__ out1,
                                                               T *__restrict__ out2, T *__restrict__ out3) {
    const int L = lik_arg.nlatent, La = aux_per_point(lik_arg);
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
         i += (int64_t)gridDim.x * blockDim.x)
        lik_dispatch(lik_arg, [&](const agpl_lik_dev &lik) {
            lik_aux_posterior<T>(
                lik, YAcc<T, T>{yv, i, lik.kind, L}, [&](int k) { return mu[i * L + k]; }, [&](int k) { return var[i * L + k]; },
                [&](int k, T o1, T o2, T o3) {
                    out1[i * La + k] = o1;
                    if (lik_needs_second(lik.kind)) out2[i * La + k] = o2;
                    if (lik.kind == AGPL_LIK_HETEROGAUSS) out3[i] = o3;
                });
        });
}

template <typename T>
__global__ __launch_bounds__(kBlock) void expected_pp_kernel(agpl_lik_dev lik_arg, int64_t n, const void *yv,
                                                             const T *__restrict__ q1, const T *__restrict__ q2,
                                                             const T *__restrict__ mu_g, T *__restrict__ beta,
                                                             T *__restrict__ gamma) {
    const int L = lik_arg.nlatent, La = aux_per_point(lik_arg);
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
         i += (int64_t)gridDim.x * blockDim.x)
        lik_dispatch(lik_arg, [&](const agpl_lik_dev &lik) {
            lik_expected_pp<T>(
                lik, YAcc<T, T>{yv, i, lik.kind, L},
                [&](int k) { return LikAux<T>{q1[i * La + k], lik_needs_second(lik.kind) ? q2[i * La + k] : T(0)}; },
                [&](int) { return mu_g[i]; },
                [&](int k, T gm, T bt, T) {
                    gamma[(int64_t)k * n + i] = gm;
                    beta[(int64_t)k * n + i] = bt;
                });
        });
}

__global__ __launch_bounds__(kBlock) void potential_precision_kernel(agpl_lik_dev lik_arg, int64_t n, const void *yv,
                                                                     const double *__restrict__ omega,
                                                                     const int64_t *__restrict__ nn,
                                                                     const double *__restrict__ fg,
                                                                     double *__restrict__ beta,
                                                                     double *__restrict__ gamma) {
    const int L = lik_arg.nlatent, La = aux_per_point(lik_arg);
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
         i += (int64_t)gridDim.x * blockDim.x)
        lik_dispatch(lik_arg, [&](const agpl_lik_dev &lik) {
            lik_sampled_pp(
                lik, YAcc<double>{yv, i, lik.kind, L}, [&](int k) { return omega[i * La + k]; },
                [&](int k) { return (double)nn[i * La + k]; }, [&](int k) { return fg[i * L + k]; },
                [&](int k, double gm, double bt) {
                    gamma[(int64_t)k * n + i] = gm;
                    beta[(int64_t)k * n + i] = bt;
                });
        });
}

// ------------------------------------------------------------------------------------------------
// ELBO N-reductions.  Per-point terms (float64), block tree-reduce, fixed-order final sum:
// bitwise reproducible.
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ double logcosh_(double x) { // LogExpFunctions.logcosh
    double ax = fabs(x);
    return ax + log1p(exp(-2.0 * ax)) - kLogTwo;
}
__device__ __forceinline__ double pg_logtilt(double omega, double b, double c) { // polyagamma.jl:108-110
    return b * logcosh_(c / 2.0) - c * c * omega / 2.0;
}
__device__ __forceinline__ double pg_kl(double b, double c) { // polyagamma.jl:99-106
    return pg_logtilt(pg_mean(b, c), b, c);
}
__device__ __forceinline__ double negbin_logconst(double y, double r) { // negativebinomial.jl:51-52
    return lgamma(y + r) - lgamma(y + 1.0) - lgamma(r);
}
// log C(n, y) of the binomial kind (agpl.h); a count outside 0..n meets a pole of lgamma: -inf
__device__ __forceinline__ double binomial_logconst(double y, double n) {
    return lgamma(n + 1.0) - lgamma(y + 1.0) - lgamma(n - y + 1.0);
}
// The binomial kinds' per-point terms with the trials as an argument: kind 8 passes p[0], kind 11 the point's own n_i.
__device__ __forceinline__ double binomial_logtilt(double yy, double nt, double f, double omega) {
    return binomial_logconst(yy, nt) - nt * kLogTwo + (yy - nt / 2.0) * f - f * f * omega / 2.0;
}
__device__ __forceinline__ double binomial_expected_logtilt(double yy, double nt, double m, double v, double c) {
    double th = pg_mean(nt, c);
    return binomial_logconst(yy, nt) - nt * kLogTwo + (yy - nt / 2.0) * m - (m * m + v) * th / 2.0;
}
// expected_logtilt - KL with the theta terms cancelled (elbo_point): log C - n log 2 + (y - n / 2) mu - n logcosh(c / 2)
__device__ __forceinline__ double binomial_elbo_term(double yy, double nt, double m, double c) {
    return binomial_logconst(yy, nt) - nt * kLogTwo + (yy - nt / 2.0) * m - nt * logcosh_(c / 2.0);
}
__device__ __forceinline__ double digamma_(double x) {
    double r = 0.0;
    while (x < 6.0) {
        r -= 1.0 / x;
        x += 1.0;
    }
    double f = 1.0 / (x * x);
    return r + log(x) - 0.5 / x -
           f * (1.0 / 12.0 - f * (1.0 / 120.0 - f * (1.0 / 252.0 - f * (1.0 / 240.0 - f / 132.0))));
}

// logpdf(PolyaGamma(b, c), x) -- polyagamma.jl:37-91: exponential tilt + (b-1) log 2 - (log 2pi + 3 log x) / 2 + the
// log of the 101-term alternating series (n = 0, 2, .., 200), evaluated in the log domain (logsumexp) for x < 1e-2
// exactly as the reference does.  The running product prod_{m<=n} (1 + (b-1)/m) is carried along; the log-domain
// branch makes two passes over the terms (maximum, then sum) instead of materialising them.
__device__ __forceinline__ double log1mexp_(double x) { // LogExpFunctions.log1mexp, x < 0
    return x < -kLogTwo ? log1p(-exp(x)) : log(-expm1(x));
}
__device__ double pg_log_series_term(double x, double b, int n, double logprod) {
    const double Rn = 2.0 * n + b;
    const double log_c_nb = log(n + b) - log(n + 1.0) + log(2.0 / Rn + 1.0);
    const double log_inner = log1mexp_(log_c_nb + ((Rn + 1.0) / (-2.0 * x)));
    return (n == 0 ? 0.0 : logprod) + log(Rn) + Rn * Rn / (-8.0 * x) + log_inner;
}
__device__ double pg_logpdf(double b, double c, double x) {
    if (b == 0.0) return x == 0.0 ? 0.0 : -__builtin_inf();
    const double ext = b * logcosh_(c / 2.0) - c * c * x / 2.0 + (b - 1.0) * kLogTwo - (kLog2Pi + 3.0 * log(x)) / 2.0;
    if (x < 1e-2) {
        double mx = -__builtin_inf(), logprod = 0.0;
        int m = 0;
        for (int n = 0; n <= 200; n += 2) {
            while (m < n) {
                m += 1;
                logprod += log(1.0 + (b - 1.0) / m);
            }
            const double t = pg_log_series_term(x, b, n, logprod);
            mx = t > mx ? t : mx;
        }
        double ssum = 0.0;
        logprod = 0.0;
        m = 0;
        for (int n = 0; n <= 200; n += 2) {
            while (m < n) {
                m += 1;
                logprod += log(1.0 + (b - 1.0) / m);
            }
            ssum += exp(pg_log_series_term(x, b, n, logprod) - mx);
        }
        return ext + mx + log(ssum);
    }
    double prod = 1.0, acc = 0.0;
    int m = 0;
    for (int n = 0; n <= 200; n += 2) {
        while (m < n) {
            m += 1;
            prod *= 1.0 + (b - 1.0) / m;
        }
        const double Rn = 2.0 * n + b;
        const double c_nb = ((n + b) / (n + 1.0)) * (2.0 / Rn + 1.0);
        acc += (n == 0 ? 1.0 : prod) * Rn * exp(Rn * Rn / (-8.0 * x)) * (1.0 - c_nb * exp((Rn + 1.0) / (-2.0 * x)));
    }
    if (!(acc > 2.2250738585072014e-308)) acc = 2.2250738585072014e-308; // max(s, floatmin)
    return ext + log(acc);
}

enum { RED_LOGTILT = 0, RED_EXPECTED_LOGTILT = 1, RED_KL = 2, RED_AUX_PRIOR_LOGPDF = 3, RED_AUG_LOGLIK = 4, RED_EXPECTED_AUG_LOGLIK = 5 };

struct RedArgs {
    const void *y;
    const double *a1; // omega | q1
    const double *a2; // (unused) | q2
    const int64_t *nn;
    const double *f;   // f | mu
    const double *var; // var
};

// One point's expected_logtilt (bernoulli.jl:59-65, negativebinomial.jl:59-65, studentt.jl:80-83, categorical.jl:172-180,
// poisson.jl:76-85, laplace.jl:83-88) and aux_kldivergence (generic.jl:56-62) term from accessors -- y(k), q1(k), q2(k), mu(k),
// var(k), all double, k = latent -- shared by the reduction kernels (accessors over arrays) and by the sweep's per-point kernel
// (accessors over the marginals it has just formed): the same expressions, hence the same float64 results.
template <class Y, class Q1, class Q2, class MU, class VAR>
__device__ __forceinline__ double expected_logtilt_point(const agpl_lik_dev &lik, Y y, Q1 q1, Q2 q2, MU mu, VAR var) {
    const int L = lik.nlatent;
    switch (lik.kind) {
    case AGPL_LIK_BERNOULLI_LOGISTIC: { // bernoulli.jl:59-65
        double s = y(0) != 0.0 ? 1.0 : -1.0;
        double th = pg_mean(1.0, q1(0));
        return -kLogTwo + (s * mu(0) - (mu(0) * mu(0) + var(0)) * th) / 2.0;
    }
    case AGPL_LIK_NEGBINOMIAL: { // negativebinomial.jl:59-65
        double r = lik.p[0], yy = y(0);
        double th = pg_mean(yy + r, q1(0));
        return negbin_logconst(yy, r) - (yy + r) * kLogTwo + (mu(0) * (yy - r) - (mu(0) * mu(0) + var(0)) * th) / 2.0;
    }
    case AGPL_LIK_BINOMIAL: // (agpl.h) logtilt with f -> mu, f^2 -> mu^2 + var, omega -> theta = E PG(n, c)
    case AGPL_LIK_BINOMIAL_N: {
        double nt = binomial_n<double>(lik, y), yy = y(0);
        return binomial_expected_logtilt(yy, nt, mu(0), var(0), q1(0));
    }
    case AGPL_LIK_STUDENTT: { // studentt.jl:80-83
        double th = ((lik.p[0] + 1.0) / 2.0) / q1(0);
        double d = mu(0) - y(0);
        return -0.5 * kLog2Pi + 0.5 * log(th) - 0.5 * d * d * th - var(0) * th / 2.0;
    }
    case AGPL_LIK_CATEGORICAL:
    case AGPL_LIK_CATEGORICAL_BIJ: { // categorical.jl:172-180
        double sp = 0.0;
        for (int k = 0; k < L; ++k) sp += q2(k);
        double p0 = 1.0 - sp, s1 = 0.0, s2 = 0.0;
        for (int k = 0; k < L; ++k) {
            double yk = y(k), nbar = q2(k) / p0;
            double w = pg_mean(yk + nbar, q1(k));
            double m = mu(k), v = var(k);
            s1 += yk + nbar;
            s2 += ((yk - nbar) * m - (m * m + v) * w) / 2.0;
        }
        return -s1 * kLogTwo + s2;
    }
    case AGPL_LIK_POISSON: { // poisson.jl:76-85
        double yy = y(0), nbar = q2(0);
        double w = pg_mean(yy + nbar, q1(0));
        return -(yy + nbar) * kLogTwo + ((yy - nbar) * mu(0) - (mu(0) * mu(0) + var(0)) * w) / 2.0 + yy * log(lik.p[0]) -
               lgamma(yy + 1.0);
    }
    case AGPL_LIK_LAPLACE: { // laplace.jl:83-88
        double yy = y(0);
        return lgamma(0.5) - 0.5 * log(kPi) - log(2.0 * lik.p[0]) - ((mu(0) - yy) * (mu(0) - yy) + var(0)) * q1(0);
    }
    case AGPL_LIK_ASYMLAPLACE: { // (agpl.h) Laplace's at beta = 2 sigma + kappa (y - mu) + log(4 tau (1 - tau))
        double yy = y(0);
        return lgamma(0.5) - 0.5 * log(kPi) - log(2.0 * ald_beta<double>(lik)) - ((mu(0) - yy) * (mu(0) - yy) + var(0)) * q1(0) +
               ald_kappa<double>(lik) * (yy - mu(0)) + ald_logconst(lik);
    }
    case AGPL_LIK_LOGISTIC_NOISE: { // (agpl.h) logtilt with (y - f)^2 -> (mu - y)^2 + var, omega -> theta = E PG(2, c)
        double s = lik.p[0], yy = y(0);
        double th = pg_mean(2.0, q1(0));
        return -log(4.0 * s) - ((mu(0) - yy) * (mu(0) - yy) + var(0)) * th / (2.0 * s * s);
    }
    default:
        return __builtin_nan("");
    }
}
template <class Y, class Q1, class Q2>
__device__ __forceinline__ double aux_kl_point(const agpl_lik_dev &lik, Y y, Q1 q1, Q2 q2) {
    const int L = lik.nlatent;
    switch (lik.kind) {
    case AGPL_LIK_BERNOULLI_LOGISTIC:
        return pg_kl(1.0, q1(0));
    case AGPL_LIK_NEGBINOMIAL:
        return pg_kl(y(0) + lik.p[0], q1(0));
    case AGPL_LIK_BINOMIAL:
    case AGPL_LIK_BINOMIAL_N:
        return pg_kl(binomial_n<double>(lik, y), q1(0));
    case AGPL_LIK_LOGISTIC_NOISE:
        return pg_kl(2.0, q1(0));
    case AGPL_LIK_STUDENTT: { // KL(Gamma(alpha, 1/beta_i) || Gamma(nu/2, 2 sigma^2/nu)) studentt.jl:85-91
        double nu = lik.p[0], sg = lik.p[1];
        double ap = (nu + 1.0) / 2.0, thp = 1.0 / q1(0);
        double aq = nu / 2.0, thq = sg * sg / (nu / 2.0);
        return (ap - aq) * digamma_(ap) - lgamma(ap) + lgamma(aq) + aq * (log(thq) - log(thp)) + ap * (thp - thq) / thq;
    }
    case AGPL_LIK_POISSON: { // polyagammapoisson.jl:47-51
        double lq = q2(0), lp = lik.p[0];
        double klp = lq > 0 ? lq * (log(lq) - log(lp)) - lq + lp : lp;
        return pg_kl(y(0) + lq, q1(0)) + klp;
    }
    case AGPL_LIK_LAPLACE: { // laplace.jl:96-104
        double lam = 1.0 / ((2.0 * lik.p[0]) * (2.0 * lik.p[0]));
        return log(2.0 * lam) / 2.0 - log(2.0 * kPi) / 2.0 - log(lam) / 2.0 + lgamma(0.5) + lam / q1(0);
    }
    case AGPL_LIK_ASYMLAPLACE: { // Laplace's at beta = 2 sigma
        double lam = 1.0 / ((2.0 * ald_beta<double>(lik)) * (2.0 * ald_beta<double>(lik)));
        return log(2.0 * lam) / 2.0 - log(2.0 * kPi) / 2.0 - log(lam) / 2.0 + lgamma(0.5) + lam / q1(0);
    }
    case AGPL_LIK_CATEGORICAL_BIJ: { // polyagammanegativemultinomial.jl:56-65, negativemultinomial.jl:72-82
        double sp = 0.0;
        for (int k = 0; k < L; ++k) sp += q2(k);
        double p0 = 1.0 - sp;
        double pp = 1.0 / lik.sum_theta;
        double p0p = 1.0 - L * pp;
        double s = 0.0, acc = 0.0;
        for (int k = 0; k < L; ++k) {
            double nbar = q2(k) / p0;
            acc += pg_kl(y(k) + nbar, q1(k));
            s += q2(k) * (log(q2(k)) - log(pp));
        }
        return acc + log(p0) - log(p0p) + s / p0;
    }
    default:
        return __builtin_nan("");
    }
}
__device__ double red_term(int mode, const agpl_lik_dev &lik, int64_t i, const RedArgs &A);

// logpdf(Poisson(lam), n) -- Distributions.jl closed form (upstream, unpinned)
__device__ __forceinline__ double poisson_logpdf(double lam, double n) {
    if (lam == 0.0) return n == 0.0 ? 0.0 : -__builtin_inf();
    return n * log(lam) - lam - lgamma(n + 1.0);
}
// logdensity_def(aux_prior(lik, y), Omega) per point -- the second half of aug_loglik (generic.jl:48-50).
// PG(1, 0) bernoulli.jl:51-57 ; PG(y + r, 0) negativebinomial.jl:67-73 ; Gamma(nu/2, scale 2 sigma^2/nu) studentt.jl:91 ;
// PolyaGammaPoisson(y, 0, lambda) poisson.jl:67-76 with the joint density of polyagammapoisson.jl:29-33 ;
// InverseGamma(1/2, (2 beta)^-2) laplace.jl:90-96.  The categorical prior goes through the reference's broken logdensity_def
// (polyagammanegativemultinomial.jl:33-39): unsupported.  The heteroscedastic likelihood has no aux_prior
// (its aug_loglik is its own method, below).
__device__ double aux_prior_logpdf_term(const agpl_lik_dev &lik, int64_t i, const RedArgs &A) {
    const double *omega = A.a1;
    switch (lik.kind) {
    case AGPL_LIK_BERNOULLI_LOGISTIC:
        return pg_logpdf(1.0, 0.0, omega[i]);
    case AGPL_LIK_NEGBINOMIAL:
        return pg_logpdf((double)((const int32_t *)A.y)[i] + lik.p[0], 0.0, omega[i]);
    case AGPL_LIK_BINOMIAL: // PG(n, 0)
        return pg_logpdf(lik.p[0], 0.0, omega[i]);
    case AGPL_LIK_BINOMIAL_N: // PG(n_i, 0)
        return pg_logpdf(binomial_trials<double>((double)((const int32_t *)A.y)[2 * i + 1]), 0.0, omega[i]);
    case AGPL_LIK_LOGISTIC_NOISE: // PG(2, 0)
        return pg_logpdf(2.0, 0.0, omega[i]);
    case AGPL_LIK_STUDENTT: {
        const double a = lik.p[0] / 2.0, th = lik.p[1] * lik.p[1] / a;
        return -lgamma(a) - a * log(th) + (a - 1.0) * log(omega[i]) - omega[i] / th;
    }
    case AGPL_LIK_POISSON: {
        const double nk = (double)A.nn[i];
        return poisson_logpdf(lik.p[0], nk) + pg_logpdf((double)((const int32_t *)A.y)[i] + nk, 0.0, omega[i]);
    }
    case AGPL_LIK_LAPLACE: {
        const double lam = 1.0 / ((2.0 * lik.p[0]) * (2.0 * lik.p[0]));
        return 0.5 * log(lam) - lgamma(0.5) - 1.5 * log(omega[i]) - lam / omega[i];
    }
    case AGPL_LIK_ASYMLAPLACE: { // InverseGamma(1/2, (2 beta)^-2) at beta = 2 sigma
        const double lam = 1.0 / ((2.0 * ald_beta<double>(lik)) * (2.0 * ald_beta<double>(lik)));
        return 0.5 * log(lam) - lgamma(0.5) - 1.5 * log(omega[i]) - lam / omega[i];
    }
    default:
        return __builtin_nan("");
    }
}
// aug_loglik(lik::AugHeteroGaussian, (omega, n), y, (f, g)) heteroscedasticgaussian.jl:118-128 ; fg = [2, N]
__device__ double hetero_aug_loglik_term(const agpl_lik_dev &lik, int64_t i, const RedArgs &A) {
    const double ff = A.f[2 * i], gg = A.f[2 * i + 1], yy = ((const double *)A.y)[i];
    const double nk = (double)A.nn[i], om = A.a1[i];
    return -(0.5 + nk) * kLogTwo + ((0.5 - nk) * gg - gg * gg * om) / 2.0 + pg_logpdf(0.5 + nk, 0.0, om) +
           poisson_logpdf(lik.p[0] / 2.0 * (yy - ff) * (yy - ff), nk);
}
// expected_aug_loglik(lik::AugHeteroGaussian, qOmega, y, qfg) heteroscedasticgaussian.jl:130-145 ; q1 = c, q2 = lambda of
// aux_posterior!, (mu, var) = q(f), q(g) as [2, N]; `var(first(qg))` is read as var(qg)
__device__ double hetero_expected_aug_loglik_term(const agpl_lik_dev &lik, int64_t i, const RedArgs &A) {
    const double lam = lik.p[0], yy = ((const double *)A.y)[i];
    const double mf = A.f[2 * i], vf = A.var[2 * i], g = A.f[2 * i + 1], vg = A.var[2 * i + 1];
    const double tn = A.a2[i], tw = pg_mean(0.5 + tn, A.a1[i]);
    const double lp = lam / 2.0 * ((yy - mf) * (yy - mf) + vf);
    const double klp = tn > 0 ? tn * (log(tn) - log(lp)) - tn + lp : lp;
    return 0.5 * (log(lam) + log(2.0 / kPi)) - (0.5 + tn) * kLogTwo + ((0.5 - tn) * g - (g * g + vg) * tw) / 2.0 +
           pg_kl(0.5 + tn, A.a1[i]) + klp;
}

__device__ double red_term(int mode, const agpl_lik_dev &lik, int64_t i, const RedArgs &A) {
    const int L = lik.nlatent;
    const double nanv = __builtin_nan("");
    if (mode == RED_AUX_PRIOR_LOGPDF) return aux_prior_logpdf_term(lik, i, A);
    if (lik.kind == AGPL_LIK_HETEROGAUSS) // the two methods the reference defines for it; everything else is refused on the host
        return mode == RED_AUG_LOGLIK ? hetero_aug_loglik_term(lik, i, A) : hetero_expected_aug_loglik_term(lik, i, A);
    if (mode == RED_AUG_LOGLIK) return red_term(RED_LOGTILT, lik, i, A) + aux_prior_logpdf_term(lik, i, A);
    if (mode == RED_EXPECTED_AUG_LOGLIK) // generic.jl:52-54: expected_logtilt + aux_kldivergence (the sign is the reference's)
        return red_term(RED_EXPECTED_LOGTILT, lik, i, A) + red_term(RED_KL, lik, i, A);
    if (mode == RED_LOGTILT) {
        const double *omega = A.a1, *f = A.f;
        switch (lik.kind) {
        case AGPL_LIK_BERNOULLI_LOGISTIC: { // bernoulli.jl:47-49
            double s = ((const uint8_t *)A.y)[i] ? 1.0 : -1.0;
            return -kLogTwo + (s * f[i] - f[i] * f[i] * omega[i]) / 2.0;
        }
        case AGPL_LIK_NEGBINOMIAL: { // negativebinomial.jl:54-57
            double r = lik.p[0], yy = (double)((const int32_t *)A.y)[i];
            return negbin_logconst(yy, r) - (yy + r) * kLogTwo + (f[i] * (yy - r) - f[i] * f[i] * omega[i]) / 2.0;
        }
        case AGPL_LIK_BINOMIAL: { // (agpl.h)
            return binomial_logtilt((double)((const int32_t *)A.y)[i], lik.p[0], f[i], omega[i]);
        }
        case AGPL_LIK_BINOMIAL_N: { // kind 8's at the point's n
            const int32_t *yn = (const int32_t *)A.y + 2 * i;
            return binomial_logtilt((double)yn[0], binomial_trials<double>((double)yn[1]), f[i], omega[i]);
        }
        case AGPL_LIK_STUDENTT: { // studentt.jl:76-78
            double d = ((const double *)A.y)[i] - f[i];
            return -0.5 * kLog2Pi + 0.5 * log(omega[i]) - 0.5 * d * d * omega[i];
        }
        case AGPL_LIK_CATEGORICAL:
        case AGPL_LIK_CATEGORICAL_BIJ: { // categorical.jl:138-145
            const uint8_t *y = (const uint8_t *)A.y;
            double s1 = 0.0, s2 = 0.0;
            for (int k = 0; k < L; ++k) {
                double yk = (double)y[i * L + k], nk = (double)A.nn[i * L + k], fk = f[i * L + k];
                s1 += yk + nk;
                s2 += (yk - nk) * fk - fk * fk * omega[i * L + k];
            }
            return -s1 * kLogTwo + s2 / 2.0;
        }
        case AGPL_LIK_POISSON: { // poisson.jl:62-65
            double yy = (double)((const int32_t *)A.y)[i], nk = (double)A.nn[i];
            return yy * log(lik.p[0]) - (yy + nk) * kLogTwo - lgamma(yy + 1.0) +
                   ((yy - nk) * f[i] - f[i] * f[i] * omega[i]) / 2.0;
        }
        case AGPL_LIK_LAPLACE: { // laplace.jl:78-81
            double d = ((const double *)A.y)[i] - f[i];
            return lgamma(0.5) - 0.5 * log(kPi) - log(2.0 * lik.p[0]) - d * d * omega[i];
        }
        case AGPL_LIK_ASYMLAPLACE: { // (agpl.h) Laplace's at beta = 2 sigma + kappa (y - f) + log(4 tau (1 - tau))
            double d = ((const double *)A.y)[i] - f[i];
            return lgamma(0.5) - 0.5 * log(kPi) - log(2.0 * ald_beta<double>(lik)) - d * d * omega[i] + ald_kappa<double>(lik) * d +
                   ald_logconst(lik);
        }
        case AGPL_LIK_LOGISTIC_NOISE: { // (agpl.h)
            double s = lik.p[0], d = ((const double *)A.y)[i] - f[i];
            return -log(4.0 * s) - d * d * omega[i] / (2.0 * s * s);
        }
        default:
            return nanv;
        }
    }
    const double *q1 = A.a1, *q2 = A.a2;
    const YAcc<double> y{A.y, i, lik.kind, L};
    auto q1a = [&](int k) { return q1[i * L + k]; };
    auto q2a = [&](int k) { return q2[i * L + k]; };
    if (mode == RED_EXPECTED_LOGTILT) {
        const double *mu = A.f, *var = A.var;
        return expected_logtilt_point(lik, y, q1a, q2a, [&](int k) { return mu[i * L + k]; }, [&](int k) { return var[i * L + k]; });
    }
    return aux_kl_point(lik, y, q1a, q2a); // RED_KL: aux_kldivergence generic.jl:56-62
}

__global__ __launch_bounds__(kBlock) void reduce_terms_kernel(int mode, agpl_lik_dev lik, int64_t n, RedArgs A,
                                                              double *__restrict__ partial) {
    __shared__ double sm[kBlock];
    double acc = 0.0;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
         i += (int64_t)gridDim.x * blockDim.x)
        acc += red_term(mode, lik, i, A);
    sm[threadIdx.x] = acc;
    __syncthreads();
    for (int s = kBlock / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) sm[threadIdx.x] += sm[threadIdx.x + s];
        __syncthreads();
    }
    if (threadIdx.x == 0) partial[blockIdx.x] = sm[0];
}

__global__ void reduce_final_kernel(int nparts, const double *__restrict__ partial, double *__restrict__ out) {
    if (threadIdx.x == 0 && blockIdx.x == 0) {
        double acc = 0.0;
        for (int i = 0; i < nparts; ++i) acc += partial[i];
        *out = acc;
    }
}

int32_t run_reduction(agpl_ctx *ctx, int mode, const agpl_lik_desc *lik, int64_t n, const RedArgs &A,
                      double *out_host) {
    if (!ctx || !out_host) return AGPL_ERR_INVALID_ARGUMENT;
    agpl_lik_dev ld;
    int32_t rc = agpl_lik_to_device(ctx, lik, &ld);
    if (rc) return rc;
    if ((mode == RED_KL || mode == RED_EXPECTED_AUG_LOGLIK) && lik->kind == AGPL_LIK_CATEGORICAL)
        AGPL_FAIL(ctx, AGPL_ERR_UNSUPPORTED,
                  "the kl-divergence cannot be computed for the non-bijective LogisticSoftMaxLink "
                  "(categorical.jl:165-170); use the bijective link");
    if (lik->kind == AGPL_LIK_HETEROGAUSS && mode != RED_AUG_LOGLIK && mode != RED_EXPECTED_AUG_LOGLIK)
        AGPL_FAIL(ctx, AGPL_ERR_UNSUPPORTED,
                  "the heteroscedastic likelihood defines aug_loglik and expected_aug_loglik only "
                  "(heteroscedasticgaussian.jl:106-145): its tilt, prior and KL are not split in the reference");
    if ((mode == RED_AUX_PRIOR_LOGPDF || mode == RED_AUG_LOGLIK) &&
        (lik->kind == AGPL_LIK_CATEGORICAL || lik->kind == AGPL_LIK_CATEGORICAL_BIJ))
        AGPL_FAIL(ctx, AGPL_ERR_UNSUPPORTED,
                  "aug_loglik / the aux-prior log-density of the categorical likelihood: the reference's logdensity_def of "
                  "PolyaGammaNegativeMultinomial is broken (polyagammanegativemultinomial.jl:33-39, SURVEY App. B)");
    // (the categorical kinds were refused above)
    if ((mode == RED_AUX_PRIOR_LOGPDF || mode == RED_AUG_LOGLIK) && lik_needs_counts(lik->kind) && n > 0 && !A.nn)
        AGPL_FAIL(ctx, AGPL_ERR_INVALID_ARGUMENT, "this likelihood's prior density needs the counts n_aux");
    if (n <= 0) {
        *out_host = 0.0;
        return AGPL_OK;
    }
    // one partial per workgroup, as many as their region of the small scratch holds (agpl_ws2.h)
    int nb = grid_for(n);
    if (nb > kRedParts) nb = kRedParts;
    rc = agpl_ws2_reserve(ctx, kWs2Head);
    if (rc) return rc;
    double *partial = agpl_ws2_partials(ctx), *result = agpl_ws2_result(ctx);
    reduce_terms_kernel<<<nb, kBlock, 0, ctx->stream>>>(mode, ld, n, A, partial);
    AGPL_LAUNCH_CHECK(ctx);
    reduce_final_kernel<<<1, 64, 0, ctx->stream>>>(nb, partial, result);
    AGPL_LAUNCH_CHECK(ctx);
    AGPL_HIP(ctx, hipMemcpyAsync(out_host, result, sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    AGPL_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return AGPL_OK;
}

} // namespace

extern "C" int32_t agpl_potential_precision(agpl_ctx *ctx, const agpl_lik_desc *lik, int64_t n, const void *y,
                                            const double *omega, const int64_t *n_aux, const double *fg,
                                            double *beta_out, double *gamma_out) {
    if (!ctx) return AGPL_ERR_INVALID_ARGUMENT;
    agpl_lik_dev ld;
    int32_t rc = agpl_lik_to_device(ctx, lik, &ld);
    if (rc) return rc;
    if (n < 0) AGPL_FAIL(ctx, AGPL_ERR_INVALID_ARGUMENT, "n < 0");
    if (n == 0) return AGPL_OK;
    if (!y || !omega || !beta_out || !gamma_out) AGPL_FAIL(ctx, AGPL_ERR_INVALID_ARGUMENT, "null argument");
    if (lik_needs_counts(ld.kind) && !n_aux) AGPL_FAIL(ctx, AGPL_ERR_INVALID_ARGUMENT, "this likelihood needs n_aux");
    if (ld.kind == AGPL_LIK_HETEROGAUSS && !fg) AGPL_FAIL(ctx, AGPL_ERR_INVALID_ARGUMENT, "heterogauss needs fg");
    potential_precision_kernel<<<grid_for(n), kBlock, 0, ctx->stream>>>(ld, n, y, omega, n_aux, fg, beta_out,
                                                                        gamma_out);
    AGPL_LAUNCH_CHECK(ctx);
    return AGPL_OK;
}

extern "C" int32_t agpl_aux_posterior(agpl_ctx *ctx, const agpl_lik_desc *lik, int32_t dtype, int64_t n,
                                      const void *y, const void *mu, const void *var, void *out1, void *out2,
                                      void *out3) {
    if (!ctx) return AGPL_ERR_INVALID_ARGUMENT;
    agpl_lik_dev ld;
    int32_t rc = agpl_lik_to_device(ctx, lik, &ld);
    if (rc) return rc;
    if (n < 0) AGPL_FAIL(ctx, AGPL_ERR_INVALID_ARGUMENT, "n < 0");
    if (n == 0) return AGPL_OK;
    if (!mu || !var || !out1) AGPL_FAIL(ctx, AGPL_ERR_INVALID_ARGUMENT, "null mu / var / out1");
    if (lik_needs_second(ld.kind) && !out2) AGPL_FAIL(ctx, AGPL_ERR_INVALID_ARGUMENT, "this likelihood needs out2");
    if (ld.kind == AGPL_LIK_HETEROGAUSS && !out3) AGPL_FAIL(ctx, AGPL_ERR_INVALID_ARGUMENT, "heterogauss needs out3");
    if (lik_needs_y(ld.kind) && !y) AGPL_FAIL(ctx, AGPL_ERR_INVALID_ARGUMENT, "null y");
    if (dtype == AGPL_F64)
        aux_posterior_kernel<double><<<grid_for(n), kBlock, 0, ctx->stream>>>(
            ld, n, y, (const double *)mu, (const double *)var, (double *)out1, (double *)out2, (double *)out3);
    else if (dtype == AGPL_F32)
        aux_posterior_kernel<float><<<grid_for(n), kBlock, 0, ctx->stream>>>(
            ld, n, y, (const float *)mu, (const float *)var, (float *)out1, (float *)out2, (float *)out3);
    else
        AGPL_FAIL(ctx, AGPL_ERR_INVALID_ARGUMENT, "dtype must be AGPL_F32 or AGPL_F64");
    AGPL_LAUNCH_CHECK(ctx);
    return AGPL_OK;
}

extern "C" int32_t agpl_expected_potential_precision(agpl_ctx *ctx, const agpl_lik_desc *lik, int32_t dtype,
                                                     int64_t n, const void *y, const void *q1, const void *q2,
                                                     const void *mu_g, void *beta_out, void *gamma_out) {
    if (!ctx) return AGPL_ERR_INVALID_ARGUMENT;
    agpl_lik_dev ld;
    int32_t rc = agpl_lik_to_device(ctx, lik, &ld);
    if (rc) return rc;
    if (n < 0) AGPL_FAIL(ctx, AGPL_ERR_INVALID_ARGUMENT, "n < 0");
    if (n == 0) return AGPL_OK;
    if (!y || !q1 || !beta_out || !gamma_out) AGPL_FAIL(ctx, AGPL_ERR_INVALID_ARGUMENT, "null argument");
    if (lik_needs_second(ld.kind) && !q2) AGPL_FAIL(ctx, AGPL_ERR_INVALID_ARGUMENT, "this likelihood needs q2");
    if (ld.kind == AGPL_LIK_HETEROGAUSS && !mu_g) AGPL_FAIL(ctx, AGPL_ERR_INVALID_ARGUMENT, "heterogauss needs mu_g");
    if (dtype == AGPL_F64)
        expected_pp_kernel<double><<<grid_for(n), kBlock, 0, ctx->stream>>>(
            ld, n, y, (const double *)q1, (const double *)q2, (const double *)mu_g, (double *)beta_out,
            (double *)gamma_out);
    else if (dtype == AGPL_F32)
        expected_pp_kernel<float><<<grid_for(n), kBlock, 0, ctx->stream>>>(
            ld, n, y, (const float *)q1, (const float *)q2, (const float *)mu_g, (float *)beta_out,
            (float *)gamma_out);
    else
        AGPL_FAIL(ctx, AGPL_ERR_INVALID_ARGUMENT, "dtype must be AGPL_F32 or AGPL_F64");
    AGPL_LAUNCH_CHECK(ctx);
    return AGPL_OK;
}

extern "C" int32_t agpl_logtilt(agpl_ctx *ctx, const agpl_lik_desc *lik, int64_t n, const void *y,
                                const double *omega, const int64_t *n_aux, const double *f, double *out_host) {
    RedArgs A{y, omega, nullptr, n_aux, f, nullptr};
    return run_reduction(ctx, RED_LOGTILT, lik, n, A, out_host);
}
extern "C" int32_t agpl_aux_prior_logpdf(agpl_ctx *ctx, const agpl_lik_desc *lik, int64_t n, const void *y,
                                         const double *omega, const int64_t *n_aux, double *out_host) {
    RedArgs A{y, omega, nullptr, n_aux, nullptr, nullptr};
    return run_reduction(ctx, RED_AUX_PRIOR_LOGPDF, lik, n, A, out_host);
}
extern "C" int32_t agpl_aug_loglik(agpl_ctx *ctx, const agpl_lik_desc *lik, int64_t n, const void *y,
                                   const double *omega, const int64_t *n_aux, const double *f, double *out_host) {
    RedArgs A{y, omega, nullptr, n_aux, f, nullptr};
    return run_reduction(ctx, RED_AUG_LOGLIK, lik, n, A, out_host);
}
extern "C" int32_t agpl_expected_logtilt(agpl_ctx *ctx, const agpl_lik_desc *lik, int64_t n, const void *y,
                                         const double *q1, const double *q2, const double *mu, const double *var,
                                         double *out_host) {
    RedArgs A{y, q1, q2, nullptr, mu, var};
    return run_reduction(ctx, RED_EXPECTED_LOGTILT, lik, n, A, out_host);
}
extern "C" int32_t agpl_aux_kldivergence(agpl_ctx *ctx, const agpl_lik_desc *lik, int64_t n, const void *y,
                                         const double *q1, const double *q2, double *out_host) {
    RedArgs A{y, q1, q2, nullptr, nullptr, nullptr};
    return run_reduction(ctx, RED_KL, lik, n, A, out_host);
}
extern "C" int32_t agpl_expected_aug_loglik(agpl_ctx *ctx, const agpl_lik_desc *lik, int64_t n, const void *y,
                                            const double *q1, const double *q2, const double *mu, const double *var,
                                            double *out_host) {
    RedArgs A{y, q1, q2, nullptr, mu, var};
    return run_reduction(ctx, RED_EXPECTED_AUG_LOGLIK, lik, n, A, out_host);
}

// fused elementwise step of a sweep: aux_posterior! + expected potential / precision of point i from its marginals.
// MG gives the marginal of latent k (m(k, i), v(k, i)); OUT takes (gamma, beta) of latent k.  One code path for both callers:
// agpl_fused_elementwise_kernel (marginals in arrays, outputs in arrays) and agpl_fused_point_kernel (marginals summed on
// the fly from the marginal kernel's row-block partials, outputs as the accumulation's gamma | beta records).
template <class MG, class OUT>
__device__ __forceinline__ void fused_point(const agpl_lik_dev &lik_arg, int64_t i, const void *yv, const MG &mg, OUT &out,
                                            float *__restrict__ c_out) {
    const int L = lik_arg.nlatent;
    lik_dispatch(lik_arg, [&](const agpl_lik_dev &lik) {
        const YAcc<float, float> y{yv, i, lik.kind, L};
        if (lik_is_categorical(lik.kind)) { // L latents, a run-time count: q(omega_k) is re-formed where the expectation reads it
            lik_expected_pp<float>(         // (twice per latent) instead of being kept in per-point arrays
                lik, y,
                [&](int k) {
                    float o1, o2, o3;
                    lik_aux_posterior_at<float>(lik, k, y, [&](int kk) { return mg.m(kk, i); }, [&](int kk) { return mg.v(kk, i); }, o1, o2, o3);
                    return LikAux<float>{o1, o2};
                },
                [](int) { return 0.f; },
                [&](int k, float gm, float bt, float c) {
                    out.put(k, i, gm, bt);
                    if (c_out) c_out[i * L + k] = c;
                });
            return;
        }
        // one auxiliary variable, one or two latents: the marginals are summed once and everything stays in registers between the rules
        const bool two = lik.kind == AGPL_LIK_HETEROGAUSS;
        const float m0 = mg.m(0, i), v0 = mg.v(0, i), m1 = two ? mg.m(1, i) : 0.f, v1 = two ? mg.v(1, i) : 0.f;
        float q1 = 0.f, q2 = 0.f, og[2], ob[2];
        lik_aux_posterior<float>(
            lik, y, [&](int k) { return k ? m1 : m0; }, [&](int k) { return k ? v1 : v0; },
            [&](int, float o1, float o2, float) { q1 = o1, q2 = o2; });
        lik_expected_pp<float>(
            lik, y, [&](int) { return LikAux<float>{q1, q2}; }, [&](int) { return m1; },
            [&](int k, float gm, float bt, float) { og[k] = gm, ob[k] = bt; });
        if (c_out) c_out[i] = q1;
        out.put(0, i, og[0], ob[0]);
        if (two) out.put(1, i, og[1], ob[1]);
    });
}

// expected_logtilt_i - aux_kldivergence_i (the per-point part of aug_elbo, examples/bernoulli/script.jl:65-70) for q(f_i) = the
// marginal `mg` gives and qOmega_i = aux_posterior(lik, y_i, q(f_i)), evaluated in float64 FROM the float32 marginals -- the value
// the float64 operator kernels (aux_posterior_kernel<double>, reduce_terms_kernel) give for the same marginals.  NaN for the
// likelihoods whose terms the reference does not define (non-bijective categorical KL, heteroscedastic).
template <class MG>
__device__ __forceinline__ double elbo_point(const agpl_lik_dev &lik, int64_t i, const void *yv, const MG &mg) {
    const int L = lik.nlatent;
    const YAcc<float> y{yv, i, lik.kind, L};
    auto mu = [&](int k) { return (double)mg.m(k, i); };
    auto var = [&](int k) { return (double)mg.v(k, i); };
    auto q1 = [&](int k) { // out1 of aux_posterior!
        double o1, o2, o3;
        lik_aux_posterior_at<double>(lik, k, y, mu, var, o1, o2, o3);
        return o1;
    };
    auto q2 = [&](int k) { // out2 of aux_posterior!
        double o1, o2, o3;
        lik_aux_posterior_at<double>(lik, k, y, mu, var, o1, o2, o3);
        return o2;
    };
    // Bernoulli / negative binomial / binomial: with theta = E[omega] = b tanh(c / 2) / (2 c) and c^2 = mu^2 + sigma^2 the theta terms of
    // expected_logtilt (.. - c^2 theta / 2) and of KL(PG(b, c) || PG(b, 0)) = b logcosh(c / 2) - c^2 theta / 2 cancel: what is
    // left needs one logcosh (0.78 -> ~0.1 ms per 1e7 points against the literal expressions; equal to them to rounding)
    if (lik.kind == AGPL_LIK_BERNOULLI_LOGISTIC || lik.kind == AGPL_LIK_NEGBINOMIAL || lik.kind == AGPL_LIK_BINOMIAL ||
        lik.kind == AGPL_LIK_BINOMIAL_N) {
        const double m = mu(0), v = var(0);
        double c, o2, o3;
        lik_aux_posterior_at<double>(lik, 0, y, [&](int) { return m; }, [&](int) { return v; }, c, o2, o3);
        if (lik.kind == AGPL_LIK_BERNOULLI_LOGISTIC) return -kLogTwo + (y(0) != 0.0 ? m : -m) / 2.0 - logcosh_(c / 2.0);
        if (lik.kind == AGPL_LIK_BINOMIAL || lik.kind == AGPL_LIK_BINOMIAL_N) {
            const double nt = binomial_n<double>(lik, y), yy = y(0);
            return binomial_elbo_term(yy, nt, m, c);
        }
        const double r = lik.p[0], yy = y(0);
        return negbin_logconst(yy, r) - (yy + r) * kLogTwo + m * (yy - r) / 2.0 - (yy + r) * logcosh_(c / 2.0);
    }
    // logistic noise: the same cancellation at b = 2 with c^2 = ((mu - y)^2 + sigma^2) / s^2
    if (lik.kind == AGPL_LIK_LOGISTIC_NOISE) {
        const double m = mu(0), v = var(0);
        double c, o2, o3;
        lik_aux_posterior_at<double>(lik, 0, y, [&](int) { return m; }, [&](int) { return v; }, c, o2, o3);
        return -log(4.0 * lik.p[0]) - 2.0 * logcosh_(c / 2.0);
    }
    return expected_logtilt_point(lik, y, q1, q2, mu, var) - aux_kl_point(lik, y, q1, q2);
}

struct MargArrays { // marginals latent-major [L][N]
    const float *mu, *var;
    int64_t n;
    __device__ __forceinline__ float m(int k, int64_t i) const { return mu[(int64_t)k * n + i]; }
    __device__ __forceinline__ float v(int k, int64_t i) const { return var[(int64_t)k * n + i]; }
};
struct OutArrays {
    float *gamma, *beta;
    int64_t n;
    __device__ __forceinline__ void put(int k, int64_t i, float g, float b) {
        gamma[(int64_t)k * n + i] = g;
        beta[(int64_t)k * n + i] = b;
    }
};

__global__ __launch_bounds__(kBlock) void agpl_fused_elementwise_kernel(agpl_lik_dev lik, int64_t n, const void *yv,
                                                                        const float *__restrict__ mu,
                                                                        const float *__restrict__ var,
                                                                        float *__restrict__ gamma,
                                                                        float *__restrict__ beta,
                                                                        float *__restrict__ c_out) {
    const MargArrays mg{mu, var, n};
    OutArrays out{gamma, beta, n};
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
        fused_point(lik, i, yv, mg, out, c_out);
}

// The sweep's ONE per-point kernel (image path): the marginal kernel's row-block partial sums -> q(f_i) -> aux_posterior! ->
// expected potential / precision -> the accumulation's gamma | beta records (256 bytes per 32-point step: gamma x 32 |
// beta x 32, zeros beyond N) and max gamma (one atomic per workgroup) -- what marginal_combine_kernel,
// agpl_fused_elementwise_kernel and acc_prep_kernel did in three launches and three round trips through HBM.
struct MargParts {
    const float *resid, *mu0, *qpart, *mpart;
    int64_t n;
    int L, nb2;
    __device__ __forceinline__ float m(int k, int64_t i) const {
        float s = 0.f;
        for (int rb = 0; rb < nb2; ++rb) s += mpart[((int64_t)rb * L + k) * n + i]; // (row blocks in ascending order)
        return mu0 ? s + mu0[(int64_t)k * n + i] : s;
    }
    __device__ __forceinline__ float v(int k, int64_t i) const {
        float q = 0.f;
        for (int rb = 0; rb < nb2; ++rb) q += qpart[((int64_t)rb * L + k) * n + i];
        return resid[i] + q;
    }
};
struct OutRecords {
    float *gamma, *beta; // optional [L][N] copies
    float *gb;
    int64_t n, nrec;     // nrec = records per latent
    unsigned gmax, bad;
    __device__ __forceinline__ void put(int k, int64_t i, float g, float b) {
        if (gamma) gamma[(int64_t)k * n + i] = g;
        if (beta) beta[(int64_t)k * n + i] = b;
        float *rec = gb + ((int64_t)k * nrec + (i >> 5)) * 64 + (i & 31);
        rec[0] = g;
        rec[32] = b;
        const unsigned gbits = __float_as_uint(g), ab = gbits & 0x7FFFFFFFu;
        if (ab >= 0x7F800000u || ((gbits >> 31) && ab != 0u)) bad = max(bad, (unsigned)min((int64_t)0x7FFFFFFE, k * n + i) + 1u);
        else gmax = max(gmax, ab);
    }
};

// ELBO: the instantiation that also sums the ELBO terms (float64 transcendental code: kept out of the plain kernel, whose
// register footprint and 0.13 ms per 1e7 points it would otherwise cost -- 0.47 ms with the branch compiled in, measured)
// (KIND: the likelihood of an ELBO instantiation, so that only its own float64 terms are compiled in; -1: taken from `lik`)
template <bool ELBO, int KIND>
__global__ __launch_bounds__(kBlock) void agpl_fused_point_kernel(agpl_lik_dev lik_arg, int64_t n, int64_t npad, int nb2,
                                                                  const void *yv, const float *__restrict__ resid,
                                                                  const float *__restrict__ mu0,
                                                                  const float *__restrict__ qpart,
                                                                  const float *__restrict__ mpart,
                                                                  float *__restrict__ gamma, float *__restrict__ beta,
                                                                  float *__restrict__ c_out, float *__restrict__ gb,
                                                                  unsigned *__restrict__ scal,
                                                                  unsigned *__restrict__ queues,
                                                                  double *__restrict__ elbo_part) {
    // queues: the marginal kernel's item queues; behind them (agpl_ws2.h) 1 + index of a gamma that is negative or not finite, kept
    // until the update's last kernel forwards it to the host (agpl_pending_resolve reports AGPL_ERR_DOMAIN)
    __shared__ unsigned red[2][kBlock / 64];
    agpl_lik_dev lik = lik_arg;
    if (KIND >= 0) lik.kind = KIND; // (a compile-time constant from here on: the switches over the kind fold)
    const int L = lik.nlatent;
    if (blockIdx.x == 0 && threadIdx.x < kWs2QueueWords) queues[threadIdx.x] = 0u; // the marginal kernel's item queues, for its next launch
    const MargParts mg{resid, mu0, qpart, mpart, n, L, nb2};
    OutRecords out{gamma, beta, gb, n, npad / 32, 0u, 0u};
    double eacc = 0.0; // (elbo_part != nullptr) this thread's ELBO terms, points in ascending order
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < npad; i += (int64_t)gridDim.x * blockDim.x) {
        if (i < n) {
            fused_point(lik, i, yv, mg, out, c_out);
            if (ELBO) eacc += elbo_point(lik, i, yv, mg);
        } else { // the zero tail of the records
            for (int k = 0; k < L; ++k) {
                float *rec = gb + ((int64_t)k * out.nrec + (i >> 5)) * 64 + (i & 31);
                rec[0] = 0.f;
                rec[32] = 0.f;
            }
        }
    }
    unsigned m = out.gmax, b = out.bad;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        m = max(m, (unsigned)__shfl_xor((int)m, o));
        b = max(b, (unsigned)__shfl_xor((int)b, o));
    }
    if ((threadIdx.x & 63) == 0) {
        red[0][threadIdx.x >> 6] = m;
        red[1][threadIdx.x >> 6] = b;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < kBlock / 64; ++w) {
            m = max(m, red[0][w]);
            b = max(b, red[1][w]);
        }
        if (m) atomicMax(scal, m);
        if (b) {
            atomicMax(scal + 1, b);
            atomicMax(queues + kWs2BadGammaWord, b);
        }
    }
    if (ELBO) { // the ELBO rides the pass: fixed-order tree over the workgroup, one partial per workgroup
        __shared__ double esum[kBlock];
        esum[threadIdx.x] = eacc;
        __syncthreads();
        for (int st = kBlock / 2; st > 0; st >>= 1) {
            if ((int)threadIdx.x < st) esum[threadIdx.x] += esum[threadIdx.x + st];
            __syncthreads();
        }
        if (threadIdx.x == 0) elbo_part[blockIdx.x] = esum[0];
    }
}

// internal (agpl_update.hip): the per-point kernel of the image sweep; scal must be zero (the marginal kernel zeroes it)
int32_t agpl_launch_fused_point(agpl_ctx *ctx, const agpl_lik_dev &ld, int64_t n, int64_t npad, int nb2, const void *y,
                                const float *resid, const float *mu0, const float *qpart, const float *mpart,
                                float *gamma, float *beta, float *c_out, float *gb, unsigned *scal, unsigned *queues,
                                double *elbo_terms_out) {
    int64_t nblk = agpl_cdiv(npad, kBlock);
    if (nblk > 1024) nblk = 1024; // (one atomic per workgroup on the max-gamma word)
    double *part = nullptr;
    if (elbo_terms_out) { // the sum over points of expected_logtilt_i - aux_kldivergence_i rides the pass
        if (ld.kind == AGPL_LIK_CATEGORICAL || ld.kind == AGPL_LIK_HETEROGAUSS)
            AGPL_FAIL(ctx, AGPL_ERR_UNSUPPORTED,
                      "the ELBO terms are not defined for this likelihood (categorical.jl:165-170: non-bijective link; "
                      "heteroscedastic: not split in the reference)");
        if (!ctx->elbo_part) {
            AGPL_HIP(ctx, hipMalloc((void **)&ctx->elbo_part, sizeof(double) * 1024));
        }
        part = ctx->elbo_part;
    }
#define AGPL_LAUNCH_FUSED(E_, K_)                                                                               \
    agpl_fused_point_kernel<E_, K_><<<(unsigned)nblk, kBlock, 0, ctx->stream>>>(ld, n, npad, nb2, y, resid, mu0, qpart, mpart, \
                                                                               gamma, beta, c_out, gb, scal, queues, part)
    if (!part) {
        AGPL_LAUNCH_FUSED(false, -1);
    } else {
        const bool launched = lik_switch(ld.kind, [&](auto K) {
            constexpr bool taken = K() != AGPL_LIK_CATEGORICAL && K() != AGPL_LIK_HETEROGAUSS; // (refused above)
            if constexpr (taken) AGPL_LAUNCH_FUSED(true, K());
            return taken;
        });
        if (!launched) AGPL_FAIL(ctx, AGPL_ERR_UNSUPPORTED, "the fused per-point kernel has no ELBO form for likelihood kind %d", ld.kind);
    }
#undef AGPL_LAUNCH_FUSED
    AGPL_LAUNCH_CHECK(ctx);
    if (part) {
        reduce_final_kernel<<<1, 64, 0, ctx->stream>>>((int)nblk, part, elbo_terms_out);
        AGPL_LAUNCH_CHECK(ctx);
    }
    return AGPL_OK;
}

int32_t agpl_launch_fused_elementwise(agpl_ctx *ctx, const agpl_lik_dev &ld, int64_t n, const void *y,
                                      const float *mu, const float *var, float *gamma, float *beta, float *c_out) {
    agpl_fused_elementwise_kernel<<<grid_for(n), kBlock, 0, ctx->stream>>>(ld, n, y, mu, var, gamma, beta, c_out);
    AGPL_LAUNCH_CHECK(ctx);
    return AGPL_OK;
}
