// agpl_predictive.hip -- libagpl_predictive.so (include/agpl_predictive.h): p(y*) = int p(y* | f) q(f) df per point, its mean and
// variance, log p(y*) of held-out observations and their deterministic sum.  float64, one lane per point (one wave per point for
// the categorical Monte Carlo); the rules and their measured errors are in DESIGN.md 4.10, their numpy twin in
// tools/predictive_twin.py.  Compiled without fused-multiply-add contraction, like agpl_operators.hip.
#include <math.h>

#include "../../include/agpl_predictive.h"
#include "agpl_common.h"
#include "agpl_random.h"

namespace {

constexpr int kBlock = 256;      // lanes per workgroup
constexpr int kMaxBlocks = 1024; // workgroups of one launch = partial sums of logp_sum (ctx->elbo_part holds 1024 doubles)
constexpr int kGrid = 65;        // seed grid over mu +- kSpan s
constexpr int kRecentre = 32;   // times the seed grid may move to a maximum found on its edge
constexpr int kNewton = 48;      // safeguarded Newton steps from the grid's maximum, at most (stopped at kNewtonTol of the width)
constexpr double kNewtonTol = 1e-3;
constexpr int kBracket = 64;     // doublings of the bracket beside the Poisson candidate, at most
constexpr int kMaxHalf = 1024;   // points on each side of the mode in the final trapezoid rule, at most
constexpr int kStNewton = 6;     // Student-t: Newton steps from each of the two starts, each clamped to kStStep
constexpr int kStMaxHalf = 1024; // Student-t: points on each side of the centre, at most
constexpr double kStStep = 2.0;
constexpr double kStDrop = 30.0; // Student-t: the rule ends where the integrand is exp(-30) of its largest value so far
constexpr double kSpan = 8.0;
// Largest spacing of a rule over an integrand with poles at distance pi from the real axis (the logistic's; v(g) = 0 of the
// heteroscedastic likelihood; v(t) = 0 and the Gamma density in t = log x): the trapezoid rule's error is exp(-2 pi pi / spacing)
// of the integral, 7e-18 at 0.5.  s / 4 alone is below it only for s <= 2.
constexpr double kPoleCap = 0.5;
constexpr double kLogSqrt2Pi = 0.91893853320467274178;

} // namespace

// the rules over q(f) themselves (sig_terms, peak_integral, sigma_moments, studentt_logp, laplace_logp, logistic_noise_logp, bad_marginal), shared with
// agpl_quantile.hip: that file includes this one with AGPL_PREDICTIVE_RULES_ONLY defined and so takes the constants above from
// where they are stated, and nothing below
#include "agpl_predictive_rules.h"

#ifndef AGPL_PREDICTIVE_RULES_ONLY
namespace {

// sum of this workgroup's per-lane values in a fixed order -> part[blockIdx.x]
__device__ void block_sum(double v, double *__restrict__ part) {
    __shared__ double red[kBlock];
    red[threadIdx.x] = v;
    __syncthreads();
    for (int st = kBlock / 2; st > 0; st >>= 1) {
        if ((int)threadIdx.x < st) red[threadIdx.x] += red[threadIdx.x + st];
        __syncthreads();
    }
    if (threadIdx.x == 0) part[blockIdx.x] = red[0];
}

template <int KIND>
__global__ __launch_bounds__(kBlock) void predictive_kernel(double p0, double p1, int64_t n, const double *__restrict__ mu,
                                                            const double *__restrict__ var, const void *__restrict__ yv,
                                                            double *__restrict__ mean_out, double *__restrict__ var_out,
                                                            double *__restrict__ logp_out, double *__restrict__ part) {
    // the binomial kinds' trials: p0 for kind 8; the point's own (y [N][2], column 1; NaN outside 1 <= n < 2^22) for kind 11, whose
    // y is therefore never NULL and whose column 0 is read only where a log density is asked for
    constexpr bool kBin = KIND == AGPL_LIK_BINOMIAL || KIND == AGPL_LIK_BINOMIAL_N;
    auto trials = [&](int64_t i) { return KIND == AGPL_LIK_BINOMIAL_N ? agpl::binomial_trials<double>((double)((const int32_t *)yv)[2 * i + 1]) : p0; };
    double lsum = 0.0; // this lane's log densities, points in ascending order
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
        double ey = NAN, vy = NAN, lp = NAN;
        if (!bad) {
            // ---- moments
            if (KIND == AGPL_LIK_BERNOULLI_LOGISTIC || KIND == AGPL_LIK_POISSON || kBin) {
                double e1, e2;
                if (v == 0.0) {
                    e1 = sig_terms(m).sig;
                    e2 = e1 * e1;
                } else {
                    sigma_moments(m, v, e1, e2);
                }
                if (KIND == AGPL_LIK_BERNOULLI_LOGISTIC) {
                    ey = e1;
                    vy = e1 * (1.0 - e1);
                } else if (kBin) { // E[n s (1 - s)] + Var[n s], s = sigma(f)
                    const double nt = trials(i);
                    ey = nt * e1;
                    vy = nt * (e1 - e2) + nt * nt * (e2 - e1 * e1);
                } else {
                    ey = p0 * e1;
                    vy = p0 * e1 + p0 * p0 * (e2 - e1 * e1);
                }
            } else if (KIND == AGPL_LIK_NEGBINOMIAL) {
                const double m1 = exp(m + 0.5 * v), m2 = exp(2.0 * m + 2.0 * v);
                ey = p0 * m1;
                // (m2 >= m1^2: where m2 overflows so does the variance, and inf - inf must not make it NaN)
                vy = isfinite(m2) ? p0 * (m1 + m2) + p0 * p0 * (m2 - m1 * m1) : INFINITY;
            } else if (KIND == AGPL_LIK_STUDENTT) {
                ey = p0 > 1.0 ? m : NAN;
                vy = p0 > 2.0 ? v + p1 * p1 * p0 / (p0 - 2.0) : INFINITY;
            } else if (KIND == AGPL_LIK_LAPLACE) {
                ey = m;
                vy = v + 2.0 * p0 * p0;
            } else if (KIND == AGPL_LIK_ASYMLAPLACE) { // p0 = sigma, p1 = tau
                const double tt = p1 * (1.0 - p1);
                ey = m + p0 * (1.0 - 2.0 * p1) / tt;
                vy = v + p0 * p0 * (1.0 - 2.0 * p1 + 2.0 * p1 * p1) / (tt * tt);
            } else if (KIND == AGPL_LIK_LOGISTIC_NOISE) { // p0 = the scale: Var of Logistic(0, 1) = pi^2 / 3
                ey = m;
                vy = v + p0 * p0 * (agpl::kPi * agpl::kPi / 3.0);
            } else {
                ey = m;
                vy = v + (1.0 + exp(-mg + 0.5 * vg)) / p0;
            }
            // ---- log density of the observation
            if (KIND == AGPL_LIK_BINOMIAL_N ? (logp_out || part) : yv != nullptr) {
                if (KIND == AGPL_LIK_BERNOULLI_LOGISTIC || KIND == AGPL_LIK_NEGBINOMIAL || KIND == AGPL_LIK_POISSON || kBin) {
                    CountLik lik;
                    double c0 = 0.0, y, nt = 0.0;
                    if (KIND == AGPL_LIK_BERNOULLI_LOGISTIC) {
                        y = ((const uint8_t *)yv)[i] ? 1.0 : 0.0;
                        lik = CountLik{y, 1.0 - y, 0.0};
                    } else {
                        y = (double)((const int32_t *)yv)[KIND == AGPL_LIK_BINOMIAL_N ? 2 * i : i];
                        if (KIND == AGPL_LIK_NEGBINOMIAL) {
                            lik = CountLik{y, p0, 0.0};
                            c0 = lgamma(y + p0) - lgamma(y + 1.0) - lgamma(p0);
                        } else if (kBin) { // exponents (y, n - y), constant log C(n, y)
                            nt = trials(i);
                            lik = CountLik{y, nt - y, 0.0};
                            c0 = lgamma(nt + 1.0) - lgamma(y + 1.0) - lgamma(nt - y + 1.0);
                        } else {
                            lik = CountLik{y, 0.0, p0};
                            c0 = y * log(p0) - lgamma(y + 1.0);
                        }
                    }
                    if (KIND == AGPL_LIK_BINOMIAL_N && nt != nt)
                        lp = NAN;
                    else if (y < 0.0 || (kBin && y > nt))
                        lp = -INFINITY;
                    else
                        lp = c0 + (v == 0.0 ? lik.lp(m) : peak_integral(lik, m, v));
                } else if (KIND == AGPL_LIK_STUDENTT) {
                    lp = studentt_logp(p0, p1, ((const double *)yv)[i], m, v);
                } else if (KIND == AGPL_LIK_LAPLACE) {
                    lp = laplace_logp(p0, ((const double *)yv)[i], m, v);
                } else if (KIND == AGPL_LIK_ASYMLAPLACE) {
                    lp = asymlaplace_logp(p0, p1, ((const double *)yv)[i], m, v);
                } else if (KIND == AGPL_LIK_LOGISTIC_NOISE) {
                    lp = logistic_noise_logp(p0, ((const double *)yv)[i], m, v);
                } else {
                    const double y = ((const double *)yv)[i];
                    const HeteroLik lik{v, 1.0 / p0, (y - m) * (y - m)};
                    lp = (vg == 0.0 ? lik.lp(mg) : peak_integral(lik, mg, vg)) - kLogSqrt2Pi;
                }
            }
        }
        if (mean_out) mean_out[i] = ey;
        if (var_out) var_out[i] = vy;
        if (logp_out) logp_out[i] = lp;
        lsum += lp;
    }
    if (part) block_sum(lsum, part);
}

// ---- categorical: Monte Carlo, one wave per point ---------------------------------------------------------------------------
// The wave is cut into 64 / G draw slots of G lanes (G = the power of two >= L): lane (slot, k) draws latent k of draw
// j = j0 + slot from block j of sub-stream 1 + k of the point's Philox stream -- a pure function of (seed, global point, sweep, j, k)
// -- the slot's lanes normalise theta_k sigma(f_k) among themselves (xor butterflies: every lane holds the same sum), each lane
// adds its class's share, and the slots are summed at the end, all in a fixed order.
struct CatParams {
    int32_t L, bij, G;
    double logtheta[65];
};

__device__ __forceinline__ double group_max(double v, int G) {
    for (int o = 1; o < G; o <<= 1) v = fmax(v, __shfl_xor(v, o));
    return v;
}
__device__ __forceinline__ double group_sum(double v, int lo, int hi) {
    for (int o = lo; o < hi; o <<= 1) v += __shfl_xor(v, o);
    return v;
}

__global__ __launch_bounds__(kBlock) void predictive_cat_kernel(CatParams cp, int64_t n, int64_t point_offset, uint64_t seed, uint32_t sweep,
                                                                uint32_t nsamples, const double *__restrict__ mu,
                                                                const double *__restrict__ var, const uint8_t *__restrict__ y,
                                                                double *__restrict__ probs, double *__restrict__ logp_out,
                                                                double *__restrict__ part) {
    __shared__ double red[kBlock / 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int L = cp.L, G = cp.G, K = L + (cp.bij ? 1 : 0);
    const int k = lane & (G - 1), slot = lane / G, nslots = 64 / G;
    const bool live = k < L;
    const double lth = live ? cp.logtheta[k] : 0.0;
    const double lconst = cp.bij ? cp.logtheta[L] - agpl::kLogTwo : -INFINITY; // the last class's constant weight theta_L / 2
    double wsum = 0.0;
    for (int64_t i = (int64_t)blockIdx.x * (kBlock / 64) + wave; i < n; i += (int64_t)gridDim.x * (kBlock / 64)) {
        const double m = live ? mu[i * L + k] : 0.0, v = live ? var[i * L + k] : 0.0;
        const bool bad = __ballot(bad_marginal(m, v)) != 0ull;
        const double s = sqrt(v);
        agpl::Philox base;
        base.init(seed, (uint64_t)(point_offset + i), sweep);
        agpl::Philox g = base.sub(1u + (uint32_t)k);
        double acc = 0.0, accc = 0.0;
        for (uint32_t j0 = 0; j0 < nsamples; j0 += (uint32_t)nslots) {
            const uint32_t j = j0 + (uint32_t)slot;
            g.c0 = j; // block j of the sub-stream: the two uniforms of one normal
            g.pos = 4;
            const double f = m + s * g.normal();
            const double a = live ? lth + sig_terms(f).lsp : -INFINITY;
            const double mx = fmax(group_max(a, G), lconst);
            const double u = live ? exp(a - mx) : 0.0, uc = exp(lconst - mx);
            const double tot = group_sum(u, 1, G) + uc;
            if (j < nsamples) {
                acc += u / tot;
                accc += uc / tot;
            }
        }
        acc = group_sum(acc, G, 64);
        accc = group_sum(accc, G, 64);
        const double pk = bad ? NAN : acc / (double)nsamples, pc = bad ? NAN : accc / (double)nsamples;
        if (probs && slot == 0) {
            if (live) probs[i * K + k] = pk;
            if (cp.bij && lane == 0) probs[i * K + L] = pc;
        }
        if (y) {
            const bool on = live && y[i * L + k] != 0;
            const double obs = group_sum(on ? pk : 0.0, 1, G);
            const bool any = __ballot(on && slot == 0) != 0ull;
            // an all-zero row: class L of the bijective link, no class (probability 0) otherwise
            const double lp = bad ? NAN : log(any ? obs : (cp.bij ? pc : 0.0));
            if (lane == 0) {
                if (logp_out) logp_out[i] = lp;
                wsum += lp;
            }
        }
    }
    if (part) {
        if (lane == 0) red[wave] = wsum;
        __syncthreads();
        if (threadIdx.x == 0) {
            double t = red[0];
            for (int w = 1; w < kBlock / 64; ++w) t += red[w];
            part[blockIdx.x] = t;
        }
    }
}

// second level of logp_sum: one workgroup, fixed order
__global__ __launch_bounds__(kBlock) void predictive_sum_kernel(const double *__restrict__ part, int nblk, double *__restrict__ out) {
    __shared__ double red[kBlock];
    double t = 0.0;
    for (int b = threadIdx.x; b < nblk; b += kBlock) t += part[b];
    red[threadIdx.x] = t;
    __syncthreads();
    for (int st = kBlock / 2; st > 0; st >>= 1) {
        if ((int)threadIdx.x < st) red[threadIdx.x] += red[threadIdx.x + st];
        __syncthreads();
    }
    if (threadIdx.x == 0) *out = red[0];
}

} // namespace

extern "C" AGPL_API int32_t agpl_predictive(agpl_ctx *ctx, const agpl_lik_desc *lik, int64_t n, const double *mu, const double *var,
                                            const void *y, uint32_t nsamples, uint32_t sweep, double *mean_out, double *var_out,
                                            double *logp_out, double *logp_sum) {
    if (!ctx) return AGPL_ERR_INVALID_ARGUMENT;
    AGPL_LIK_CHECK(ctx, lik);
    if (n < 0) AGPL_FAIL(ctx, AGPL_ERR_INVALID_ARGUMENT, "n = %lld < 0", (long long)n);
    if ((logp_out || logp_sum) && !y) AGPL_FAIL(ctx, AGPL_ERR_INVALID_ARGUMENT, "logp_out / logp_sum need the observations y");
    if (lik->kind == AGPL_LIK_BINOMIAL_N && n > 0 && !y)
        AGPL_FAIL(ctx, AGPL_ERR_INVALID_ARGUMENT,
                  "the per-point Binomial's moments need the trials: y (int32 [n][2], column 1 = n_i) may not be NULL");
    const bool cat = lik_is_categorical(lik->kind);
    const double p0 = lik->p[0], p1 = lik->p[1];
    CatParams cp{};
    if (cat) {
        if (nsamples == 0u) nsamples = 4096u;
        if (nsamples < 16u || nsamples > (1u << 20))
            AGPL_FAIL(ctx, AGPL_ERR_INVALID_ARGUMENT, "nsamples = %u: the Monte Carlo rule takes 16 .. 1048576 draws (0 = 4096)", nsamples);
        cp.L = lik->nlatent;
        cp.bij = lik->kind == AGPL_LIK_CATEGORICAL_BIJ;
        cp.G = 1;
        while (cp.G < cp.L) cp.G <<= 1;
        for (int k = 0; k < cp.L + cp.bij; ++k) {
            if (!isfinite(lik->logtheta[k])) AGPL_FAIL(ctx, AGPL_ERR_INVALID_ARGUMENT, "logtheta[%d] is not finite", k);
            cp.logtheta[k] = lik->logtheta[k];
        }
    }
    if (n == 0) {
        if (logp_sum) AGPL_HIP(ctx, hipMemsetAsync(logp_sum, 0, sizeof(double), ctx->stream));
        return AGPL_OK;
    }
    if (!mu || !var) AGPL_FAIL(ctx, AGPL_ERR_INVALID_ARGUMENT, "null mu / var");
    if (!mean_out && !var_out && !logp_out && !logp_sum) return AGPL_OK;
    double *part = nullptr;
    if (logp_sum) {
        if (!ctx->elbo_part) AGPL_HIP(ctx, hipMalloc((void **)&ctx->elbo_part, sizeof(double) * kMaxBlocks));
        part = ctx->elbo_part;
    }
    const int per_block = cat ? kBlock / 64 : kBlock;
    const int64_t want = agpl_cdiv(n, per_block);
    const int nblk = (int)(want < kMaxBlocks ? want : kMaxBlocks);
    const bool launched = agpl::lik_switch(lik->kind, [&](auto K) {
        if constexpr (lik_is_categorical(K()))
            predictive_cat_kernel<<<(unsigned)nblk, kBlock, 0, ctx->stream>>>(cp, n, ctx->point_offset, ctx->seed, sweep, nsamples, mu, var,
                                                                            (const uint8_t *)y, mean_out, logp_out, part);
        else
            predictive_kernel<K()><<<(unsigned)nblk, kBlock, 0, ctx->stream>>>(p0, p1, n, mu, var, y, mean_out, var_out, logp_out, part);
        return true;
    });
    if (!launched) AGPL_FAIL(ctx, AGPL_ERR_INVALID_ARGUMENT, "agpl_predictive: no kernel for likelihood kind %d", lik->kind);
    AGPL_LAUNCH_CHECK(ctx);
    if (logp_sum) {
        predictive_sum_kernel<<<1, kBlock, 0, ctx->stream>>>(part, nblk, logp_sum);
        AGPL_LAUNCH_CHECK(ctx);
    }
    return AGPL_OK;
}
#endif // AGPL_PREDICTIVE_RULES_ONLY
