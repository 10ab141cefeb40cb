// agpl_sample_y.hip -- libagpl_sampley.so (include/agpl_sample_y.h): draws of the observable y ~ p(y | f) from a block of function
// draws F [T][L][ldf].  One lane per (draw, point), points fastest, one kernel instantiation per likelihood kind; every draw has
// its own Philox sub-stream, so a value does not depend on the launch geometry.  The rules and the order in which they consume
// the stream are stated in the header, their numpy twin is tests/sample_y_reference.py; DESIGN.md 4.19.  Compiled without
// fused-multiply-add contraction, like agpl_predictive.hip.
#include <math.h>

#include "../../include/agpl_sample_y.h"
#include "agpl_common.h"
#include "agpl_random.h"

namespace {

constexpr int kBlock = 256;               // lanes per workgroup
constexpr int kSampleYMaxBlocks = 2048;   // workgroups of one launch (256 CUs x 8): beyond kSampleYMaxBlocks x kBlock draws the lanes stride
constexpr int32_t kMaxDrawEnd = (1 << 24) - 2; // draw0 + T at most: the sub-stream id 1 + draw has 24 bits
constexpr double kCountMax = 2147483647.0;

struct SyParams {
    int32_t L, bij;
    double p0, p1;
    double theta[65]; // categorical: exp(logtheta[k]); theta[L] of the bijective link is its constant weight theta_L / 2
};

template <int KIND>
struct YType {
    using type = double;
};
template <>
struct YType<AGPL_LIK_NEGBINOMIAL> {
    using type = int32_t;
};
template <>
struct YType<AGPL_LIK_POISSON> {
    using type = int32_t;
};
template <>
struct YType<AGPL_LIK_BINOMIAL> {
    using type = int32_t;
};
template <>
struct YType<AGPL_LIK_BERNOULLI_LOGISTIC> {
    using type = uint8_t;
};
template <>
struct YType<AGPL_LIK_CATEGORICAL> {
    using type = uint8_t;
};
template <>
struct YType<AGPL_LIK_CATEGORICAL_BIJ> {
    using type = uint8_t;
};

// the "no observation" value of agpl_predictive: NaN, -1 or 255
template <typename Y>
__device__ __forceinline__ Y no_observation() {
    if constexpr (sizeof(Y) == 8) return (Y)NAN;
    return sizeof(Y) == 4 ? (Y)-1 : (Y)255;
}

__device__ __forceinline__ int32_t count_draw(agpl::Philox &g, double rate) {
    if (rate >= kCountMax) return 2147483647;
    const int64_t k = agpl::rand_poisson(g, rate);
    return k > 2147483647ll ? 2147483647 : (int32_t)k;
}

// y ~ Binomial(n, p), the header's rule: up to kBinomialDirect trials the sum of n comparisons; beyond, on q = min(p, 1 - p) (the
// result mirrored for p > 1/2), the inverse-cdf walk from 0 while n q < kBinomialWalk and Hormann's transformed rejection BTRS from there
constexpr double kBinomialDirect = 64.0, kBinomialWalk = 10.0;
__device__ int32_t binomial_draw(agpl::Philox &g, double n, double p) {
    if (n <= kBinomialDirect) {
        int32_t y = 0;
        for (int j = 0; j < (int)n; ++j) y += g.u01() < p ? 1 : 0;
        return y;
    }
    const bool flip = p > 0.5;
    const double q = flip ? 1.0 - p : p;
    double k;
    if (n * q < kBinomialWalk) {
        const double s = q / (1.0 - q), a = (n + 1.0) * s;
        double r = exp(n * log1p(-q)), u = g.u01();
        k = 0.0;
        while (u > r && k < n) {
            u -= r;
            k += 1.0;
            r *= a / k - s;
        }
    } else {
        const double spq = sqrt(n * q * (1.0 - q)), b = 1.15 + 2.53 * spq, a = -0.0873 + 0.0248 * b + 0.01 * q, c = n * q + 0.5;
        const double vr = 0.92 - 4.2 / b, alpha = (2.83 + 5.1 / b) * spq, lpq = log(q / (1.0 - q)), m = floor((n + 1.0) * q);
        const double h = lgamma(m + 1.0) + lgamma(n - m + 1.0);
        for (;;) {
            const double U = g.u01() - 0.5, V = g.u01(), us = 0.5 - fabs(U);
            k = floor((2.0 * a / us + b) * U + c);
            if (k < 0.0 || k > n) continue;
            if (us >= 0.07 && V <= vr) break;
            if (log(V * alpha / (a / (us * us) + b)) <= h - lgamma(k + 1.0) - lgamma(n - k + 1.0) + (k - m) * lpq) break;
        }
    }
    return (int32_t)(flip ? n - k : k);
}

// step = (gridDim.x * kBlock) as (step_t draws, step_i points): the lanes walk (t, i) without a 64-bit division per element
template <int KIND>
__global__ __launch_bounds__(kBlock) void sample_y_kernel(SyParams sp, int32_t T, int64_t Ns, int64_t ldf, const float *__restrict__ F,
                                                          uint64_t seed, uint64_t gpoint0, uint32_t draw0, uint32_t sweep,
                                                          int64_t step_t, int64_t step_i, void *__restrict__ yv) {
    using Y = typename YType<KIND>::type;
    constexpr bool kCat = KIND == AGPL_LIK_CATEGORICAL || KIND == AGPL_LIK_CATEGORICAL_BIJ;
    Y *__restrict__ y = (Y *)yv;
    const int L = kCat ? sp.L : (KIND == AGPL_LIK_HETEROGAUSS ? 2 : 1);
    const int64_t e0 = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    int64_t t = e0 / Ns, i = e0 - t * Ns;
    for (; t < (int64_t)T;) {
        const float *__restrict__ fp = F + (t * L) * ldf + i;
        const int64_t o = t * Ns + i;
        agpl::Philox base;
        base.init(seed, gpoint0 + (uint64_t)i, sweep);
        agpl::Philox g = base.sub(1u + draw0 + (uint32_t)t);
        if (kCat) {
            double tot = KIND == AGPL_LIK_CATEGORICAL_BIJ ? sp.theta[L] : 0.0;
            bool bad = false;
            for (int k = 0; k < L; ++k) {
                const double f = (double)fp[k * ldf];
                bad = bad || !isfinite(f);
                tot += sp.theta[k] * agpl::logistic(f);
            }
            const double u = g.u01() * tot;
            double cum = 0.0;
            int cls = L; // falls through to the implicit class
            for (int k = 0; k < L; ++k) { // (no early exit: k stays wave-uniform, theta[k] a scalar load)
                cum += sp.theta[k] * agpl::logistic((double)fp[k * ldf]);
                if (cls == L && u < cum) cls = k;
            }
            if (KIND == AGPL_LIK_CATEGORICAL && cls == L) cls = L - 1;
            for (int k = 0; k < L; ++k) y[o * L + k] = bad ? (uint8_t)255 : (uint8_t)(k == cls ? 1 : 0);
        } else {
            const double f = (double)fp[0];
            bool bad = !isfinite(f);
            double fg = 0.0;
            if (KIND == AGPL_LIK_HETEROGAUSS) {
                fg = (double)fp[ldf];
                bad = bad || !isfinite(fg);
            }
            if (bad) {
                y[o] = no_observation<Y>();
            } else if (KIND == AGPL_LIK_BERNOULLI_LOGISTIC) {
                y[o] = g.u01() < agpl::logistic(f) ? 1 : 0;
            } else if (KIND == AGPL_LIK_POISSON) {
                y[o] = (Y)count_draw(g, sp.p0 * agpl::logistic(f));
            } else if (KIND == AGPL_LIK_NEGBINOMIAL) {
                const double a = agpl::rand_gamma(g, sp.p0);
                y[o] = (Y)count_draw(g, a * exp(f));
            } else if (KIND == AGPL_LIK_BINOMIAL) {
                y[o] = (Y)binomial_draw(g, sp.p0, agpl::logistic(f));
            } else if (KIND == AGPL_LIK_STUDENTT) {
                const double z = g.normal();
                const double ch = 2.0 * agpl::rand_gamma(g, sp.p0 / 2.0);
                y[o] = (Y)(f + sp.p1 * z / sqrt(ch / sp.p0));
            } else if (KIND == AGPL_LIK_LAPLACE) {
                const double d = g.u01() - 0.5;
                const double sgn = d > 0.0 ? 1.0 : (d < 0.0 ? -1.0 : 0.0);
                y[o] = (Y)(f - sp.p0 * sgn * log1p(-2.0 * fabs(d)));
            } else if (KIND == AGPL_LIK_ASYMLAPLACE) { // the header's rule: the inverse cdf, p0 = sigma, p1 = tau
                const double d = g.u01() - sp.p1;
                y[o] = (Y)(d < 0.0 ? f + sp.p0 * log1p(d / sp.p1) / (1.0 - sp.p1) : f - sp.p0 * log1p(-d / (1.0 - sp.p1)) / sp.p1);
            } else if (KIND == AGPL_LIK_LOGISTIC_NOISE) { // the header's rule: the inverse cdf of Logistic(0, 1), p0 = the scale
                const double u = g.u01();
                y[o] = (Y)(f + sp.p0 * (log(u) - log1p(-u)));
            } else {
                const double z = g.normal();
                y[o] = (Y)(f + z / sqrt(sp.p0 * agpl::logistic(fg)));
            }
        }
        t += step_t;
        i += step_i;
        if (i >= Ns) {
            i -= Ns;
            t += 1;
        }
    }
}

} // namespace

extern "C" AGPL_API int32_t agpl_sample_y(agpl_ctx *ctx, const agpl_lik_desc *lik, int32_t T, int64_t Ns, int64_t ldf, const float *F,
                                          int64_t point0, int32_t draw0, uint32_t sweep, void *y_out) {
    if (!ctx) return AGPL_ERR_INVALID_ARGUMENT;
    AGPL_LIK_CHECK(ctx, lik);
    if (lik->kind == AGPL_LIK_BINOMIAL_N)
        AGPL_FAIL(ctx, AGPL_ERR_INVALID_ARGUMENT,
                  "draws of the per-point Binomial need the trials n_i, which agpl_sample_y has no argument for: draw with "
                  "AGPL_LIK_BINOMIAL per group of equal n");
    if (T < 0 || Ns < 0 || ldf < Ns)
        AGPL_FAIL(ctx, AGPL_ERR_INVALID_ARGUMENT, "need T >= 0, Ns >= 0, ldf >= Ns (T = %d, Ns = %lld, ldf = %lld)", T, (long long)Ns, (long long)ldf);
    if (draw0 < 0 || draw0 > kMaxDrawEnd - T)
        AGPL_FAIL(ctx, AGPL_ERR_INVALID_ARGUMENT, "need 0 <= draw0 and draw0 + T <= %d (draw0 = %d, T = %d)", kMaxDrawEnd, draw0, T);
    SyParams sp{};
    sp.L = lik->nlatent;
    sp.p0 = lik->p[0], sp.p1 = lik->p[1];
    if (lik_is_categorical(lik->kind)) {
        sp.bij = lik->kind == AGPL_LIK_CATEGORICAL_BIJ;
        for (int k = 0; k < sp.L + sp.bij; ++k) {
            if (!isfinite(lik->logtheta[k])) AGPL_FAIL(ctx, AGPL_ERR_INVALID_ARGUMENT, "logtheta[%d] is not finite", k);
            sp.theta[k] = exp(lik->logtheta[k]);
        }
        if (sp.bij) sp.theta[sp.L] *= 0.5; // categorical.jl:12-14
    }
    if (T == 0 || Ns == 0) return AGPL_OK;
    if (!F || !y_out) AGPL_FAIL(ctx, AGPL_ERR_INVALID_ARGUMENT, "null F / y_out");
    if (Ns > INT64_MAX / ((int64_t)T * sp.L) || ldf > INT64_MAX / ((int64_t)T * sp.L))
        AGPL_FAIL(ctx, AGPL_ERR_INVALID_ARGUMENT, "T L ldf overflows a 64-bit index");
    const int64_t total = (int64_t)T * Ns, want = agpl_cdiv(total, kBlock);
    const int nblk = (int)(want < kSampleYMaxBlocks ? want : kSampleYMaxBlocks);
    const int64_t step = (int64_t)nblk * kBlock, step_t = step / Ns, step_i = step - step_t * Ns;
    const uint64_t gpoint0 = (uint64_t)(ctx->point_offset + point0);
    const bool launched = agpl::lik_switch(lik->kind, [&](auto K) {
        constexpr bool taken = K() != AGPL_LIK_BINOMIAL_N; // (refused above)
        if constexpr (taken)
            sample_y_kernel<K()><<<(unsigned)nblk, kBlock, 0, ctx->stream>>>(sp, T, Ns, ldf, F, ctx->seed, gpoint0, (uint32_t)draw0, sweep, step_t, step_i, y_out);
        return taken;
    });
    if (!launched) AGPL_FAIL(ctx, AGPL_ERR_INVALID_ARGUMENT, "agpl_sample_y: no kernel for likelihood kind %d", lik->kind);
    AGPL_LAUNCH_CHECK(ctx);
    return AGPL_OK;
}
