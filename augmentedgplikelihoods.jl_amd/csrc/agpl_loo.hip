// agpl_loo.hip -- the leave-one-out cavity of a plan's q(v) at the training points (include/agpl_loo.h).
//
//   agpl_marginals_plan  (libagpl.so) q(f_i) of the plan's q(v) into the work area: the plan's own marginal kernel, unchanged.
//   loo_cavity_kernel    the streaming pass, memory-bound (per pair 16 or 20 bytes read -- mu, var, gamma, beta, mu0 -- and 16 or 24
//                        written, 4 bytes of the residual per point; two float64 divisions).  One lane per point, looping over the
//                        latents: the [L][N] reads of a wave are one coalesced 256-byte stream each; the [N][L] writes of a lane are
//                        L consecutive doubles (strided between lanes for L > 1; not staged).  A workgroup of
//                        kLooThreads lanes strides over tiles of kLooThreads consecutive points.  Per workgroup ONE place each for
//                        the leverage sums (a partial per latent), the count and the lowest index of the pairs without a cavity
//                        (one 64-bit integer atomicAdd / atomicMin, only when there is one).
//   loo_sum_kernel       second level of lev_sum: one workgroup per latent, fixed order (as predictive_sum_kernel of agpl_predictive.hip).
// No float atomics: the bits do not depend on the call.  The file is compiled without contraction (Makefile: NOFMA): every operation
// of the rule is rounded once, in the header's order.
#include "../../include/agpl_loo.h"
#include "agpl_plan_impl.h"

#include <math.h>

namespace {

constexpr int kLooThreads = 256;   // lanes of a workgroup = points of a tile
constexpr int kLooPartials = 1024; // workgroups of the pass at the most = partial sums per latent in the work area
constexpr int kLooMaxL = 64;       // latents a plan takes
constexpr unsigned long long kLooNone = ~0ull;
static_assert(kLooMaxL == 64, "a wave zeroes its kLooMaxL running sums with one store per lane");

struct LooWork {
    float *mu, *var;
    double *part;
};

inline size_t loo_marginal_bytes(int64_t N, int32_t L) { return agpl_align256(sizeof(float) * (size_t)L * (size_t)N); }

inline int64_t loo_bytes(int64_t N, int32_t L) {
    return (int64_t)(2 * loo_marginal_bytes(N, L) + sizeof(double) * (size_t)L * kLooPartials);
}

inline LooWork loo_work(void *work, int64_t N, int32_t L) {
    LooWork w;
    w.mu = (float *)work;
    w.var = (float *)((char *)work + loo_marginal_bytes(N, L));
    w.part = (double *)((char *)work + 2 * loo_marginal_bytes(N, L));
    return w;
}

__device__ __forceinline__ bool loo_finite(float x) { return fabsf(x) <= 3.402823466e38f; }

__global__ __launch_bounds__(kLooThreads) void loo_cavity_kernel(int64_t N, int L, const float *__restrict__ mu,
                                                                 const float *__restrict__ var, const float *__restrict__ resid,
                                                                 const float *__restrict__ mu0, const float *__restrict__ gamma,
                                                                 const float *__restrict__ beta, double *__restrict__ mu_out,
                                                                 double *__restrict__ var_out, double *__restrict__ lev_out,
                                                                 double *__restrict__ part, unsigned long long *__restrict__ info) {
    __shared__ double ws[kLooThreads / 64][kLooMaxL]; // a wave's running leverage sum per latent (touched by that wave only)
    __shared__ unsigned long long scount[kLooThreads / 64], sfirst[kLooThreads / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    ws[wave][lane] = 0.0;
    unsigned long long nbad = 0, first = kLooNone;
    const int64_t ntiles = (N + kLooThreads - 1) / kLooThreads;
    for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const int64_t i = tile * kLooThreads + tid;
        const bool in = i < N;
        const double d = in ? (double)resid[i] : 0.0;
        for (int l = 0; l < L; ++l) {
            double hs = 0.0;
            if (in) {
                const int64_t at = (int64_t)l * N + i;
                const float muf = mu[at], varf = var[at], gf = gamma[at], bf = beta[at];
                const double m0 = mu0 ? (double)mu0[at] : 0.0;
                double mo = NAN, vo = NAN, ho = NAN;
                bool ok = loo_finite(muf) && loo_finite(varf) && loo_finite(gf) && loo_finite(bf) && !(gf < 0.f);
                if (ok) {
                    const double g = (double)gf, b = (double)bf;
                    double q = (double)varf - d;
                    if (!(q > 0.0)) q = 0.0;
                    const double a = (double)muf - m0;
                    const double h = g * q;
                    ok = h < 1.0;
                    if (ok) {
                        const double t = 1.0 - h;
                        vo = d + q / t;
                        const double u = b * q;
                        const double w = a - u;
                        mo = m0 + w / t;
                        ho = h;
                        hs = h;
                    }
                }
                if (!ok) {
                    nbad += 1;
                    first = (unsigned long long)at < first ? (unsigned long long)at : first;
                }
                const int64_t to = i * L + l;
                mu_out[to] = mo;
                var_out[to] = vo;
                if (lev_out) lev_out[to] = ho;
            }
            if (part) {
                for (int o = 32; o > 0; o >>= 1) hs += __shfl_xor(hs, o, 64);
                if (lane == 0) ws[wave][l] += hs;
            }
        }
    }
    for (int o = 32; o > 0; o >>= 1) {
        nbad += __shfl_xor(nbad, o, 64);
        const unsigned long long of = __shfl_xor(first, o, 64);
        first = of < first ? of : first;
    }
    if (lane == 0) {
        scount[wave] = nbad;
        sfirst[wave] = first;
    }
    __syncthreads();
    if (part && tid < L) {
        double t = ws[0][tid];
        for (int w = 1; w < kLooThreads / 64; ++w) t += ws[w][tid];
        part[(int64_t)tid * kLooPartials + blockIdx.x] = t;
    }
    if (info && tid == 0) {
        for (int w = 1; w < kLooThreads / 64; ++w) {
            nbad += scount[w];
            first = sfirst[w] < first ? sfirst[w] : first;
        }
        if (nbad) {
            atomicAdd(info, nbad);
            atomicMin(info + 1, first);
        }
    }
}

// second level of lev_sum: one workgroup per latent, fixed order
__global__ __launch_bounds__(kLooThreads) void loo_sum_kernel(const double *__restrict__ part, int nblk, double *__restrict__ out) {
    __shared__ double red[kLooThreads];
    const double *p = part + (int64_t)blockIdx.x * kLooPartials;
    double t = 0.0;
    for (int b = threadIdx.x; b < nblk; b += kLooThreads) t += p[b];
    red[threadIdx.x] = t;
    __syncthreads();
    for (int st = kLooThreads / 2; st > 0; st >>= 1) {
        if ((int)threadIdx.x < st) red[threadIdx.x] += red[threadIdx.x + st];
        __syncthreads();
    }
    if (threadIdx.x == 0) out[blockIdx.x] = red[0];
}

} // namespace

extern "C" int64_t agpl_plan_loo_bytes(int64_t N, int32_t L) {
    if (N < 1 || L < 1 || L > kLooMaxL) return 0;
    return loo_bytes(N, L);
}

extern "C" int32_t agpl_plan_loo(agpl_plan *p, const float *mu0, const float *gamma, const float *beta, void *work,
                                 int64_t work_bytes, double *mu_out, double *var_out, double *lev_out, double *lev_sum, int64_t *info) {
    if (!p || !p->ctx) return AGPL_ERR_INVALID_ARGUMENT;
    agpl_ctx *ctx = p->ctx;
    if (p->flags & AGPL_PLAN_NO_MARGINALS)
        AGPL_FAIL(ctx, AGPL_ERR_INVALID_ARGUMENT, "this plan was created without the marginal image (AGPL_PLAN_NO_MARGINALS)");
    if (!gamma || !beta) AGPL_FAIL(ctx, AGPL_ERR_INVALID_ARGUMENT, "null gamma / beta: the cavity needs the sites of the plan's q(v)");
    if (!mu_out || !var_out) AGPL_FAIL(ctx, AGPL_ERR_INVALID_ARGUMENT, "null mu_out / var_out");
    int64_t N = 0;
    int32_t L = 0;
    const float *resid = nullptr;
    if (agpl_plan_info(p, &N, nullptr, &L, nullptr, nullptr) || agpl_plan_state(p, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, &resid))
        AGPL_FAIL(ctx, AGPL_ERR_INVALID_ARGUMENT, "the plan does not report its sizes and residual");
    if (!work) AGPL_FAIL(ctx, AGPL_ERR_INVALID_ARGUMENT, "null work area");
    if (work_bytes < loo_bytes(N, L))
        AGPL_FAIL(ctx, AGPL_ERR_INVALID_ARGUMENT, "the work area has %lld bytes, agpl_plan_loo_bytes(%lld, %d) = %lld", (long long)work_bytes,
                  (long long)N, L, (long long)loo_bytes(N, L));
    const LooWork w = loo_work(work, N, L);
    const int32_t rc = agpl_marginals_plan(p, mu0, w.mu, w.var);
    if (rc) return rc;
    if (info) { // {0, -1}: the count to add to, the index to take the minimum with (all ones as unsigned)
        AGPL_HIP(ctx, hipMemsetAsync(info, 0, sizeof(int64_t), ctx->stream));
        AGPL_HIP(ctx, hipMemsetAsync(info + 1, 0xff, sizeof(int64_t), ctx->stream));
    }
    const int64_t tiles = agpl_cdiv(N, kLooThreads);
    const int nblk = (int)(tiles < kLooPartials ? tiles : kLooPartials);
    loo_cavity_kernel<<<(unsigned)nblk, kLooThreads, 0, ctx->stream>>>(N, L, w.mu, w.var, resid, mu0, gamma, beta, mu_out, var_out,
                                                                     lev_out, lev_sum ? w.part : nullptr,
                                                                     reinterpret_cast<unsigned long long *>(info));
    AGPL_LAUNCH_CHECK(ctx);
    if (lev_sum) {
        loo_sum_kernel<<<(unsigned)L, kLooThreads, 0, ctx->stream>>>(w.part, nblk, lev_sum);
        AGPL_LAUNCH_CHECK(ctx);
    }
    return AGPL_OK;
}
