// agpl_se_create.h -- a plan built straight from raw inputs, stated once for the two libraries that export it: libagpl_se.so
// (agpl_features.hip: agpl_plan_create_se, the squared exponential) and libagpl_kernels.so (agpl_kernels.hip:
// agpl_plan_create_stationary, every kind of agpl_kernel_rules.h).  Internal: every including source gets its own copy.
//
//   se_kzz_kernel          K_ZZ + (jitter - 1) I in float64 at Mp (zero beyond the caller's M): the G whose inverse factor
//                          chol(I + G)^-1 the library's float64 route computes is then exactly L^-1 (identity beyond M).
//   se_whitening_kernel    L^-1 (float64 column-major lower triangle) -> float32 [b][a] (the A' operand layout of
//                          agpl_mfma.hip's transform), upper triangle zero; checks the pivots against numerical singularity.
//   agpl_se_create         the entry points' body.  It builds plans with the layout of agpl_plan_impl.h and otherwise reaches
//                          libagpl.so through its public ABI only (agpl_gaussian_factor, agpl_plan_update, agpl_ctx_synchronize).
#pragma once
#include "agpl_se_build.h"

namespace {

// K_ZZ + (jitter - 1) I at Mp (rows / columns >= Mc zero) of the covariance function `kind` (float64 throughout; one uniform switch)
// and the scaled inducing inputs zs = z / ell; first non-finite z -> words[0], first lengthscale that is not positive and finite
// -> words[4].  wl: the lengthscales of the distance rule (agpl::kernel_warp; read by a warped kind only): ell itself when z is raw,
// the plan's when z arrives already divided by them and ell is all ones (hy_linv).  wtab (NULL: not written): the plan's lengthscale
// block, whose second half a warped kind fills with the rule's float64 constants, wtab[16 + d] = ell_d / kparam for the dimensions it
// warps (agpl::kernel_dim_warped; agpl_plan_impl.h) or modulates (agpl::kernel_dim_modulated: there wl also feeds the factor).
__global__ __launch_bounds__(256) void se_kzz_kernel(int kind, double kparam, int Mp, int Mc, int D, const double *__restrict__ z,
                                                     const double *ell, const double *wl, double *wtab, double s2, double jitter,
                                                     double *__restrict__ G, double *__restrict__ zs,
                                                     unsigned long long *__restrict__ words) {
    if (blockIdx.x == 0 && threadIdx.x == 0)
        for (int d = D - 1; d >= 0; --d) {
            if (!(ell[d] > 0.0 && ell[d] <= 1.79e308)) words[4] = (unsigned long long)d; // (first bad lengthscale)
            if (wtab && (agpl::kernel_dim_warped(kind, d, D) || agpl::kernel_dim_modulated(kind, d, D))) wtab[16 + d] = ell[d] / kparam;
        }
    const int64_t total = (int64_t)Mp * Mp;
    for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (int64_t)gridDim.x * blockDim.x) {
        const int a = (int)(t / Mp), b = (int)(t - (int64_t)a * Mp);
        double v = 0.0;
        if (a < Mc && b < Mc) {
            double r2 = 0.0, mod = 1.0;
            for (int d = 0; d < D; ++d) {
                const double us = (z[(int64_t)a * D + d] - z[(int64_t)b * D + d]) / ell[d];
                const double u = agpl::kernel_warp_value(kind, d, D, us, wl[d], kparam);
                r2 += u * u;
                if (agpl::kernel_dim_modulated(kind, d, D)) mod = agpl::kernel_modulation(us, wl[d] / kparam);
            }
            v = s2 * agpl::kernel_value<double>(kind, r2, kparam);
            if (agpl::kernel_kind_modulated(kind)) v *= mod; // (the factor of a modulated kind: even in us to the bit, so K_ZZ stays symmetric)
            if (a == b) {
                v += jitter - 1.0;
                for (int d = 0; d < D; ++d) {
                    const double zd = z[(int64_t)a * D + d];
                    if (!(fabs(zd) <= 1.79e308)) atomicMin(&words[0], (unsigned long long)a);
                    zs[(int64_t)a * D + d] = zd / ell[d];
                }
            }
        }
        G[t] = v;
    }
}

// Lt[b][a] = L^-1[a][b] = A[b Mp + a] for a >= b, else 0 (float32).  A pivot r_aa = 1 / L^-1[a][a] with r_aa^2 <= tol (numerically
// singular K_ZZ + jitter I: duplicated inducing inputs and no jitter) -> words[1] = min such a.
__global__ __launch_bounds__(256) void se_whitening_kernel(int Mp, const double *__restrict__ A, float *__restrict__ Lt, double tol,
                                                           unsigned long long *__restrict__ words) {
    const int64_t total = (int64_t)Mp * Mp;
    for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (int64_t)gridDim.x * blockDim.x) {
        const int b = (int)(t / Mp), a = (int)(t - (int64_t)b * Mp);
        const double u = a >= b ? A[t] : 0.0;
        Lt[t] = (float)u;
        if (a == b && !(1.0 / (u * u) > tol)) atomicMin(&words[1], (unsigned long long)a);
    }
}

} // namespace

// K_ZZ + (jitter - 1) I at Mp into G (float64 [Mp][Mp]) and zs = z / ell (float64 [Mc][D]); words[0] <- first non-finite z
static int32_t agpl_se_kzz(agpl_ctx *ctx, int32_t kind, double kparam, int32_t Mp, int32_t Mc, int32_t D, const double *z, const double *ell,
                    const double *wl, double *wtab, double s2, double jitter,
                    double *G, double *zs, unsigned long long *words) {
    int64_t nblk = agpl_cdiv((int64_t)Mp * Mp, 256);
    if (nblk > 4096) nblk = 4096;
    se_kzz_kernel<<<(unsigned)nblk, 256, 0, ctx->stream>>>(kind, kparam, Mp, Mc, D, z, ell, wl, wtab, s2, jitter, G, zs, words);
    AGPL_LAUNCH_CHECK(ctx);
    return AGPL_OK;
}

// float32 [b][a] copy of L^-1 (A: column-major lower triangle); words[1] <- first pivot with r_aa^2 <= tol
static int32_t agpl_se_whitening(agpl_ctx *ctx, int32_t Mp, const double *A, float *Lt, double tol, unsigned long long *words) {
    int64_t nblk = agpl_cdiv((int64_t)Mp * Mp, 256);
    if (nblk > 4096) nblk = 4096;
    se_whitening_kernel<<<(unsigned)nblk, 256, 0, ctx->stream>>>(Mp, A, Lt, tol, words);
    AGPL_LAUNCH_CHECK(ctx);
    return AGPL_OK;
}

namespace {
// agpl_image_scale_exp (agpl_syrk.hip) for a max |phi| whose float32 bit pattern is hmx: 2^e max in [2^13, 2^14)
int32_t se_scale_exp(agpl_ctx *ctx, unsigned hmx, int *e_out) {
    const int ex = (int)(hmx >> 23) - 127;
    int e = 13 - ex;
    if (e > 37 || e < -30) AGPL_FAIL(ctx, AGPL_ERR_DOMAIN, "sigma is outside the range the split-float16 images can be scaled for");
    *e_out = e > 30 ? 30 : e;
    return AGPL_OK;
}
} // namespace

// The body of agpl_plan_create_se (include/agpl_se.h: kind = AGPL_KERNEL_SE) and agpl_plan_create_stationary
// (include/agpl_kernels.h): the plan of the covariance function `kind` with parameter `param`.
static int32_t agpl_se_create(agpl_ctx *ctx, int64_t N, int32_t M, int32_t L, int32_t D, int32_t kind, double param, const double *x,
                              const double *z, const double *lengthscale, double variance, double jitter, uint32_t flags, void *storage,
                              agpl_plan **plan_out) {
    if (!ctx) return AGPL_ERR_INVALID_ARGUMENT;
    if (!plan_out) AGPL_FAIL(ctx, AGPL_ERR_INVALID_ARGUMENT, "null plan_out");
    *plan_out = nullptr;
    if (!agpl::kernel_kind_known(kind)) AGPL_FAIL(ctx, AGPL_ERR_INVALID_ARGUMENT, "unknown kernel kind %d", kind);
    if (const char *what = agpl::kernel_param_refused(kind, param, 1e300, false))
        AGPL_FAIL(ctx, AGPL_ERR_INVALID_ARGUMENT, "param = %g (%s) must be positive and finite", param, what);
    if (!agpl::kernel_has_param(kind)) param = 0.0; // (ignored)
    if (N <= 0 || M <= 0 || M > (1 << 20) || L <= 0 || L > 64 || D < 1 || D > 16)
        AGPL_FAIL(ctx, AGPL_ERR_INVALID_ARGUMENT, "bad sizes N=%lld M=%d L=%d D=%d (1 <= D <= 16)", (long long)N, M, L, D);
    if (!x || !z || !lengthscale) AGPL_FAIL(ctx, AGPL_ERR_INVALID_ARGUMENT, "null argument");
    if (!(variance > 0.0) || !(variance < 1e300)) AGPL_FAIL(ctx, AGPL_ERR_INVALID_ARGUMENT, "variance = %g must be positive and finite", variance);
    if (!(jitter >= 0.0) || !(jitter < 1e300)) AGPL_FAIL(ctx, AGPL_ERR_INVALID_ARGUMENT, "jitter = %g must be >= 0 and finite", jitter);
    if (flags & ~(uint32_t)AGPL_PLAN_NO_MARGINALS) AGPL_FAIL(ctx, AGPL_ERR_INVALID_ARGUMENT, "unknown plan flags 0x%x", flags);
    const int32_t Mc = M;
    M = plan_padded(Mc);
    // ONE scale for both images, before any element is written: |phi_ai| <= |phi_i| <= sigma (Nystrom bound, L^-1 computed here)
    const double smax = sqrt(variance) * (1.0 + 1e-3);
    const float fmax = (float)smax;
    unsigned hmx;
    memcpy(&hmx, &fmax, 4);
    int e = 0;
    int32_t rc = se_scale_exp(ctx, hmx, &e);
    if (rc) return rc;
    const PlanLayout lo = plan_layout(N, M, Mc, L, flags);
    const size_t total = lo.total + plan_se_extra(M, D);
    agpl_plan *p = new agpl_plan;
    p->flags = flags;
    p->ctx = ctx;
    p->N = N;
    p->M = M;
    p->Mc = Mc;
    p->L = L;
    p->scale_exp = e;
    p->bytes = total;
    if (storage) {
        p->base = (char *)storage;
    } else {
        if (hipMalloc((void **)&p->base, total) != hipSuccess) {
            (void)hipGetLastError(); // (a failed allocation leaves a sticky error behind)
            delete p;
            AGPL_FAIL(ctx, AGPL_ERR_OUT_OF_MEMORY, "hipMalloc(%zu) for the plan failed", total);
        }
        p->own = true;
    }
    p->Phi_hi = p->base + lo.hi;
    p->Phi_lo = p->base + lo.lo;
    p->Phi_acc = p->base + lo.acc;
    p->resid = (float *)(p->base + lo.resid);
    p->U_hi = p->base + lo.uhi;
    p->U_lo = p->base + lo.ulo;
    p->A_work = (double *)(p->base + lo.awork);
    p->v = (double *)(p->base + lo.v);
    p->v32 = (float *)(p->base + lo.v32);
    p->logdet = (double *)(p->base + lo.logdet);
    p->klpart = (double *)(p->base + lo.klpart);
    if (Mc != M) {
        p->Gp = (double *)(p->base + lo.stage);
        p->gp = p->Gp + (size_t)L * M * M;
        p->eta0p = p->gp + (size_t)L * M;
        p->vp = p->eta0p + (size_t)L * M;
    }
    p->se = true;
    p->D = D;
    p->s2 = variance;
    p->kind = kind;
    p->kparam = param;
    p->jitter = jitter;
    {
        auto al = [](size_t v) { return (v + 255) & ~(size_t)255; };
        p->Lt = (float *)(p->base + lo.total);
        p->zs = (double *)(p->base + lo.total + al(sizeof(float) * (size_t)M * M));
        p->ell = (double *)((char *)p->zs + al(sizeof(double) * (size_t)M * D));
    }
    // transient: eight status words and max |phi| | G = K_ZZ + (jitter - 1) I [M][M], g = 0 [M] for the whitening factor, then
    // G = 0 [L][Mc][Mc], g = 0 [L][Mc] for the plan's first update (q(v) = N(0, I))
    char *tmp = nullptr;
    const size_t nat = (size_t)L * Mc * Mc + (size_t)L * Mc, fac = (size_t)M * M + M;
    const size_t tmp_bytes = 128 + sizeof(double) * (nat > fac ? nat : fac);
    if (hipMalloc((void **)&tmp, tmp_bytes) != hipSuccess) {
        (void)hipGetLastError();
        if (p->own) (void)hipFree(p->base);
        delete p;
        AGPL_FAIL(ctx, AGPL_ERR_OUT_OF_MEMORY, "hipMalloc(%zu) for the whitening factor failed", tmp_bytes);
    }
    unsigned long long *words = (unsigned long long *)tmp; // [0] z, [1] pivot, [2] x, [3] residual, [4] lengthscale
    unsigned *maxbits = (unsigned *)(words + 8);
    double *G = (double *)(tmp + 128), *g = G + (size_t)M * M;
    auto fail = [&](int32_t code) {
        (void)hipStreamSynchronize(ctx->stream);
        (void)hipFree(tmp);
        if (p->own) (void)hipFree(p->base);
        delete p;
        return code;
    };
#define AGPL_SE_TRY(call_)                                                                                                  \
    do {                                                                                                                     \
        if ((call_) != hipSuccess) {                                                                                         \
            snprintf(ctx->err, sizeof(ctx->err), "plan from inputs: %s failed: %s", #call_, hipGetErrorString(hipGetLastError())); \
            return fail(AGPL_ERR_HIP);                                                                                       \
        }                                                                                                                    \
    } while (0)
    AGPL_SE_TRY(hipMemsetAsync(g, 0, sizeof(double) * M, ctx->stream));
    AGPL_SE_TRY(hipMemsetAsync(words, 0xff, 8 * sizeof(unsigned long long), ctx->stream));
    AGPL_SE_TRY(hipMemsetAsync(maxbits, 0, sizeof(unsigned), ctx->stream));
    AGPL_SE_TRY(hipMemcpyAsync(p->ell, lengthscale, sizeof(double) * D, hipMemcpyDeviceToDevice, ctx->stream));
    rc = agpl_se_kzz(ctx, kind, param, M, Mc, D, z, p->ell, p->ell, p->ell, variance, jitter, G, p->zs, words);
    if (rc) return fail(rc);
    // L^-1 = chol(I + G)^-1 on the library's float64 route (only the float64 factor is taken: |L^-1| is not bounded by 1)
    rc = agpl_gaussian_factor(ctx, M, 1, G, g, nullptr, p->A_work, nullptr, nullptr);
    if (rc) return fail(rc);
    rc = agpl_se_whitening(ctx, M, p->A_work, p->Lt, 16.0 * 2.220446049250313e-16 * Mc * variance, words);
    if (rc) return fail(rc);
    rc = agpl_se_build(ctx, kind, param, N, M, Mc, D, x, p->zs, p->ell, variance, p->Lt, e,
                       (flags & AGPL_PLAN_NO_MARGINALS) ? nullptr : p->Phi_hi, (flags & AGPL_PLAN_NO_MARGINALS) ? nullptr : p->Phi_lo, p->Phi_acc, p->resid, maxbits, words);
    if (rc) return fail(rc);
    // q(v) = N(0, I) to start from (script.jl:41-42): the plan's own update of G = 0, g = 0 (U = I, v = 0, log det = 0 and the
    // U images); A_work held L^-1 until here.  If the whitening factor failed, this call reports it (after the checks below).
    AGPL_SE_TRY(hipMemsetAsync(G, 0, sizeof(double) * nat, ctx->stream));
    const int32_t upd = agpl_plan_update(p, G, G + (size_t)L * Mc * Mc, nullptr, nullptr);
    unsigned long long hw[8];
    unsigned hmax = 0;
    AGPL_SE_TRY(hipMemcpyAsync(hw, words, sizeof(hw), hipMemcpyDeviceToHost, ctx->stream));
    AGPL_SE_TRY(hipMemcpyAsync(&hmax, maxbits, sizeof(hmax), hipMemcpyDeviceToHost, ctx->stream));
#undef AGPL_SE_TRY
    // waits, and collects the outcome of the factorisations (always: the context stays usable)
    const int32_t synced = agpl_ctx_synchronize(ctx);
    const int32_t pend = upd ? upd : synced;
    float realised;
    memcpy(&realised, &hmax, 4);
    if (hw[4] != ~0ull) {
        snprintf(ctx->err, sizeof(ctx->err), "lengthscale[%llu] must be positive and finite", hw[4]);
        return fail(AGPL_ERR_INVALID_ARGUMENT);
    }
    if (hw[0] != ~0ull) {
        snprintf(ctx->err, sizeof(ctx->err), "inducing input z[%llu] is not finite", hw[0]);
        return fail(AGPL_ERR_DOMAIN);
    }
    if (hw[2] != ~0ull) {
        snprintf(ctx->err, sizeof(ctx->err), "input x[%llu] is not finite", hw[2]);
        return fail(AGPL_ERR_DOMAIN);
    }
    if (pend) return fail(pend);
    if (hw[1] != ~0ull) {
        snprintf(ctx->err, sizeof(ctx->err),
                 "K_ZZ + jitter I is numerically singular at pivot %llu (duplicate inducing inputs? add jitter)", hw[1]);
        return fail(AGPL_ERR_NOT_POSDEF);
    }
    if (!(realised <= smax)) {
        snprintf(ctx->err, sizeof(ctx->err), "max |phi| = %g exceeds sigma (1 + 1e-3) = %g: the whitening lost accuracy",
                 (double)realised, smax);
        return fail(AGPL_ERR_DOMAIN);
    }
    if (hw[3] != ~0ull) {
        snprintf(ctx->err, sizeof(ctx->err), "Nystrom residual of point %llu is negative beyond round-off", hw[3]);
        return fail(AGPL_ERR_DOMAIN);
    }
    (void)hipFree(tmp);
    ctx->live_plans += 1;
    *plan_out = p;
    return AGPL_OK;
}
