// agpl_features.hip -- a plan's images built straight from the raw inputs of a squared-exponential model (agpl_plan_create_se,
// agpl_plan_predict): the whitened features Phi = L^-1 K_ZX, K_Z + jitter I = L L', are formed tile by tile in registers and LDS
// and leave the kernel only as the plan's split-float16 images and the Nystrom residual -- neither K_ZX nor Phi exists in HBM.
//
//   se_kzz_kernel          K_ZZ + (jitter - 1) I in float64 at Mp (zero beyond the caller's M): the G whose inverse factor
//                          chol(I + G)^-1 the library's float64 route computes is then exactly L^-1 (identity beyond M).
//   se_whitening_kernel    L^-1 (float64 column-major lower triangle) -> float32 [b][a] (the A' operand layout of
//                          agpl_mfma.hip's transform), upper triangle zero; checks the pivots against numerical singularity.
//   se_build_kernel        (agpl_se_build.h, shared with agpl_chain.hip) one 128-point tile per workgroup: for each 128-row block rb of Phi,
//                              Phi[rb] = sum over 16-deep k-slices b < 128 (rb + 1) of L^-1[rb, b] K[b, tile]
//                          on v_mfma_f32_32x32x2_f32 (the zero upper triangle of L^-1 is skipped block-wise: half the flops),
//                          K[b, n] = s2 exp(-|x_n - z_b|^2_ell / 2) generated in the staging step (distance in float64, exp in
//                          float32); the 128 x 128 block goes through LDS once per 64 points and is written as BOTH images in
//                          exactly the layouts of split_features_kernel (agpl_split.hip) and accumulate_image_kernel
//                          (agpl_syrk.hip); |phi_n|^2 and max |phi| ride the epilogue, the residual s2 - |phi_n|^2 is written
//                          with plan_residual_kernel's clamp.  Every value of a point depends on that point's x alone (fixed
//                          k order, fixed reduction order): a point's rows do not depend on N, its position or the launch.
//   se_decode_kernel       features (hi + lo) 2^-e from the accumulate image (agpl_plan_features).
#include "../../include/agpl_se.h"
#include "agpl_plan_impl.h"
#include "agpl_se_build.h"

namespace {

// K_ZZ + (jitter - 1) I at Mp (rows / columns >= Mc zero) and the scaled inducing inputs zs = z / ell; first non-finite z -> words[0],
// first lengthscale that is not positive and finite -> words[4]
__global__ __launch_bounds__(256) void se_kzz_kernel(int Mp, int Mc, int D, const double *__restrict__ z, const double *__restrict__ ell,
                                                     double s2, double jitter, double *__restrict__ G, double *__restrict__ zs,
                                                     unsigned long long *__restrict__ words) {
    if (blockIdx.x == 0 && threadIdx.x == 0)
        for (int d = D - 1; d >= 0; --d)
            if (!(ell[d] > 0.0 && ell[d] <= 1.79e308)) words[4] = (unsigned long long)d; // (first bad lengthscale)
    const int64_t total = (int64_t)Mp * Mp;
    for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (int64_t)gridDim.x * blockDim.x) {
        const int a = (int)(t / Mp), b = (int)(t - (int64_t)a * Mp);
        double v = 0.0;
        if (a < Mc && b < Mc) {
            double r2 = 0.0;
            for (int d = 0; d < D; ++d) {
                const double u = (z[(int64_t)a * D + d] - z[(int64_t)b * D + d]) / ell[d];
                r2 += u * u;
            }
            v = s2 * exp(-0.5 * r2);
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

// out[i][a] = (hi + lo) 2^-e for points i0 .. i0 + n - 1, features a < Mc, from the accumulate image
__global__ __launch_bounds__(256) void se_decode_kernel(int Mp, int Mc, int64_t i0, int64_t n, float inv_scale,
                                                        const _Float16 *__restrict__ blocks, float *__restrict__ out) {
    const int nb = Mp / BS;
    const int64_t total = n * Mc;
    for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (int64_t)gridDim.x * blockDim.x) {
        const int64_t i = t / Mc, pt = i0 + i;
        const int a = (int)(t - i * Mc);
        const int64_t ps = pt >> 4;
        const int plane = (int)((pt >> 3) & 1), j = (int)(pt & 7);
        const int64_t o = ((((ps * nb + a / BS) * 2) * 256 + plane * 128 + (a & 127)) * 8) + j;
        out[t] = ((float)blocks[o] + (float)blocks[o + 256 * 8]) * inv_scale;
    }
}

} // namespace

// ---- launch helpers of the entry points below -------------------------------------------------------------------------------------

// K_ZZ + (jitter - 1) I at Mp into G (float64 [Mp][Mp]) and zs = z / ell (float64 [Mc][D]); words[0] <- first non-finite z
static int32_t agpl_se_kzz(agpl_ctx *ctx, int32_t Mp, int32_t Mc, int32_t D, const double *z, const double *ell, double s2, double jitter,
                    double *G, double *zs, unsigned long long *words) {
    int64_t nblk = agpl_cdiv((int64_t)Mp * Mp, 256);
    if (nblk > 4096) nblk = 4096;
    se_kzz_kernel<<<(unsigned)nblk, 256, 0, ctx->stream>>>(Mp, Mc, D, z, ell, s2, jitter, G, zs, words);
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

static int32_t agpl_se_decode(agpl_ctx *ctx, int32_t Mp, int32_t Mc, int64_t i0, int64_t n, int scale_exp, const void *acc_image, float *out) {
    int64_t nblk = agpl_cdiv(n * Mc, 256);
    if (nblk > 16384) nblk = 16384;
    if (nblk < 1) return AGPL_OK;
    se_decode_kernel<<<(unsigned)nblk, 256, 0, ctx->stream>>>(Mp, Mc, i0, n, ldexpf(1.f, -scale_exp),
                                                             (const _Float16 *)((const unsigned char *)acc_image + 256), out);
    AGPL_LAUNCH_CHECK(ctx);
    return AGPL_OK;
}

// ---- the entry points of include/agpl_se.h ----------------------------------------------------------------------------------------
// They build and read plans with the layout of agpl_plan_impl.h and otherwise reach libagpl.so through its public ABI only
// (agpl_plan_bytes, agpl_gaussian_factor, agpl_plan_update, agpl_marginals_plan, agpl_ctx_synchronize).
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

extern "C" int64_t agpl_plan_se_bytes(int64_t N, int32_t M, int32_t L, int32_t D, uint32_t flags) {
    const int64_t base = agpl_plan_bytes(N, M, L, flags);
    if (!base || D < 1 || D > 16) return 0;
    return base + (int64_t)plan_se_extra(plan_padded(M), D);
}

extern "C" int32_t agpl_plan_create_se(agpl_ctx *ctx, int64_t N, int32_t M, int32_t L, int32_t D, const double *x, const double *z,
                                       const double *lengthscale, double variance, double jitter, uint32_t flags, void *storage,
                                       agpl_plan **plan_out) {
    if (!ctx) return AGPL_ERR_INVALID_ARGUMENT;
    if (!plan_out) AGPL_FAIL(ctx, AGPL_ERR_INVALID_ARGUMENT, "null plan_out");
    *plan_out = nullptr;
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
            snprintf(ctx->err, sizeof(ctx->err), "agpl_plan_create_se: %s failed: %s", #call_, hipGetErrorString(hipGetLastError())); \
            return fail(AGPL_ERR_HIP);                                                                                       \
        }                                                                                                                    \
    } while (0)
    AGPL_SE_TRY(hipMemsetAsync(g, 0, sizeof(double) * M, ctx->stream));
    AGPL_SE_TRY(hipMemsetAsync(words, 0xff, 8 * sizeof(unsigned long long), ctx->stream));
    AGPL_SE_TRY(hipMemsetAsync(maxbits, 0, sizeof(unsigned), ctx->stream));
    AGPL_SE_TRY(hipMemcpyAsync(p->ell, lengthscale, sizeof(double) * D, hipMemcpyDeviceToDevice, ctx->stream));
    rc = agpl_se_kzz(ctx, M, Mc, D, z, p->ell, variance, jitter, G, p->zs, words);
    if (rc) return fail(rc);
    // L^-1 = chol(I + G)^-1 on the library's float64 route (only the float64 factor is taken: |L^-1| is not bounded by 1)
    rc = agpl_gaussian_factor(ctx, M, 1, G, g, nullptr, p->A_work, nullptr, nullptr);
    if (rc) return fail(rc);
    rc = agpl_se_whitening(ctx, M, p->A_work, p->Lt, 16.0 * 2.220446049250313e-16 * Mc * variance, words);
    if (rc) return fail(rc);
    rc = agpl_se_build(ctx, N, M, Mc, D, x, p->zs, p->ell, variance, p->Lt, e, (flags & AGPL_PLAN_NO_MARGINALS) ? nullptr : p->Phi_hi,
                       (flags & AGPL_PLAN_NO_MARGINALS) ? nullptr : p->Phi_lo, p->Phi_acc, p->resid, maxbits, words);
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

namespace {
constexpr int64_t kPredictChunk = 1 << 16; // points per agpl_plan_predict step (images 4 Mp bytes per point)
}

extern "C" int32_t agpl_plan_predict(agpl_plan *p, int64_t Ns, const double *x_s, const float *mu0_s, float *mu_out, float *var_out) {
    if (!p || !p->ctx) return AGPL_ERR_INVALID_ARGUMENT;
    agpl_ctx *ctx = p->ctx;
    if (p->flags & AGPL_PLAN_NO_MARGINALS)
        AGPL_FAIL(ctx, AGPL_ERR_INVALID_ARGUMENT, "this plan was created without the marginal image (AGPL_PLAN_NO_MARGINALS)");
    int32_t rc;
    if (!p->se) AGPL_FAIL(ctx, AGPL_ERR_INVALID_ARGUMENT, "agpl_plan_predict needs a plan made by agpl_plan_create_se");
    if (Ns < 0) AGPL_FAIL(ctx, AGPL_ERR_INVALID_ARGUMENT, "Ns = %lld < 0", (long long)Ns);
    if (Ns == 0) return AGPL_OK;
    if (!x_s || !mu_out || !var_out) AGPL_FAIL(ctx, AGPL_ERR_INVALID_ARGUMENT, "null argument");
    const int L = p->L, M = p->M;
    const int64_t C = Ns < kPredictChunk ? Ns : kPredictChunk;
    auto al = [](size_t v) { return (v + 255) & ~(size_t)255; };
    const size_t img = al((size_t)agpl_split_features_bytes(C, M));
    const size_t io = L > 1 ? al(sizeof(float) * (size_t)L * C) : 0; // [L][C] staging of mu0, mu, var
    const size_t need = 2 * img + al(sizeof(float) * C) + 3 * io + 256;
    if (p->pred_bytes < need) {
        if (p->pred) {
            AGPL_HIP(ctx, hipStreamSynchronize(ctx->stream));
            (void)hipFree(p->pred);
        }
        p->pred = nullptr;
        p->pred_bytes = 0;
        if (hipMalloc(&p->pred, need) != hipSuccess) {
            (void)hipGetLastError();
            p->pred = nullptr;
            AGPL_FAIL(ctx, AGPL_ERR_OUT_OF_MEMORY, "hipMalloc(%zu) for the prediction scratch failed", need);
        }
        p->pred_bytes = need;
    }
    char *w = (char *)p->pred;
    void *Ph = w, *Pl = w + img;
    float *rs = (float *)(w + 2 * img);
    float *m0 = (float *)(w + 2 * img + al(sizeof(float) * C)), *mu = m0 + io / sizeof(float), *var = mu + io / sizeof(float);
    unsigned long long *words = (unsigned long long *)(w + 2 * img + al(sizeof(float) * C) + 3 * io);
    unsigned *maxbits = (unsigned *)(words + 8);
    // the chunk as a plan of its own: the chunk's images and residual, the plan's scale and q(v) -- served by agpl_marginals_plan
    agpl_plan view = *p;
    view.Phi_hi = Ph, view.Phi_lo = Pl, view.resid = rs, view.flags = 0;
    for (int64_t c0 = 0; c0 < Ns; c0 += C) {
        const int64_t n = Ns - c0 < C ? Ns - c0 : C;
        view.N = n;
        rc = agpl_se_build(ctx, n, M, p->Mc, p->D, x_s + c0 * p->D, p->zs, p->ell, p->s2, p->Lt, p->scale_exp, Ph, Pl, nullptr, rs,
                           maxbits, words);
        if (rc) return rc;
        if (L == 1) {
            rc = agpl_marginals_plan(&view, mu0_s ? mu0_s + c0 : nullptr, mu_out + c0, var_out + c0);
            if (rc) return rc;
            continue;
        }
        const size_t row = sizeof(float) * (size_t)n, pitch = sizeof(float) * (size_t)Ns;
        if (mu0_s) AGPL_HIP(ctx, hipMemcpy2DAsync(m0, row, mu0_s + c0, pitch, row, L, hipMemcpyDeviceToDevice, ctx->stream));
        rc = agpl_marginals_plan(&view, mu0_s ? m0 : nullptr, mu, var);
        if (rc) return rc;
        AGPL_HIP(ctx, hipMemcpy2DAsync(mu_out + c0, pitch, mu, row, row, L, hipMemcpyDeviceToDevice, ctx->stream));
        AGPL_HIP(ctx, hipMemcpy2DAsync(var_out + c0, pitch, var, row, row, L, hipMemcpyDeviceToDevice, ctx->stream));
    }
    return AGPL_OK;
}

extern "C" int32_t agpl_plan_features(const agpl_plan *p, int64_t i0, int64_t n, float *Phi_out) {
    if (!p || !p->ctx) return AGPL_ERR_INVALID_ARGUMENT;
    if (i0 < 0 || n < 0 || i0 + n > p->N)
        AGPL_FAIL(p->ctx, AGPL_ERR_INVALID_ARGUMENT, "points [%lld, %lld) outside [0, %lld)", (long long)i0, (long long)(i0 + n),
                  (long long)p->N);
    if (n == 0) return AGPL_OK;
    if (!Phi_out) AGPL_FAIL(p->ctx, AGPL_ERR_INVALID_ARGUMENT, "null argument");
    return agpl_se_decode(p->ctx, p->M, p->Mc, i0, n, p->scale_exp, p->Phi_acc, Phi_out);
}
