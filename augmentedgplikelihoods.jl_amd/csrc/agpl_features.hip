// agpl_features.hip -- a plan's images built straight from the raw inputs of a squared-exponential model (agpl_plan_create_se,
// agpl_plan_predict): the whitened features Phi = L^-1 K_ZX, K_Z + jitter I = L L', are formed tile by tile in registers and LDS
// and leave the kernel only as the plan's split-float16 images and the Nystrom residual -- neither K_ZX nor Phi exists in HBM.
//
//   se_kzz_kernel, se_whitening_kernel, agpl_se_create   (agpl_se_create.h, shared with agpl_kernels.hip) the whitening factor
//                          L^-1 and the body of agpl_plan_create_se, which serves every covariance function of agpl_kernel_rules.h.
//   se_build_kernel        (agpl_se_build.h, shared with agpl_chain.hip and agpl_kernels.hip; one instantiation per covariance
//                          function, here for agpl_plan_predict of any plan) one 128-point tile per workgroup: for each 128-row block rb of Phi,
//                              Phi[rb] = sum over 16-deep k-slices b < 128 (rb + 1) of L^-1[rb, b] K[b, tile]
//                          on v_mfma_f32_32x32x2_f32 (the zero upper triangle of L^-1 is skipped block-wise: half the flops),
//                          K[b, n] = s2 kappa(|x_n - z_b|_ell) generated in the staging step (distance in float64, the rule's
//                          exponential in float32; squared exponential: s2 exp(-r^2 / 2)); the 128 x 128 block goes through LDS once per 64 points and is written as BOTH images in
//                          exactly the layouts of split_features_kernel (agpl_split.hip) and accumulate_image_kernel
//                          (agpl_syrk.hip); |phi_n|^2 and max |phi| ride the epilogue, the residual s2 - |phi_n|^2 is written
//                          with plan_residual_kernel's clamp.  Every value of a point depends on that point's x alone (fixed
//                          k order, fixed reduction order): a point's rows do not depend on N, its position or the launch.
//   se_decode_kernel       features (hi + lo) 2^-e from the accumulate image (agpl_plan_features).
#include "../../include/agpl_se.h"
#include "agpl_plan_impl.h"
#include "agpl_se_build.h"
#include "agpl_se_create.h"

namespace {

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
extern "C" int32_t agpl_plan_create_se(agpl_ctx *ctx, int64_t N, int32_t M, int32_t L, int32_t D, const double *x, const double *z,
                                       const double *lengthscale, double variance, double jitter, uint32_t flags, void *storage,
                                       agpl_plan **plan_out) {
    return agpl_se_create(ctx, N, M, L, D, AGPL_KERNEL_SE, 0.0, x, z, lengthscale, variance, jitter, flags, storage, plan_out);
}

extern "C" int64_t agpl_plan_se_bytes(int64_t N, int32_t M, int32_t L, int32_t D, uint32_t flags) {
    const int64_t base = agpl_plan_bytes(N, M, L, flags);
    if (!base || D < 1 || D > 16) return 0;
    return base + (int64_t)plan_se_extra(plan_padded(M), D);
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
    const auto al = agpl_align256;
    const size_t img = al((size_t)agpl_split_features_bytes(C, M));
    const size_t io = L > 1 ? al(sizeof(float) * (size_t)L * C) : 0; // [L][C] staging of mu0, mu, var
    const size_t need = 2 * img + al(sizeof(float) * C) + 3 * io + 256;
    if (int32_t rc_ = agpl_pred_reserve(p, need, "prediction")) return rc_; // (every call carves the scratch anew)
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
        rc = agpl_se_build(ctx, p->kind, p->kparam, n, M, p->Mc, p->D, x_s + c0 * p->D, p->zs, p->ell, p->s2, p->Lt, p->scale_exp, Ph, Pl,
                           nullptr, rs, maxbits, words);
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
