// agpl_grad.hip -- the posterior of the gradient of f at new inputs (agpl_plan_predict_grad, include/agpl_grad.h).  With
//     psi_d(x) = (ell_d / sqrt c) L^-1 d k_Z(x) / d x_d,      c = -lim kappa'(r) / r at r = 0,     |psi_d|^2 <= sigma^2,
// (c: times u'(0)^2 in a warped dimension, plus (2 pi ell_d / p)^2 in a modulated one: agpl_kernel_rules.h)
// the moments of d f_l / d x_d are those of agpl_plan_predict with psi_d in place of phi, times a constant per dimension:
//     E = (sqrt c / ell_d) psi_d' m_l,      Var = (c / ell_d^2) (sigma^2 - |psi_d|^2 + |U_l psi_d|^2).
//
//   se_build_kernel<kind, true>  (agpl_se_build.h: the plan's generator in its derivative mode) the chunk's marginal image of psi_d at
//                          the plan's own scale and the residual sigma^2 - |psi_d|^2; one launch per (chunk, d).
//   agpl_marginals_plan    (libagpl.so) the marginal pass on a view of the plan that holds the chunk's image: psi' m and the bracket.
//   grad_scale_kernel      dmu[l][d][c0 + i] = (sqrt c / ell_d) mu[l][i],  dvar[l][d][c0 + i] = (c / ell_d^2) var[l][i].
#include "../../include/agpl_grad.h"
#include "agpl_se_build.h"

namespace {

constexpr int64_t kGradChunk = 1 << 16; // points per step (agpl_plan_predict's chunk)

// mu, var [L][n] (the marginal pass of one dimension) -> rows [l][d] of the outputs (pitch D Ns per latent); either output may be NULL
// cmod: the curvature of a modulated dimension's factor (agpl::kernel_modulation_curvature; 0 else): the dimension's c is c + cmod ell_d^2
__global__ __launch_bounds__(256) void grad_scale_kernel(int64_t n, int L, int D, int d, int64_t Ns, int64_t c0, double c, double cmod,
                                                         const double *__restrict__ ell, const float *__restrict__ mu,
                                                         const float *__restrict__ var, float *__restrict__ dmu,
                                                         float *__restrict__ dvar) {
    c += cmod * (ell[d] * ell[d]);
    const float a = (float)(sqrt(c) / ell[d]), b = (float)(c / (ell[d] * ell[d]));
    const int64_t total = (int64_t)L * n;
    for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (int64_t)gridDim.x * blockDim.x) {
        const int64_t l = t / n, i = t - l * n;
        const int64_t o = (l * D + d) * Ns + c0 + i;
        if (dmu) dmu[o] = a * mu[t];
        if (dvar) dvar[o] = b * var[t];
    }
}

} // namespace

extern "C" int32_t agpl_plan_predict_grad(agpl_plan *p, int64_t Ns, const double *x_s, float *dmu_out, float *dvar_out) {
    if (!p || !p->ctx) return AGPL_ERR_INVALID_ARGUMENT;
    agpl_ctx *ctx = p->ctx;
    if (!p->se) AGPL_FAIL(ctx, AGPL_ERR_INVALID_ARGUMENT, "agpl_plan_predict_grad needs a plan made from raw inputs (agpl_plan_create_se, agpl_plan_create_stationary)");
    if (p->flags & AGPL_PLAN_NO_MARGINALS)
        AGPL_FAIL(ctx, AGPL_ERR_INVALID_ARGUMENT, "this plan was created without the marginal image (AGPL_PLAN_NO_MARGINALS)");
    if (Ns < 0) AGPL_FAIL(ctx, AGPL_ERR_INVALID_ARGUMENT, "Ns = %lld < 0", (long long)Ns);
    if (p->kind == AGPL_KERNEL_MATERN12)
        AGPL_FAIL(ctx, AGPL_ERR_UNSUPPORTED, "the Matern-1/2 kernel is not mean-square differentiable: f has no gradient to predict");
    if (Ns == 0) return AGPL_OK;
    if (!x_s || (!dmu_out && !dvar_out)) AGPL_FAIL(ctx, AGPL_ERR_INVALID_ARGUMENT, "null argument");
    const int L = p->L, M = p->M, D = p->D;
    const double c0r = -agpl::kernel_dvalue<double>(p->kind, 0.0, p->kparam); // the rule's own limit at r = 0
    const int64_t C = Ns < kGradChunk ? Ns : kGradChunk;
    const auto al = agpl_align256;
    const size_t img = al((size_t)agpl_split_features_bytes(C, M));
    const size_t io = al(sizeof(float) * (size_t)L * C); // [L][C] of the marginal pass
    const size_t need = 2 * img + al(sizeof(float) * C) + 2 * io + 256;
    if (int32_t rc_ = agpl_pred_reserve(p, need, "prediction")) return rc_; // (every call carves the scratch anew)
    char *w = (char *)p->pred;
    void *Ph = w, *Pl = w + img;
    float *rs = (float *)(w + 2 * img);
    float *mu = (float *)(w + 2 * img + al(sizeof(float) * C)), *var = mu + io / sizeof(float);
    unsigned long long *words = (unsigned long long *)(w + 2 * img + al(sizeof(float) * C) + 2 * io);
    unsigned *maxbits = (unsigned *)(words + 8);
    // the chunk as a plan of its own (agpl_plan_predict's view): the image and residual of psi_d, the plan's scale and q(v)
    agpl_plan view = *p;
    view.Phi_hi = Ph, view.Phi_lo = Pl, view.resid = rs, view.flags = 0;
    for (int64_t c0 = 0; c0 < Ns; c0 += C) {
        const int64_t n = Ns - c0 < C ? Ns - c0 : C;
        view.N = n;
        for (int d = 0; d < D; ++d) {
            const double u0 = agpl::kernel_dwarp_at_zero(p->kind, d, D, p->kparam);
            const double c = c0r * u0 * u0; // (times a warped dimension's u'(0)^2)
            // a modulated dimension: c + cmod ell_d^2, formed on the device where ell_d is (the generator and grad_scale_kernel, the same expression)
            const double cmod = agpl::kernel_modulation_curvature(p->kind, d, D, p->kparam);
            int32_t rc = agpl_se_build_mode<true>(ctx, p->kind, p->kparam, d, 1.0 / sqrt(c), n, M, p->Mc, D, x_s + c0 * D, p->zs, p->ell,
                                                  p->s2, p->Lt, p->scale_exp, Ph, Pl, nullptr, rs, maxbits, words);
            if (rc) return rc;
            rc = agpl_marginals_plan(&view, nullptr, mu, var);
            if (rc) return rc;
            int64_t nblk = agpl_cdiv((int64_t)L * n, 256);
            if (nblk > 4096) nblk = 4096;
            grad_scale_kernel<<<(unsigned)nblk, 256, 0, ctx->stream>>>(n, L, D, d, Ns, c0, c, cmod, p->ell, mu, var, dmu_out, dvar_out);
            AGPL_LAUNCH_CHECK(ctx);
        }
    }
    return AGPL_OK;
}
