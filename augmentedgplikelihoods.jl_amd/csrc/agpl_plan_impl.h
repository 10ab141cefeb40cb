// agpl_plan_impl.h -- the plan object and its one block of device memory, shared by libagpl.so (agpl_plan.hip) and the
// extensions that create plans from raw inputs, libagpl_se.so (agpl_features.hip) and libagpl_kernels.so (agpl_kernels.hip): plans
// that libagpl.so's entry points then serve.
#pragma once
#include "agpl_common.h"

constexpr int kKlBlocks = 16, kKlWaves = kKlBlocks * 4;

struct agpl_plan {
    agpl_ctx *ctx = nullptr;
    int64_t N = 0;
    int32_t M = 0, L = 0;  // M: the padded count Mp every kernel works on
    int32_t Mc = 0;        // the caller's feature count (<= M)
    double *Gp = nullptr, *gp = nullptr, *eta0p = nullptr, *vp = nullptr; // staging at Mp (Mc != M only)
    uint32_t flags = 0;
    int scale_exp = 0;     // both images hold 2^scale_exp Phi
    char *base = nullptr;  // the plan's device memory
    size_t bytes = 0;
    bool own = false;      // allocated here (storage == NULL at creation)
    // carved out of base
    void *Phi_hi = nullptr, *Phi_lo = nullptr, *Phi_acc = nullptr;
    float *resid = nullptr;
    void *U_hi = nullptr, *U_lo = nullptr;
    double *A_work = nullptr; // [L, M, M]: column-major lower triangle = U
    double *v = nullptr;      // [L, M]
    float *v32 = nullptr;     // [L, M]
    double *logdet = nullptr; // [L] log det(I + G)
    double *klpart = nullptr; // [L][kKlWaves][2] partial sums of the Gaussian KL
    // agpl_plan_create_se / agpl_plan_create_stationary only: what the feature generator reads (carved out of base behind the agpl_plan_bytes part)
    bool se = false;
    int32_t D = 0;
    double s2 = 0.0;          // variance sigma^2
    int32_t kind = 0;         // agpl_kernel_kind (include/agpl_kernels.h): the covariance function the generator evaluates
    double kparam = 0.0;      // its parameter (alpha of the rational quadratic, the period of the periodic kinds and of the cosine factor)
    float *Lt = nullptr;      // [Mp][Mp] float32, Lt[b][a] = L^-1[a][b] (zero for b > a)
    double *zs = nullptr;     // [Mc][D] z / ell
    double *ell = nullptr;    // [D] lengthscales in a block of 32 doubles; a warped or modulated dimension d: [16 + d] = ell_d / period (se_kzz_kernel)
    void *pred = nullptr;     // agpl_plan_predict's chunk scratch (allocated at the first call, freed with the plan)
    size_t pred_bytes = 0;
    double jitter = 0.0;      // the jitter K_ZZ was factored with (read by agpl_plan_hyper_grad, include/agpl_hyper.h)
};

namespace {

constexpr int kUExp = 15; // the plan's U images carry 2^15 U: |U[a][b]| <= 1 always (I + G >= I), so this never overflows float16

struct PlanLayout {
    size_t hi, lo, acc, resid, uhi, ulo, awork, v, v32, logdet, klpart, stage, total;
};
inline int32_t plan_padded(int32_t M) { return (M + 255) / 256 * 256; }
inline size_t agpl_align256(size_t x) { return (x + 255) & ~(size_t)255; }

// The plan's prediction scratch (p->pred), at least `need` bytes: left as it is when it is large enough, else freed behind the
// stream's work and allocated anew.  Every entry point "at new inputs" carves it afresh, so nothing is carried over.  what: the
// scratch's name in the message (a failing wait names this header's line, not the caller's).  Inline: the extension libraries
// share the plan's layout, not a symbol of libagpl.so.
inline int32_t agpl_pred_reserve(agpl_plan *p, size_t need, const char *what) {
    agpl_ctx *ctx = p->ctx;
    if (p->pred_bytes >= need) return AGPL_OK;
    if (p->pred) {
        AGPL_HIP(ctx, hipStreamSynchronize(ctx->stream));
        (void)hipFree(p->pred);
    }
    p->pred = nullptr;
    p->pred_bytes = 0;
    if (hipMalloc(&p->pred, need) != hipSuccess) {
        (void)hipGetLastError();
        p->pred = nullptr;
        AGPL_FAIL(ctx, AGPL_ERR_OUT_OF_MEMORY, "hipMalloc(%zu) for the %s scratch failed", need, what);
    }
    p->pred_bytes = need;
    return AGPL_OK;
}

// M: the padded count; Mc: the caller's
inline PlanLayout plan_layout(int64_t N, int32_t M, int32_t Mc, int32_t L, uint32_t flags) {
    auto al = [](size_t x) { return (x + 255) & ~(size_t)255; };
    PlanLayout o;
    // one of hi / lo; a plan without the marginal image (AGPL_PLAN_NO_MARGINALS: Gibbs sweeps only) keeps none
    const size_t img = (flags & AGPL_PLAN_NO_MARGINALS) ? 0 : (size_t)agpl_split_features_bytes(N, M);
    o.hi = 0;
    o.lo = al(o.hi + img);
    o.acc = al(o.lo + img);
    o.resid = al(o.acc + (size_t)agpl_accumulate_image_bytes(N, M));
    o.uhi = al(o.resid + sizeof(float) * (size_t)N);
    o.ulo = al(o.uhi + sizeof(_Float16) * (size_t)L * M * M);
    o.awork = al(o.ulo + sizeof(_Float16) * (size_t)L * M * M);
    o.v = al(o.awork + sizeof(double) * (size_t)L * M * M);
    o.v32 = al(o.v + sizeof(double) * (size_t)L * M);
    o.logdet = al(o.v32 + sizeof(float) * (size_t)L * M);
    o.klpart = al(o.logdet + sizeof(double) * (size_t)L);
    o.stage = al(o.klpart + sizeof(double) * (size_t)L * kKlWaves * 2);
    // staging of the caller's M-sized natural parameters at the padded size: G [L, M, M], g, eta0, v [L, M] each
    o.total = Mc == M ? o.stage : al(o.stage + sizeof(double) * (size_t)L * ((size_t)M * M + 3 * (size_t)M));
    return o;
}

// extra bytes of a plan made by agpl_plan_create_se (include/agpl_se.h): L^-1 as float32 [Mp][Mp], z / ell as float64 [Mp][D],
// the lengthscales (16 doubles)
inline size_t plan_se_extra(int32_t Mp, int32_t D) {
    auto al = [](size_t x) { return (x + 255) & ~(size_t)255; };
    return al(sizeof(float) * (size_t)Mp * Mp) + al(sizeof(double) * (size_t)Mp * D) + al(sizeof(double) * 16);
}

} // namespace
