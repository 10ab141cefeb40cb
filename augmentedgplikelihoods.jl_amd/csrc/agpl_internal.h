// agpl_internal.h -- the functions of libagpl.so that cross a translation unit without being part of the C ABI, declared ONCE:
// callers and definers both include this header, so a signature that drifts fails to compile.  (The context's own helpers --
// workspaces, timing, agpl_lik_to_device -- are declared beside agpl_ctx in agpl_common.h.)  Not for libagpl_se.so /
// libagpl_predictive.so: those stay on the public ABI plus agpl_plan_impl.h.
#pragma once
#include "agpl_common.h"

namespace agpl {
// launch geometry of the per-point streaming kernels (agpl_sampler.hip, agpl_operators.hip)
constexpr int kBlock = 256;
inline int grid_for(int64_t n) {
    int64_t b = agpl_cdiv(n, kBlock);
    if (b > 256 * 16) b = 256 * 16; // 256 CUs x 16 resident blocks, grid-stride the rest
    if (b < 1) b = 1;
    return (int)b;
}
} // namespace agpl

// ---- agpl_operators.hip
// the per-point kernel of the image sweep; scal must be zero (the marginal kernel zeroes it)
int32_t agpl_launch_fused_point(agpl_ctx *ctx, const agpl_lik_dev &ld, int64_t n, int64_t npad, int nb2, const void *y,
                                const float *resid, const float *mu0, const float *qpart, const float *mpart,
                                float *gamma, float *beta, float *c_out, float *gb, unsigned *scal, unsigned *queues,
                                double *elbo_terms_out);
int32_t agpl_launch_fused_elementwise(agpl_ctx *ctx, const agpl_lik_dev &ld, int64_t n, const void *y,
                                      const float *mu, const float *var, float *gamma, float *beta, float *c_out);

// ---- agpl_sampler.hip
// Phi == nullptr: the projection reads `image` (the accumulate image of the same features) instead
int32_t agpl_launch_gibbs_project_sample(agpl_ctx *ctx, const agpl_lik_dev &ld, int64_t N, int M, const float *Phi,
                                         const void *image, const float *kdiag, const float *mu0, const void *y, const double *v,
                                         uint32_t sweep, float *gamma, float *beta, double *f_out,
                                         double *omega_out, int64_t *n_out, uint32_t *nuni_out, int *bad,
                                         double *proj_work /* N * L doubles of scratch */);
int32_t agpl_launch_randn(agpl_ctx *ctx, int64_t n, uint32_t sweep, double *out);
int32_t agpl_sampler_outcome(agpl_ctx *ctx, int32_t kind, const int *bad);

// ---- agpl_mfma.hip
size_t agpl_slab_bytes(int64_t N, int32_t M, int32_t L);
// where the gamma | beta records and the two scale words of the image path live in slab_mem
void agpl_accumulate_records(int64_t N, int32_t M, int32_t L, void *slab_mem, float **gb, unsigned **scal);
// records_ready: the caller's per-point kernel has filled agpl_accumulate_records already (image path; beta / gamma unread)
int32_t agpl_accumulate_impl(agpl_ctx *ctx, int64_t N, int32_t M, int32_t L, const float *Phi, const void *acc_image,
                             const float *beta, const float *gamma, double *G_out, double *g_out, void *slab_mem,
                             bool records_ready = false);

// ---- agpl_syrk.hip
int32_t agpl_feature_range_check(agpl_ctx *ctx, int64_t N, int32_t M, const float *Phi, float limit, const char *what,
                                 unsigned *max_bits_out);
int32_t agpl_image_scale_exp(agpl_ctx *ctx, unsigned hmx, int *eA_out);
int32_t agpl_accumulate_image_build(agpl_ctx *ctx, int64_t N, int32_t M, int32_t Msrc, const float *Phi, int eA, unsigned hmx,
                                    void *image_out);
int32_t agpl_syrk_image_launch(agpl_ctx *ctx, int64_t N, int64_t Npad, int32_t M, int32_t L, const void *image,
                               const float *gamma, const float *beta, float *gb, unsigned *scal, float *slabG,
                               float *slabg, int ns, int chunk, int nbig, int small, bool records_ready);

// ---- agpl_split.hip
// the marginal image of scale * Phi (the plan has checked the features and chosen the scale)
int32_t agpl_split_features_build(agpl_ctx *ctx, int64_t N, int32_t M, int32_t Msrc, const float *Phi, float scale, void *Phi_hi,
                                  void *Phi_lo);
int32_t agpl_pack_factor_split_info(agpl_ctx *ctx, int32_t M, int32_t L, const double *A, void *U_hi, void *U_lo,
                                    const int *info, int *info_host, int ninfo, int u_scale_exp);
int32_t agpl_marginals_factor_parts(agpl_ctx *ctx, int64_t N, int32_t M, int32_t L, const void *Phi_hi, const void *Phi_lo,
                                    const void *U_hi, const void *U_lo, const float *v, unsigned *zero2, float **qpart_out,
                                    float **mpart_out, unsigned **queues_out, int image_scale_exp);
int32_t agpl_marginals_factor_internal(agpl_ctx *ctx, int64_t N, int32_t M, int32_t L, const void *Phi_hi, const void *Phi_lo,
                                       const float *resid, const float *mu0, const void *U_hi, const void *U_lo, const float *v,
                                       float *mu_out, float *var_out, int image_scale_exp);

// ---- agpl_factor.hip: U = chol(I + G)^-1 of an M x M block in ONE launch (M <= 1024; the M x M update of the sparse sweep)
int32_t agpl_factor_fused(agpl_ctx *ctx, int32_t M, int32_t L, const double *G, const double *g, const double *eta0,
                          double *T_work, double *A_work, double *v_out, float *v32_out, double *logdet_out,
                          int *info_dev, void *coop_work);
size_t agpl_factor_coop_bytes(int32_t M, int32_t L);

// ---- agpl_dense.hip
// U = chol(I + G)^-1 for 1024 < M <= 2048 as two block rows of the one-launch kernel and four products on the float64 tile
// routine -- no library call
size_t agpl_factor_two_block_bytes(int32_t M);
int32_t agpl_factor_two_block(agpl_ctx *ctx, int32_t M, int32_t L, const double *G, double *T_work, double *A_work, double *logdet_out,
                              int *info_dev, void *work);
int32_t agpl_probe_mfma_f64_impl(agpl_ctx *ctx, int32_t iters, double *tflops_host);

// ---- agpl_update.hip
int32_t agpl_get_rocblas(agpl_ctx *ctx, void **handle_out);
int32_t agpl_cavi_pass_factor_internal(agpl_ctx *ctx, const agpl_lik_desc *lik, int64_t N, int32_t M, const void *Phi_hi,
                                       const void *Phi_lo, const void *acc_image, const float *resid, const float *mu0,
                                       const void *y, const void *U_hi, const void *U_lo, const float *v, double *G_out,
                                       double *g_out, float *c_out, float *gamma_out, float *beta_out, int image_scale_exp,
                                       double *elbo_terms_out);
int32_t agpl_gaussian_factor_async_scaled(agpl_ctx *ctx, int32_t M, int32_t L, const double *G, const double *g,
                                          const double *eta0, double *A_work, double *v_out, float *v32_out, void *U_hi,
                                          void *U_lo, double *logdet_out, int u_scale_exp);
int32_t agpl_gibbs_pass_internal(agpl_ctx *ctx, const agpl_lik_desc *lik, int64_t N, int32_t M, const float *Phi,
                                 const void *acc_image, const float *kdiag, const float *mu0, const void *y,
                                 const double *v, uint32_t sweep, double *G_out, double *g_out, double *f_out, double *omega_out,
                                 int64_t *n_out, uint32_t *nuni_out);
// Feature counts: the caller's M is ANY positive count; a plan works on Mp = M rounded up to a multiple of 256 (zero features
// M .. Mp - 1).  The caller's M-sized arrays pass through the plan's Mp-sized staging copies for M != Mp (agpl_plan.hip).
int32_t agpl_pad_natural(agpl_ctx *ctx, int L, int Mc, int Mp, const double *G, const double *g, const double *e, const double *v,
                         double *Gp, double *gp, double *ep, double *vp);
int32_t agpl_unpad_natural(agpl_ctx *ctx, int L, int Mc, int Mp, const double *Gp, const double *gp, double *G, double *g);
