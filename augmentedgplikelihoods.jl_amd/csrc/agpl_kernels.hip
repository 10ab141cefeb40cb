// agpl_kernels.hip -- libagpl_kernels.so (include/agpl_kernels.h): a plan built straight from raw inputs for any stationary
// covariance function of agpl_kernel_rules.h (squared exponential, Matern-1/2, -3/2, -5/2, rational quadratic).  The build is
// agpl_plan_create_se's (agpl_se_create.h): K_ZZ in float64 with the kind's rule, the whitening factor on the library's float64
// route, then ONE pass of se_build_kernel<kind> (agpl_se_build.h) over the points.  Only the generator's rule differs between the
// kinds: the whitening GEMM, both image layouts, the residual and its clamp, the one scale fixed before anything is written
// (|phi_ai| <= |phi_i| <= sigma holds whenever k(x, x) = variance) and the per-point determinism are the squared exponential's.
// The plans are ordinary: agpl_plan_predict (libagpl_se.so) and agpl_plan_predict_chain (libagpl_chain.so) read the kind from the plan.
#include "../../include/agpl_kernels.h"
#include "agpl_se_create.h"

extern "C" int32_t agpl_plan_create_stationary(agpl_ctx *ctx, int64_t N, int32_t M, int32_t L, int32_t D, int32_t kind, double param,
                                               const double *x, const double *z, const double *lengthscale, double variance,
                                               double jitter, uint32_t flags, void *storage, agpl_plan **plan_out) {
    return agpl_se_create(ctx, N, M, L, D, kind, param, x, z, lengthscale, variance, jitter, flags, storage, plan_out);
}
