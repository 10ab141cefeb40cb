// agpl_hyper.hip -- the gradient of the sweep's bound with respect to log lengthscales and log variance at a plan's q(v)
// (agpl_plan_hyper_grad, include/agpl_hyper.h: the objective, the two parts and their derivation).  The kernels and the call's body
// are stated once in agpl_hyper_impl.h, which libagpl_zgrad.so (agpl_zgrad.hip) shares: this file instantiates them without the
// inducing-input gradient.
#include "agpl_hyper_impl.h"

extern "C" int32_t agpl_plan_hyper_grad(agpl_plan *p, int64_t N, const double *x, const float *mu0, const float *beta,
                                        const float *gamma, const double *G, const double *g, double *grad_out) {
    return hy_grad<false>("agpl_plan_hyper_grad", p, N, x, mu0, beta, gamma, G, g, grad_out, nullptr);
}
