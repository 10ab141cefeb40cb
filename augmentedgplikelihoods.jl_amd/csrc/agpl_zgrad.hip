// agpl_zgrad.hip -- the gradient of the sweep's bound with respect to the inducing inputs at a plan's q(v), and in the same pass
// the gradient for log lengthscales and log variance (agpl_plan_inducing_grad, include/agpl_zgrad.h: the formulae and the
// reduction).  The kernels and the call's body are those of agpl_hyper_impl.h, instantiated with the inducing-input gradient.
#include "../../include/agpl_zgrad.h"
#include "agpl_hyper_impl.h"

extern "C" int32_t agpl_plan_inducing_grad(agpl_plan *p, int64_t N, const double *x, const float *mu0, const float *beta,
                                           const float *gamma, const double *G, const double *g, double *grad_theta_out,
                                           double *grad_z_out) {
    return hy_grad<true>("agpl_plan_inducing_grad", p, N, x, mu0, beta, gamma, G, g, grad_theta_out, grad_z_out);
}
