"""The float64 CPU reference of ``learn_hyperparameters(learn_inducing=True)`` for tests/test_zgrad_learn_cpu.py and
tests/test_gpu_zgrad_learn.py: the schedule of tests/hyper_learn_reference.py -- ``nsweeps`` CAVI sweeps (oracle), one gradient
(autograd: tests/hyper_reference.py for theta, tests/zgrad_reference.py for z), one Adam step on (log lengthscale, log variance, z),
the features rebuilt at the new kernel and the new z with q(v) = (m, S) carried over -- on 1-D Bernoulli data from the synthetic
workload, N = 4096, M = 16.  The inducing inputs start bunched in the first third of the inputs' range [-10, 10], so that moving
them matters: two thirds of the data start without an inducing input nearby."""
import numpy as np

import hyper_learn_reference as LR
import hyper_reference as HR
import kernels_reference as KR
import zgrad_reference as ZR

N, M = 4096, 16
Z0 = np.linspace(-10.0, -10.0 + 20.0 / 3.0, M)
# Matern-3/2 at the generating lengthscale: the bunched start (spacing 0.44 = 0.31 lengthscales) keeps K_ZZ's condition near 1e3,
# which the plan's float32 whitening takes at this jitter
KIND, KERNEL = KR.MATERN32, "matern32"
ELL0, VAR0, JITTER = LR.ELL_GEN, 4.0, 1e-4
NOUTER, NSWEEPS, LR_THETA, LR_Z = 8, 3, 0.15, 0.5


def reference_loop(O, x, y, learn_inducing=True, nouter=NOUTER, nsweeps=NSWEEPS, lr=LR_THETA, lr_z=LR_Z):
    """dict(log_lengthscale [nouter + 1], log_variance [nouter + 1], z [nouter + 1, M, 1], elbo [nouter]) of the float64 loop (D = 1)."""
    olik = O.bernoulli()
    x2 = np.asarray(x, np.float64).reshape(-1, 1)
    par = np.concatenate([np.log([ELL0, VAR0]), Z0])
    step = np.concatenate([[lr, lr], np.full(M, lr_z if learn_inducing else 0.0)])
    S, m = np.eye(M)[None], np.zeros((1, M))
    m1, m2 = np.zeros_like(par), np.zeros_like(par)
    tr = {"log_lengthscale": [par[0]], "log_variance": [par[1]], "z": [par[2:].reshape(M, 1).copy()], "elbo": []}
    for it in range(1, nouter + 1):
        ell, s2, z2 = np.exp(par[:1]), float(np.exp(par[1])), par[2:].reshape(M, 1)
        Phi, kd, _ = KR.phi_f64(KIND, x2, z2, ell, s2, JITTER)
        for _ in range(nsweeps):
            G, g = O.cavi_pass(olik, Phi, kd, y, -S, m)
            S, m = O.gaussian_update(G, g)
        e, pts = LR.elbo_of(O, olik, Phi, kd, y, S, m)
        tr["elbo"].append(float(e))
        args = (KIND, 0.0, x2, z2, ell, s2, JITTER, m, S, pts["beta"], pts["gamma"])
        grad = np.concatenate([HR.gradient(*args)["grad"], ZR.gradient_z(*args)["grad"].reshape(-1)])
        m1, m2 = 0.9 * m1 + 0.1 * grad, 0.999 * m2 + 0.001 * grad * grad
        par = par + step * (m1 / (1 - 0.9 ** it)) / (np.sqrt(m2 / (1 - 0.999 ** it)) + 1e-8)
        tr["log_lengthscale"].append(par[0])
        tr["log_variance"].append(par[1])
        tr["z"].append(par[2:].reshape(M, 1).copy())
    return {k: np.array(v) for k, v in tr.items()}
