"""The float64 CPU reference of ``learn_hyperparameters`` for tests/test_hyper_learn_cpu.py and tests/test_gpu_hyper_learn.py: the
same schedule -- ``nsweeps`` CAVI sweeps (oracle), one gradient (tests/hyper_reference.py, autograd), one Adam step in log space, the
features rebuilt at the new kernel with q(v) = (m, S) carried over -- on 1-D Bernoulli data from the synthetic workload.

The workload's latent is f*(x) = 2 sin(0.7 x) + cos(0.23 x): it is no draw of a GP, and "the generating lengthscale" is taken to be
that of its dominant term, 1 / 0.7 (sin(x / ell) has the curvature scale of a squared-exponential GP of lengthscale ell)."""
import numpy as np

import hyper_reference as HR
import kernels_reference as KR

N, M, SEED = 4096, 32, 5
ELL_GEN = 1.0 / 0.7
ELL0, VAR0, JITTER = 3.0 * ELL_GEN, 4.0, 1e-3
NOUTER, NSWEEPS, LR = 8, 3, 0.15
Z = np.linspace(-10.0, 10.0, M)
# jitter 1e-3: at three times the generating lengthscale the squared-exponential K_ZZ of this grid has condition 6e7 at jitter 1e-6
# (max |L^-1| 6e2), beyond what the plan's float32 whitening takes (its build refuses the features); at 1e-3 it is 1e5.
KIND, KERNEL = KR.SE, "se"


def elbo_of(O, olik, Phi, kd, y, S, m):
    _, _, pts = O.cavi_pass(olik, Phi, kd, y, -S, m, want_points=True)
    mu, var = pts["mu"][:, 0], pts["var"][:, 0]
    q1, q2, _ = O.aux_posterior(olik, y, mu, var)
    Mv = S.shape[-1]
    kl_v = 0.5 * (np.trace(S[0]) + m[0] @ m[0] - Mv - np.linalg.slogdet(S[0])[1])
    return O.expected_logtilt(olik, y, q1, q2, mu, var) - O.aux_kl(olik, y, q1, q2) - kl_v, pts


def reference_loop(O, x, y, ell0=ELL0, var0=VAR0, nouter=NOUTER, nsweeps=NSWEEPS, lr=LR):
    """dict(log_lengthscale [nouter + 1], log_variance [nouter + 1], elbo [nouter]) of the float64 loop (squared exponential, D = 1)."""
    olik = O.bernoulli()
    x2, z2 = np.asarray(x, np.float64).reshape(-1, 1), Z.reshape(-1, 1)
    theta = np.log(np.array([ell0, var0]))
    S, m = np.eye(M)[None], np.zeros((1, M))
    m1, m2 = np.zeros(2), np.zeros(2)
    tr = {"log_lengthscale": [theta[0]], "log_variance": [theta[1]], "elbo": []}
    for it in range(1, nouter + 1):
        ell, s2 = np.exp(theta[:1]), float(np.exp(theta[1]))
        Phi, kd, _ = KR.phi_f64(KIND, x2, z2, ell, s2, JITTER)
        for _ in range(nsweeps):
            G, g = O.cavi_pass(olik, Phi, kd, y, -S, m)
            S, m = O.gaussian_update(G, g)
        e, pts = elbo_of(O, olik, Phi, kd, y, S, m)
        tr["elbo"].append(float(e))
        grad = HR.gradient(KIND, 0.0, x2, z2, ell, s2, JITTER, m, S, pts["beta"], pts["gamma"])["grad"]
        m1, m2 = 0.9 * m1 + 0.1 * grad, 0.999 * m2 + 0.001 * grad * grad
        theta = theta + lr * (m1 / (1 - 0.9 ** it)) / (np.sqrt(m2 / (1 - 0.999 ** it)) + 1e-8)
        tr["log_lengthscale"].append(theta[0])
        tr["log_variance"].append(theta[1])
    return {k: np.array(v) for k, v in tr.items()}
