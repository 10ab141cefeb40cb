"""Float64 numpy reference of the periodic kernel (include/agpl_kernels.h: AGPL_KERNEL_PERIODIC = 6, param = the period p),

    k(x, x') = s2 exp(-1/2 sum_d (sin(pi (x_d - x'_d) / p) / ell_d)^2),

for tests/test_periodic_reference_cpu.py and tests/test_gpu_periodic.py: k, K_ZZ, the whitened features, the derivatives for
log ell, z and x, and the weights of the kernel's (discrete) spectral measure.  No GPU, no library code: nothing here imports the
package."""
import numpy as np

KIND = 6
JITTER = 1e-8
PERIODS = (1.0, 2.5)
NS = (1, 255, 777)
# (D, M, ell): few harmonics are significant when ell is large (D = 1, ell = 1.5: numerical rank about 10), so the cases keep ell = 0.3
CASES = [(1, 16, 0.3), (3, 64, 0.3), (3, 200, 0.3)]


def warp(a, b, ell, p):
    """u [n, m, D] = sin(pi (a_d - b_d) / p) / ell_d and du [n, m, D] = d u / d a_d."""
    d = np.asarray(a, np.float64)[:, None, :] - np.asarray(b, np.float64)[None, :, :]
    ell = np.asarray(ell, np.float64)
    return np.sin(np.pi * d / p) / ell, (np.pi / p) * np.cos(np.pi * d / p) / ell


def kernel(a, b, ell, s2, p):
    u, _ = warp(a, b, ell, p)
    return s2 * np.exp(-0.5 * (u * u).sum(-1))


def dkernel_dlogell(a, b, ell, s2, p):
    """[D, n, m]: d k / d log ell_d = k u_d^2 (the identity -(kappa'(r) / r) u_d^2 with kappa'(r) / r = -kappa)."""
    u, _ = warp(a, b, ell, p)
    k = s2 * np.exp(-0.5 * (u * u).sum(-1))
    return np.moveaxis(k[..., None] * u * u, -1, 0)


def dkernel_da(a, b, ell, s2, p):
    """[D, n, m]: d k(a, b) / d a_d = -k u_d u'_d (d / d b_d is its negative)."""
    u, du = warp(a, b, ell, p)
    k = s2 * np.exp(-0.5 * (u * u).sum(-1))
    return np.moveaxis(-k[..., None] * u * du, -1, 0)


def factor(z, ell, s2, p, jitter=JITTER):
    Kzz = kernel(z, z, ell, s2, p) + jitter * np.eye(len(z))
    Lc = np.linalg.cholesky(Kzz)
    return Kzz, np.linalg.solve(Lc, np.eye(len(z)))


def phi_f64(x, z, ell, s2, p, jitter=JITTER):
    """Phi [N, M] = (L^-1 K_ZX)', the residual s2 - |phi|^2, L^-1."""
    _, Linv = factor(z, ell, s2, p, jitter)
    Phi = (Linv @ kernel(z, x, ell, s2, p)).T
    return Phi, np.maximum(s2 - (Phi * Phi).sum(1), 0.0), Linv


def dphi_dx(x, z, ell, s2, p, jitter=JITTER):
    """[D, N, M]: d phi(x_n) / d x_nd."""
    _, Linv = factor(z, ell, s2, p, jitter)
    return np.einsum("ab,dnb->dna", Linv, dkernel_da(x, z, ell, s2, p))


def workload(N, M, D, ell, p, seed=5):
    """x over several periods, z distinct within ONE period (a jittered grid in D = 1, uniform draws else), lengthscales ell
    (D = 3: ell, 1.2 ell, 1.5 ell)."""
    rng = np.random.default_rng(seed + 7 * M + D)
    x = rng.uniform(-2.0 * p, 3.0 * p, size=(N, D))
    if D == 1:
        z = ((np.arange(M) + 0.5 + 0.2 * rng.uniform(-1, 1, M)) * (p / M))[:, None]
    else:
        z = rng.uniform(0.0, p, size=(M, D))
    ells = ell * np.array([1.0, 1.2, 1.5][:D])
    return x, z, ells


def spectral_weights(ell, kmax=400):
    """w[k] = e^-a I_k(a), k = 0 ... kmax, a = 1 / (4 ell^2): the cosine series' coefficients by direct quadrature of
    (1 / pi) int_0^pi e^{a (cos t - 1)} cos(k t) dt (trapezoid on a periodic integrand: spectrally accurate), independent of the
    recurrence the package uses."""
    a = 1.0 / (4.0 * ell * ell)
    n = 8192
    t = (np.arange(n) + 0.5) * (np.pi / n)
    g = np.exp(a * (np.cos(t) - 1.0))
    return np.array([(g * np.cos(k * t)).mean() for k in range(kmax + 1)])


def bound_gradients(x, z, ell, s2, p, jitter, m, S, beta, gamma):
    """The sweep's bound Lb (tests/hyper_reference.py: _bound) for this kernel and its analytic gradients: ``theta`` [D + 1] for
    (log ell, log s2) and ``z`` [M, D], each with its scale, the sum of the absolute values of the terms it adds up (the yardstick
    of tests/test_gpu_hyper_grad.py and tests/test_gpu_zgrad.py), and ``auto_theta`` / ``auto_z``: the same two by autograd through
    the whole bound, which tests/test_periodic_reference_cpu.py holds the analytic ones against.  dLb / dk_ZX and dLb / dK_ZZ come
    from autograd on detached leaves, as in hyper_reference.gradient; the kernel's derivatives are the closed forms above."""
    import torch

    import hyper_reference as HR

    t = lambda a: torch.as_tensor(np.asarray(a, np.float64))
    M, D = z.shape
    kzx = t(kernel(z, x, ell, s2, p)).requires_grad_(True)
    Kzz0 = kernel(z, z, ell, s2, p)
    Kzz = t(Kzz0 + jitter * np.eye(M)).requires_grad_(True)
    Wk, Kbar = torch.autograd.grad(HR._bound(kzx, Kzz, t(s2), t(m), t(S), t(beta), t(gamma), None), (kzx, Kzz))
    Wk, Kbar = Wk.numpy(), 0.5 * (Kbar + Kbar.T).numpy()
    off = 1.0 - np.eye(M)
    gx, gz = dkernel_dlogell(z, x, ell, s2, p), dkernel_dlogell(z, z, ell, s2, p) * off
    theta, sc_theta = np.zeros(D + 1), np.zeros(D + 1)
    for d in range(D):
        tx, tz = Wk * gx[d], Kbar * gz[d]
        theta[d], sc_theta[d] = tx.sum() + tz.sum(), np.abs(tx).sum() + np.abs(tz).sum()
    tx, tz, tv = Wk * kzx.detach().numpy(), Kbar * Kzz0, -0.5 * np.asarray(gamma, np.float64) * s2
    theta[D], sc_theta[D] = tx.sum() + tz.sum() + tv.sum(), np.abs(tx).sum() + np.abs(tz).sum() + np.abs(tv).sum()
    dzx, dzz = dkernel_da(z, x, ell, s2, p), dkernel_da(z, z, ell, s2, p)  # [D, M, N], [D, M, M]: d / d z_ad of row a
    gzs, sc_z = np.zeros((M, D)), np.zeros((M, D))
    for d in range(D):
        tx, tz = Wk * dzx[d], 2.0 * Kbar * dzz[d] * off
        gzs[:, d], sc_z[:, d] = tx.sum(1) + tz.sum(1), np.abs(tx).sum(1) + np.abs(tz).sum(1)
    # autograd through everything
    th = torch.cat([t(ell).log(), torch.tensor([np.log(s2)], dtype=torch.float64)]).requires_grad_(True)
    zt = t(z).clone().requires_grad_(True)

    def k_t(a, b):
        u = torch.sin(np.pi * (a[:, None, :] - b[None, :, :]) / p) / th[:D].exp()
        return th[D].exp() * torch.exp(-0.5 * (u * u).sum(-1))

    val = HR._bound(k_t(zt, t(x)), k_t(zt, zt) + jitter * torch.eye(M, dtype=torch.float64), th[D].exp(), t(m), t(S), t(beta), t(gamma), None)
    a_th, a_z = torch.autograd.grad(val, (th, zt))
    return dict(theta=theta, scale_theta=sc_theta, z=gzs, scale_z=sc_z, auto_theta=a_th.numpy(), auto_z=a_z.numpy())


def greedy_pivots(x, M, ell, s2, p):
    """The pivoted Cholesky of K_XX in float64: the pivots (ties to the lowest index) and, per step after the first (where every
    prior variance ties), the margin between the best and the second-best conditional variance."""
    n = len(x)
    d = np.full(n, float(s2))
    cols = np.zeros((M, n))
    piv, margins = [], []
    for j in range(M):
        i = int(np.argmax(d))
        if j > 0:
            top = np.sort(d)[::-1]
            margins.append(top[0] - top[1])
        k = kernel(x, x[i:i + 1], ell, s2, p)[:, 0]
        c = (k - cols[:j].T @ cols[:j, i]) / np.sqrt(d[i])
        cols[j] = c
        d = np.maximum(d - c * c, 0.0)
        d[i] = 0.0
        piv.append(i)
    return np.array(piv), np.array(margins)


GREEDY_M, GREEDY_MARGIN = 8, 1e-9  # the margin every pick must clear: a million times the float64 round-off of the device's sums


def greedy_inputs(D, p):
    """1500 points (more than one 1024-point tile of the step kernel) inside less than half a period, where k falls monotonically with
    the distance: over whole periods the second pick sits at delta = p / 2, the flat minimum of k, and the runner-up is within
    1e-12 s2 of it for every seed tried (a near tie of the reference itself, not a question for the device)."""
    x = np.random.default_rng(5).uniform(0.0, 0.45 * p, size=(1500, D))
    return x, 0.3 * np.array([1.0, 1.2, 1.5][:D])
