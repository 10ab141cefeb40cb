"""Float64 numpy reference of the squared exponential x periodic kernel (include/agpl_kernels.h: AGPL_KERNEL_SE_PERIODIC = 8,
param = the period p),

    k(x, x') = s2 exp(-1/2 r^2),   r^2 = sum_{d < D-1} ((x_d - x'_d) / ell_d)^2 + (sin(pi (x_{D-1} - x'_{D-1}) / p) / ell_{D-1})^2,

for tests/test_se_periodic_reference_cpu.py and tests/test_gpu_se_periodic.py: k, K_ZZ, the whitened features, the derivatives for
log ell, z and x, the bound's gradients with an autograd cross-check, and greedy pivots.  No GPU, no library code: nothing here
imports the package."""
import numpy as np

KIND = 8
JITTER = 1e-8
PERIODS = (1.0, 2.5)
NS = (1, 255, 777)
ELL = 0.3
# (D, M); D = 1: the peeled loop with zero iterations, D = 2: with one; M = 200: the padding to 256.  (3, 200) is not a case: 200
# inducing inputs in three dimensions at these lengthscales give cond(K_ZZ + jitter I) = 1.1e7, beyond the worst case of
# tests/kernels_reference.py (3.3e4: the condition tests/test_se_periodic_reference_cpu.py asserts); (4, 200), 7.4e3, keeps the padding.
CASES = [(1, 16), (2, 16), (3, 64), (4, 200)]


def warp(a, b, ell, p):
    """u [n, m, D] = the terms of r^2, (a_d - b_d) / ell_d for d < D - 1 and sin(pi (a_d - b_d) / p) / ell_d for the last, and
    du [n, m, D] = d u / d a_d."""
    d = np.asarray(a, np.float64)[:, None, :] - np.asarray(b, np.float64)[None, :, :]
    ell = np.asarray(ell, np.float64)
    u, du = d / ell, np.broadcast_to(1.0 / ell, d.shape).copy()
    u[..., -1] = np.sin(np.pi * d[..., -1] / p) / ell[-1]
    du[..., -1] = (np.pi / p) * np.cos(np.pi * d[..., -1] / p) / ell[-1]
    return u, du


def kernel(a, b, ell, s2, p):
    u, _ = warp(a, b, ell, p)
    return s2 * np.exp(-0.5 * (u * u).sum(-1))


def dkernel_dlogell(a, b, ell, s2, p):
    """[D, n, m]: d k / d log ell_d = k u_d^2 (every term of r^2 is proportional to 1 / ell_d, warped or not)."""
    u, _ = warp(a, b, ell, p)
    k = s2 * np.exp(-0.5 * (u * u).sum(-1))
    return np.moveaxis(k[..., None] * u * u, -1, 0)


def dkernel_da(a, b, ell, s2, p):
    """[D, n, m]: d k(a, b) / d a_d = -k u_d u'_d (d / d b_d is its negative)."""
    u, du = warp(a, b, ell, p)
    k = s2 * np.exp(-0.5 * (u * u).sum(-1))
    return np.moveaxis(-k[..., None] * u * du, -1, 0)


def prior_grad_variance(ell, s2, p):
    """[D]: the prior variance of d f / d x_d, d^2 k / dx_d dx'_d at x = x': s2 / ell_d^2, the last s2 (pi / (p ell_d))^2."""
    ell = np.asarray(ell, np.float64)
    v = s2 / ell ** 2
    v[-1] = s2 * (np.pi / (p * ell[-1])) ** 2
    return v


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


def lengthscales(D, ell=ELL):
    return ell * np.array([1.0, 1.2, 1.5, 0.8][:D])


def workload(N, M, D, p, seed=5, ell=ELL):
    """The leading coordinates of x and z uniform in [0, 1]; the last of x over five periods, [-2 p, 3 p]; the last of z distinct
    within ONE period (a jittered grid in D = 1, uniform draws else, as tests/periodic_reference.py does it); lengthscales
    ell (1, 1.2, 1.5, 0.8)[:D].  z is drawn first: it does not depend on N, so a condition on z holds for every N."""
    rng = np.random.default_rng(seed + 7 * M + D)
    z = rng.uniform(0.0, 1.0, size=(M, D))
    if D == 1:
        z[:, 0] = (np.arange(M) + 0.5 + 0.2 * rng.uniform(-1, 1, M)) * (p / M)
    else:
        z[:, -1] *= p
    x = rng.uniform(0.0, 1.0, size=(N, D))
    x[:, -1] = -2.0 * p + 5.0 * p * x[:, -1]
    return x, z, lengthscales(D, ell)


def locally_periodic(N, M, p, seed=5):
    """x = (t, t), z = (s, s): k = SE(t - s) Per(t - s), the locally periodic kernel, from the D = 2 kind.  t over [-p, 2 p] (the
    squared exponential factor, ell = 0.3, lets a point see only the inducing inputs near it), s on a jittered grid over the same
    stretch."""
    rng = np.random.default_rng(seed + 7 * M + 2)
    s = -1.0 * p + (np.arange(M) + 0.5 + 0.2 * rng.uniform(-1, 1, M)) * (3.0 * p / M)  # (first: z does not depend on N)
    t = rng.uniform(-1.0 * p, 2.0 * p, size=N)
    return np.stack([t, t], 1), np.stack([s, s], 1), lengthscales(2) * np.array([p, 1.0])


# (D, M, p) of the cases whose posterior variance is compared (predict, predict_cov, predict_grad after ten sweeps)
FIT = [(1, 16, 2.5), (2, 16, 1.0), (3, 64, 1.0), (4, 200, 2.5)]


def predict_inputs(z, p, n=255):
    """The new inputs of the variance comparisons: leading coordinates in [0, 1], the last over four periods, [-1.5 p, 2.5 p]; the
    first sits at delta_last = p / 2 exactly from z[0] with the other differences 0 (u at its maximum, u' = 0)."""
    D = z.shape[1]
    xs = np.random.default_rng(23).uniform(0.0, 1.0, size=(n, D))
    xs[:, -1] = -1.5 * p + 4.0 * p * xs[:, -1]
    xs[0] = z[0]
    xs[0, -1] += p / 2
    return xs


def locally_periodic_predict_inputs(p, n=255):
    ts = np.random.default_rng(23).uniform(-1.0 * p, 2.0 * p, size=n)
    return np.stack([ts, ts], 1)


def max_var_lower_bound(xs, z, ell, s2, p):
    """max over xs of the residual s2 - |phi(x)|^2: a lower bound of max var for ANY q(v), since var = residual + |U phi|^2."""
    return phi_f64(xs, z, ell, s2, p)[1].max()


def bound_gradients(x, z, ell, s2, p, jitter, m, S, beta, gamma):
    """The sweep's bound Lb (tests/hyper_reference.py: _bound) for this kernel and its analytic gradients: ``theta`` [D + 1] for
    (log ell, log s2) and ``z`` [M, D], each with its scale, the sum of the absolute values of the terms it adds up (the yardstick
    of tests/test_gpu_hyper_grad.py and tests/test_gpu_zgrad.py), and ``auto_theta`` / ``auto_z``: the same two by autograd through
    the whole bound.  dLb / dk_ZX and dLb / dK_ZZ come from autograd on detached leaves, as in hyper_reference.gradient; the
    kernel's derivatives are the closed forms above."""
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
        d = a[:, None, :] - b[None, :, :]
        u = torch.cat([d[..., :-1], torch.sin(np.pi * d[..., -1:] / p)], -1) / th[:D].exp()
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


GREEDY_M = 8


def greedy_inputs(D, p):
    """1500 points (more than one 1024-point tile of the step kernel): the leading coordinates in [0, 1], the last inside less than
    half a period, where k falls monotonically with the distance (tests/periodic_reference.py: greedy_inputs says why)."""
    rng = np.random.default_rng(5)
    x = rng.uniform(0.0, 1.0, size=(1500, D))
    x[:, -1] = rng.uniform(0.0, 0.45 * p, size=1500)
    return x, lengthscales(D)
