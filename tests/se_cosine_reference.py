"""Float64 numpy reference of the squared exponential x cosine kernel (include/agpl_kernels.h: AGPL_KERNEL_SE_COSINE = 10,
param = the period p),

    k(x, x') = s2 exp(-1/2 sum_d ((x_d - x'_d) / ell_d)^2) cos(2 pi (x_{D-1} - x'_{D-1}) / p),

for tests/test_se_cosine_reference_cpu.py and tests/test_gpu_se_cosine.py: k, K_ZZ, the whitened features, the derivatives for
log ell, z and x (a product rule in the last dimension), the derivative feature's normalisation, the bound's gradients with an
autograd cross-check, the spectral draw and greedy pivots.  No GPU, no library code: nothing here imports the package."""
import numpy as np

KIND = 10
JITTER = 1e-8
# ell_{D-1} / p.  0.3: the period is longer than the envelope, which dies within a cycle (k goes negative once, at a fraction of its
# height); 1.5: several oscillations inside the envelope, about 1.5 per lengthscale (k reaches -0.95 s2 half a period away).
RATIOS = (0.3, 1.5)
# the stretch of the last coordinate, in periods, that x and z cover in each regime: what keeps cond(K_ZZ + jitter I) of every case
# under the worst of tests/kernels_reference.py's own (tests/test_se_cosine_reference_cpu.py asserts it; the spectral density of
# this kernel is two Gaussians at +-2 pi / p and next to nothing at 0, so inducing inputs much closer than ell_{D-1} in the last
# coordinate make K_ZZ singular faster than they do for the squared exponential)
SPAN = {0.3: 5.0, 1.5: 12.0}
NS = (1, 255, 777)
ELL = 0.3
# (D, M); D = 1: the peeled loop with zero iterations, D = 2: with one; M = 200: the padding to 256
CASES = [(1, 16), (2, 16), (3, 64), (4, 200)]


def cospi(t):
    """cos(pi t) with the argument reduced exactly first, so that t = +-1/2 gives exactly 0 and t = 1 exactly -1 (the device's cospi)."""
    r = np.remainder(np.abs(np.asarray(t, np.float64)), 2.0)  # exact, in [0, 2); of |t|: even to the bit
    c = np.cos(np.pi * r)
    return np.where((r == 0.5) | (r == 1.5), 0.0, c)


def sinpi(t):
    t = np.asarray(t, np.float64)
    r = np.remainder(np.abs(t), 2.0)
    return np.sign(t) * np.where((r == 0.0) | (r == 1.0), 0.0, np.sin(np.pi * r))


def parts(a, b, ell, p):
    """u [n, m, D] = (a_d - b_d) / ell_d, E [n, m] = exp(-|u|^2 / 2), c, s [n, m] = cos, sin(2 pi (a_L - b_L) / p), L = D - 1."""
    d = np.asarray(a, np.float64)[:, None, :] - np.asarray(b, np.float64)[None, :, :]
    u = d / np.asarray(ell, np.float64)
    return u, np.exp(-0.5 * (u * u).sum(-1)), cospi(2.0 * d[..., -1] / p), sinpi(2.0 * d[..., -1] / p)


def period_of(ell, ratio):
    return float(np.asarray(ell, np.float64)[-1] / ratio)


def kernel(a, b, ell, s2, p):
    _, E, c, _ = parts(a, b, ell, p)
    return s2 * E * c


def dkernel_dlogell(a, b, ell, s2, p):
    """[D, n, m]: d k / d log ell_d = u_d^2 k in every dimension, the last included (the cosine does not depend on ell)."""
    u, E, c, _ = parts(a, b, ell, p)
    return np.moveaxis((s2 * E * c)[..., None] * u * u, -1, 0)


def dkernel_da(a, b, ell, s2, p):
    """[D, n, m]: d k(a, b) / d a_d = -(u_d / ell_d) k for d < L and s2 E (-(u_L / ell_L) c - (2 pi / p) s) for the last (d / d b_d is
    its negative)."""
    u, E, c, s = parts(a, b, ell, p)
    ell = np.asarray(ell, np.float64)
    out = -(s2 * E * c)[..., None] * u / ell
    out[..., -1] -= s2 * E * (2.0 * np.pi / p) * s
    return np.moveaxis(out, -1, 0)


def prior_grad_variance(ell, s2, p):
    """[D]: the prior variance of d f / d x_d, -d^2 k / d tau_d^2 at 0: s2 / ell_d^2, the last s2 (1 / ell_L^2 + (2 pi / p)^2)."""
    v = s2 / np.asarray(ell, np.float64) ** 2
    v[-1] += s2 * (2.0 * np.pi / p) ** 2
    return v


def grad_normalisation(ell, p):
    """[D]: c_d of the normalised derivative feature psi_d = (ell_d / sqrt c_d) L^-1 d k_Z / d x_d: 1, the last 1 + (2 pi ell_L / p)^2."""
    ell = np.asarray(ell, np.float64)
    c = np.ones(len(ell))
    c[-1] += (2.0 * np.pi * ell[-1] / p) ** 2
    return c


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


def workload(N, M, D, ratio, seed=5, ell=ELL):
    """-> x, z, ells, p.  Lengthscales ell (1, 1.2, 1.5, 0.8)[:D], p = ell_{D-1} / ratio.  The leading coordinates of x and z uniform
    in [0, 1]; the last of both over SPAN[ratio] periods, [0, SPAN p] (z on a jittered grid in D = 1, uniform draws else).  z is
    drawn first: it does not depend on N, so a condition on z holds for every N.  Two pairs are placed: z[2] is z[1] moved by
    -p / 4 in the last coordinate and x[0] is z[1] moved by -p / 2, so k(x[0], z[1]) = -s2 (the other differences are 0) and
    k(x[0], z[2]) = 0 (a quarter period)."""
    ells = lengthscales(D, ell)
    p = period_of(ells, ratio)
    span = SPAN[ratio] * p
    rng = np.random.default_rng(seed + 7 * M + D)
    z = rng.uniform(0.0, 1.0, size=(M, D))
    if D == 1:
        z[:, 0] = (np.arange(M) + 0.5 + 0.2 * rng.uniform(-1, 1, M)) * (span / M)
    else:
        z[:, -1] *= span
    z[1, -1] = 0.5 * span  # (the three placed inputs stay inside the stretch)
    z[2] = z[1]
    z[2, -1] = z[1, -1] - 0.25 * p
    x = rng.uniform(0.0, 1.0, size=(N, D))
    x[:, -1] *= span
    x[0] = z[1]
    x[0, -1] = z[1, -1] - 0.5 * p
    return x, z, ells, p


# (D, M, ratio) of the cases whose posterior is compared (predict, predict_cov, predict_grad, the gradients): both regimes at every other case
FIT = [(1, 16, 0.3), (2, 16, 1.5), (3, 64, 0.3), (4, 200, 1.5)]


def predict_inputs(z, ells, p, ratio, n=255):
    """The new inputs of the posterior comparisons: leading coordinates in [0, 1], the last over the inducing inputs' stretch and two
    lengthscales beyond it on either side (there the residual is nearly s2: max var >= 0.025 s2 whatever q(v) is); the first two sit
    half and a quarter period from z[1], the other differences 0."""
    D = z.shape[1]
    xs = np.random.default_rng(23).uniform(0.0, 1.0, size=(n, D))
    lo, hi = -2.0 * ells[-1], SPAN[ratio] * p + 2.0 * ells[-1]
    xs[:, -1] = lo + (hi - lo) * xs[:, -1]
    xs[0] = z[1]
    xs[0, -1] += 0.5 * p
    xs[1] = z[1]
    xs[1, -1] += 0.25 * p
    return xs


def max_var_lower_bound(xs, z, ell, s2, p):
    """max over xs of the residual s2 - |phi(x)|^2: a lower bound of max var for ANY q(v), since var = residual + |U phi|^2."""
    return phi_f64(xs, z, ell, s2, p)[1].max()


def spectral_draw(rng, F, D, ell, p):
    """omega [F, D] in the scaled units u = x / ell: N(0, 1) in every column, the last moved by +-2 pi ell_L / p with a fair sign, so
    that E cos(omega . du) = exp(-|du|^2 / 2) cos(2 pi ell_L du_L / p)."""
    om = rng.standard_normal((F, D))
    om[:, -1] += np.where(rng.uniform(size=F) < 0.5, -1.0, 1.0) * (2.0 * np.pi * np.asarray(ell, np.float64)[-1] / p)
    return om


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
        u = d / th[:D].exp()
        return th[D].exp() * torch.exp(-0.5 * (u * u).sum(-1)) * torch.cos(2.0 * np.pi * d[..., -1] / p)

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
# (D, ell / p, periods the last coordinate covers): stretches on which every pick beats the runner-up by a clear margin
# (tests/test_se_cosine_reference_cpu.py asserts it from this file alone) and the picks meet k below zero
GREEDY_CASES = [(1, 0.3, 1.0), (2, 1.5, 2.0), (3, 0.3, 0.45)]


def greedy_inputs(D, ratio, periods):
    """-> x, ells, p: 1500 points (more than one 1024-point tile of the step kernel), the leading coordinates in [0, 1], the last over
    ``periods`` periods."""
    ells = lengthscales(D)
    p = period_of(ells, ratio)
    rng = np.random.default_rng(5)
    x = rng.uniform(0.0, 1.0, size=(1500, D))
    x[:, -1] = rng.uniform(0.0, periods * p, size=1500)
    return x, ells, p
