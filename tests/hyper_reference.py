"""Float64 CPU reference of the bound whose gradient agpl_plan_hyper_grad computes (include/agpl_hyper.h), in torch from raw
inputs, for the five kinds of include/agpl_kernels.h; the gradient comes from autograd.  No GPU, no library code.

    Lb(theta) = sum_l sum_i [ beta_li mu_li - gamma_li (mu_li^2 + var_li) / 2 ],   theta = (log ell_1 .. log ell_D, log variance)
    mu_li = mu0_li + phi_i' m_l,  var_li = variance - |phi_i|^2 + phi_i' S_l phi_i,  phi_i = L^-1 k_Z(x_i),  K_ZZ + jitter I = L L'

``gradient`` returns the gradient, its two halves -- the POINTS' part (through k_Z(x_i) and the variance, L held fixed) and the
K_ZZ part (through L) -- and, per component of theta, the SCALE sum |terms|: the absolute values of the per-(a, i) contributions
dLb/dk_ai dk_ai/dtheta, of the per-point variance terms gamma_li variance / 2, and of the per-(a, b) contributions
dLb/dK_ab dK_ab/dtheta.  The gradient is a cancelling sum of these; errors are quoted relative to the scale."""
import numpy as np
import torch

import kernels_reference as KR

F64 = torch.float64
# The bars of tests/test_gpu_hyper_grad.py on |device - reference| / scale, one per quantity: each is 4 x the worst value measured on
# an MI355X over that file's six cases and three seeds (the margin covers another draw of the data).
HYPER_BAR_FULL = 4 * 1.988e-07    # the whole gradient over the whole scale; worst: matern52, N = 65836, M = 40, D = 1, L = 2
HYPER_BAR_POINTS = 4 * 8.973e-08  # the G = NULL call (the points' part; the hot kernel); worst: the same case
# the difference of the two calls over the K_ZZ scale alone; worst: se, N = 65836, M = 40, D = 3, mu0 (1.3e-6 and 3.9e-7 at its
# other seeds, <= 6.8e-7 in the other cases)
HYPER_BAR_KZZ = 4 * 3.595e-06
HYPER_BAR = max(HYPER_BAR_FULL, HYPER_BAR_POINTS, HYPER_BAR_KZZ)  # what a broken gradient must miss a hundredfold
_TINY = 1e-300  # r = sqrt(max(r^2, tiny)): keeps autograd finite at r = 0, where every d r^2 / d theta is 0


def kappa(kind, r2, param=0.0):
    """kernels_reference.kappa in torch."""
    r = r2.clamp_min(_TINY).sqrt()
    if kind == KR.SE:
        return torch.exp(-0.5 * r2)
    if kind == KR.MATERN12:
        return torch.exp(-r)
    if kind == KR.MATERN32:
        return (1.0 + np.sqrt(3.0) * r) * torch.exp(-np.sqrt(3.0) * r)
    if kind == KR.MATERN52:
        return (1.0 + np.sqrt(5.0) * r + 5.0 * r2 / 3.0) * torch.exp(-np.sqrt(5.0) * r)
    if kind == KR.RQ:
        return (1.0 + r2 / (2.0 * param)) ** (-param)
    raise ValueError(kind)


def dkappa_over_r(kind, r2, param=0.0):
    """kappa'(r) / r in closed form (0 at r = 0 for Matern-1/2, which has no limit there)."""
    r = r2.clamp_min(_TINY).sqrt()
    if kind == KR.SE:
        return -torch.exp(-0.5 * r2)
    if kind == KR.MATERN12:
        return torch.where(r2 > 0, -torch.exp(-r) / r, torch.zeros_like(r))
    if kind == KR.MATERN32:
        return -3.0 * torch.exp(-np.sqrt(3.0) * r)
    if kind == KR.MATERN52:
        return -(5.0 / 3.0) * (1.0 + np.sqrt(5.0) * r) * torch.exp(-np.sqrt(5.0) * r)
    if kind == KR.RQ:
        return -((1.0 + r2 / (2.0 * param)) ** (-param - 1.0))
    raise ValueError(kind)


def _t(a):
    return None if a is None else torch.as_tensor(np.asarray(a), dtype=F64)


def _u2(a, b, ell):
    """((a_d - b_d) / ell_d)^2, [len(a), len(b), D]."""
    u = (a[:, None, :] - b[None, :, :]) / ell
    return u * u


def _bound(kzx, Kzz, s2, m, S, beta, gamma, mu0):
    Lc = torch.linalg.cholesky(Kzz)
    phi = torch.linalg.solve_triangular(Lc, kzx, upper=False)  # [M, N]
    total = 0.0
    for l in range(m.shape[0]):
        mu = m[l] @ phi + (mu0[l] if mu0 is not None else 0.0)
        var = s2 - (phi * phi).sum(0) + (phi * (S[l] @ phi)).sum(0)
        total = total + (beta[l] * mu - 0.5 * gamma[l] * (mu * mu + var)).sum()
    return total


def bound(kind, param, x, z, theta, jitter, m, S, beta, gamma, mu0=None):
    """Lb(theta); theta a float64 tensor [D + 1] (autograd flows through it)."""
    x, z, m, S, beta, gamma, mu0 = (_t(a) for a in (x, z, m, S, beta, gamma, mu0))
    D = x.shape[1]
    ell, s2 = theta[:D].exp(), theta[D].exp()
    kzx = s2 * kappa(kind, _u2(z, x, ell).sum(-1), param)
    Kzz = s2 * kappa(kind, _u2(z, z, ell).sum(-1), param) + jitter * torch.eye(z.shape[0], dtype=F64)
    return _bound(kzx, Kzz, s2, m, S, beta, gamma, mu0)


def gradient(kind, param, x, z, ell, s2, jitter, m, S, beta, gamma, mu0=None, broken=None):
    """dict(value, grad, points, kzz, scale, scale_points, scale_kzz), numpy float64 [D + 1] each (value a float).
    x [N, D], z [M, D], ell [D]; m [L, M], S [L, M, M]; beta, gamma, mu0 [L, N].
    ``broken``: None, or a deliberately wrong gradient: "S=I" (S replaced by the identity), "no_kzz" (the K_ZZ part dropped),
    "swap_ell" (the first two lengthscales swapped -- for D = 1 the lengthscale doubled)."""
    x, z, m, S, beta, gamma, mu0 = (_t(a) for a in (x, z, m, S, beta, gamma, mu0))
    ell = torch.as_tensor(np.asarray(ell, np.float64).reshape(-1))
    D, M = x.shape[1], z.shape[0]
    if broken == "S=I":
        S = torch.eye(M, dtype=F64).expand_as(S).clone()
    if broken == "swap_ell":
        ell = ell.clone()
        if D == 1:
            ell[0] = 2.0 * ell[0]
        else:
            ell[[0, 1]] = ell[[1, 0]]
    theta = torch.cat([ell.log(), torch.tensor([np.log(s2)], dtype=F64)]).requires_grad_(True)
    value = bound(kind, param, x, z, theta, jitter, m, S, beta, gamma, mu0)
    (full,) = torch.autograd.grad(value, theta)
    # the halves: dLb/dk_ZX and dLb/dK_ZZ by autograd on detached leaves, the kernel's elementwise derivative in closed form
    s2t = torch.tensor(float(s2), dtype=F64)
    u2x, u2z = _u2(z, x, ell), _u2(z, z, ell)
    r2x, r2z = u2x.sum(-1), u2z.sum(-1)
    kzx = (s2t * kappa(kind, r2x, param)).requires_grad_(True)
    Kzz0 = s2t * kappa(kind, r2z, param)
    Kzz = (Kzz0 + jitter * torch.eye(M, dtype=F64)).requires_grad_(True)
    Wk, Kbar = torch.autograd.grad(_bound(kzx, Kzz, s2t, m, S, beta, gamma, mu0), (kzx, Kzz))
    Kbar = 0.5 * (Kbar + Kbar.T)
    dx = -s2t * dkappa_over_r(kind, r2x, param)  # dk/dlog ell_d = dx u2_d
    dz = -s2t * dkappa_over_r(kind, r2z, param)
    dz = dz * (1.0 - torch.eye(M, dtype=F64))     # the diagonal (r = 0) carries no lengthscale term
    pts, kz, sp, sk = (torch.zeros(D + 1, dtype=F64) for _ in range(4))
    for d in range(D):
        tx, tz = Wk * dx * u2x[..., d], Kbar * dz * u2z[..., d]
        pts[d], sp[d], kz[d], sk[d] = tx.sum(), tx.abs().sum(), tz.sum(), tz.abs().sum()
    tx, tz, tv = Wk * kzx.detach(), Kbar * Kzz0, -0.5 * gamma * s2t
    pts[D], sp[D] = tx.sum() + tv.sum(), tx.abs().sum() + tv.abs().sum()
    kz[D], sk[D] = tz.sum(), tz.abs().sum()
    if broken == "no_kzz":
        full = pts.clone()
    n = lambda t: t.detach().numpy().copy()
    return {"value": float(value.detach()), "grad": n(full), "points": n(pts), "kzz": n(kz), "scale": n(sp + sk), "scale_points": n(sp),
            "scale_kzz": n(sk)}


def synthetic_q(M, L, N, seed, spread=1.0):
    """A plausible q(v) and per-point (beta, gamma, mu0) without a sweep: S = (I + G)^-1, m = S g for a random PSD G; gamma > 0."""
    rng = np.random.default_rng(seed)
    m, S = np.zeros((L, M)), np.zeros((L, M, M))
    for l in range(L):
        B = rng.normal(size=(M, 2 * M)) * spread
        S[l] = np.linalg.inv(np.eye(M) + B @ B.T / M)
        m[l] = S[l] @ rng.normal(size=M) * 3.0
    beta = rng.normal(size=(L, N))
    gamma = rng.uniform(0.05, 0.3, size=(L, N))
    mu0 = 0.5 * rng.normal(size=(L, N))
    return m, S, beta, gamma, mu0
