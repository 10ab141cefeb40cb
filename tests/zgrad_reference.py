"""Float64 CPU reference of the gradient agpl_plan_inducing_grad computes (include/agpl_zgrad.h): the bound of tests/hyper_reference.py
as a function of the inducing inputs z, in torch from raw inputs, for the five kinds; the gradient comes from autograd.  No GPU,
no library code.

``gradient_z`` returns the gradient [M, D], its two halves in closed form -- the POINTS' part (through k_Z(x_i), L held fixed)
    dLb/dz_ad = sum_l sum_i W_ai variance q(r_ai) (z_ad - x_id) / ell_d^2,   q(r) = kappa'(r) / r,  W = dLb / dk_ZX
and the K_ZZ part (through L)
    dLb/dz_ad += 2 sum_{b != a} Kbar_ab variance q(r_ab) (z_ad - z_bd) / ell_d^2,   Kbar = sym(dLb / dK_ZZ)
-- and, per component, the SCALE sum |terms| of each half.  The gradient is a cancelling sum of these; errors are quoted relative
to the scale."""
import numpy as np
import torch

import hyper_reference as HR

F64 = torch.float64
# The bars of tests/test_gpu_zgrad.py on |device - reference| / scale, worst over (a, d), one per quantity: each is 4 x the worst value
# measured on an MI355X over that file's six cases and three seeds (the margin covers another draw of the data).
ZGRAD_BAR_FULL = 4 * 6.900e-06    # the whole gradient over the whole scale; worst: rq, N = 1000, M = 300, D = 3, seed 5
ZGRAD_BAR_POINTS = 4 * 2.486e-06  # the G = NULL call (the points' part; the hot kernel); worst: se, N = 1000, M = 40, D = 1, seed 5
# the K_ZZ part: the difference of the two calls over the K_ZZ scale alone, with G, g formed in float64 from the reference's features at
# the plan's gamma, beta; worst: se, N = 65836, M = 40, D = 3, mu0, seed 4 (3.0e-8 and 2.8e-8 at its other seeds: the prior-mean term
# h comes from the split-float16 images; <= 7.2e-12 in the cases without mu0 at N = 65836, <= 4.5e-13 elsewhere).  With the SWEEP's
# G, g the same difference is up to 2.608e-5 of the K_ZZ scale (the same case, seed 5): their 2^-22 (split-float16 products)
# carried through L^-1 of a K_ZZ at jitter 1e-6 -- the inputs' precision, not the sequence's; the whole-gradient bar covers that path.
ZGRAD_BAR_KZZ = 4 * 4.602e-08
ZGRAD_BAR = max(ZGRAD_BAR_FULL, ZGRAD_BAR_POINTS)  # what a broken gradient must miss a hundredfold (the K_ZZ half: ZGRAD_BAR_KZZ)


def _du(a, b, ell):
    """(a_d - b_d) / ell_d, [len(a), len(b), D]."""
    return (a[:, None, :] - b[None, :, :]) / ell


def bound_z(kind, param, x, z, ell, s2, jitter, m, S, beta, gamma, mu0=None):
    """Lb as a function of z: a float64 tensor [M, D] (autograd flows through it); the rest numpy or tensors."""
    x, m, S, beta, gamma, mu0 = (HR._t(a) for a in (x, m, S, beta, gamma, mu0))
    ell = torch.as_tensor(np.asarray(ell, np.float64).reshape(-1))
    s2 = torch.tensor(float(s2), dtype=F64)
    ux, uz = _du(z, x, ell), _du(z, z, ell)
    kzx = s2 * HR.kappa(kind, (ux * ux).sum(-1), param)
    Kzz = s2 * HR.kappa(kind, (uz * uz).sum(-1), param) + jitter * torch.eye(z.shape[0], dtype=F64)
    return HR._bound(kzx, Kzz, s2, m, S, beta, gamma, mu0)


def gradient_z(kind, param, x, z, ell, s2, jitter, m, S, beta, gamma, mu0=None, broken=None):
    """dict(value, grad, points, kzz, scale, scale_points, scale_kzz), numpy float64 [M, D] each (value a float).
    x [N, D], z [M, D], ell [D]; m [L, M], S [L, M, M]; beta, gamma, mu0 [L, N].
    ``broken``: None, or a deliberately wrong gradient: "S=I" (S replaced by the identity), "no_kzz" (the K_ZZ part dropped),
    "sign" (x - z in place of z - x), "ell_once" (divided by ell_d once, not twice)."""
    x, m, S, beta, gamma, mu0 = (HR._t(a) for a in (x, m, S, beta, gamma, mu0))
    ell = torch.as_tensor(np.asarray(ell, np.float64).reshape(-1))
    M = np.asarray(z).shape[0]
    if broken == "S=I":
        S = torch.eye(M, dtype=F64).expand_as(S).clone()
    zt = HR._t(z).clone().requires_grad_(True)
    value = bound_z(kind, param, x, zt, ell, s2, jitter, m, S, beta, gamma, mu0)
    (full,) = torch.autograd.grad(value, zt)
    # the halves: dLb/dk_ZX and dLb/dK_ZZ by autograd on detached leaves, the kernel's elementwise derivative in closed form
    z0 = zt.detach()
    s2t = torch.tensor(float(s2), dtype=F64)
    ux, uz = _du(z0, x, ell), _du(z0, z0, ell)
    r2x, r2z = (ux * ux).sum(-1), (uz * uz).sum(-1)
    kzx = (s2t * HR.kappa(kind, r2x, param)).requires_grad_(True)
    Kzz = (s2t * HR.kappa(kind, r2z, param) + jitter * torch.eye(M, dtype=F64)).requires_grad_(True)
    Wk, Kbar = torch.autograd.grad(HR._bound(kzx, Kzz, s2t, m, S, beta, gamma, mu0), (kzx, Kzz))
    Kbar = 0.5 * (Kbar + Kbar.T)
    qx = s2t * HR.dkappa_over_r(kind, r2x, param)
    qz = s2t * HR.dkappa_over_r(kind, r2z, param) * (1.0 - torch.eye(M, dtype=F64))  # the diagonal of K_ZZ does not depend on z
    tx = (Wk * qx)[..., None] * ux / ell         # [M, N, D]: (z_ad - x_id) / ell_d^2 = u_d / ell_d
    tz = 2.0 * (Kbar * qz)[..., None] * uz / ell  # [M, M, D]
    pts, sp, kz, sk = tx.sum(1), tx.abs().sum(1), tz.sum(1), tz.abs().sum(1)
    if broken == "no_kzz":
        full = pts.clone()
    if broken == "sign":
        full = -full
    if broken == "ell_once":
        full = full * ell
    n = lambda t: t.detach().numpy().copy()
    return {"value": float(value.detach()), "grad": n(full), "points": n(pts), "kzz": n(kz), "scale": n(sp + sk), "scale_points": n(sp),
            "scale_kzz": n(sk)}


def points_part_chunked(kind, param, x, z, ell, s2, jitter, m, S, beta, gamma, mu0=None, broken=None, chunk=4096):
    """dict(points, scale_points) of ``gradient_z``, summed over chunks of ``chunk`` points: no [M, N, D] tensor is formed, so N may be
    large.  The bound is a sum over the points and, with z (so L), m and S fixed, W_ai = dLb/dk_ZX of a point depends on that point
    alone: a chunk's W is autograd's on the chunk's own bound, and the sum over chunks is ``gradient_z``'s up to the order of the
    float64 additions.  ``broken``: None, or those of ``gradient_z`` that reach the points' part ("S=I", "sign", "ell_once")."""
    if broken not in (None, "S=I", "sign", "ell_once"):
        raise ValueError(broken)
    x, m, S, beta, gamma, mu0 = (HR._t(a) for a in (x, m, S, beta, gamma, mu0))
    ell = torch.as_tensor(np.asarray(ell, np.float64).reshape(-1))
    z0 = HR._t(z)
    M = z0.shape[0]
    if broken == "S=I":
        S = torch.eye(M, dtype=F64).expand_as(S).clone()
    s2t = torch.tensor(float(s2), dtype=F64)
    uz = _du(z0, z0, ell)
    Kzz = s2t * HR.kappa(kind, (uz * uz).sum(-1), param) + jitter * torch.eye(M, dtype=F64)
    pts, sp = torch.zeros(M, z0.shape[1], dtype=F64), torch.zeros(M, z0.shape[1], dtype=F64)
    for i0 in range(0, x.shape[0], chunk):
        sl = slice(i0, min(i0 + chunk, x.shape[0]))
        ux = _du(z0, x[sl], ell)
        r2x = (ux * ux).sum(-1)
        kzx = (s2t * HR.kappa(kind, r2x, param)).requires_grad_(True)
        (Wk,) = torch.autograd.grad(HR._bound(kzx, Kzz, s2t, m, S, beta[:, sl], gamma[:, sl], None if mu0 is None else mu0[:, sl]), kzx)
        tx = (Wk * (s2t * HR.dkappa_over_r(kind, r2x, param)))[..., None] * ux / ell
        pts += tx.sum(1)
        sp += tx.abs().sum(1)
    if broken == "sign":
        pts = -pts
    if broken == "ell_once":
        pts = pts * ell
    return {"points": pts.numpy().copy(), "scale_points": sp.numpy().copy()}
