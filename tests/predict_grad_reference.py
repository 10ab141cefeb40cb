"""Float64 numpy reference of the posterior of the gradient of f at new inputs (include/agpl_grad.h), for
tests/test_predict_grad_reference_cpu.py and tests/test_gpu_predict_grad.py, built on tests/kernels_reference.py.  No GPU, no
library code: nothing here imports the package.

With K_ZZ + jitter I = L L', q(v) = N(m, S), S = U' U, m = U' v, u_ad = (x_d - z_ad) / ell_d, r^2 = sum_d u_ad^2:
    d k(x, z_a) / d x_d = s2 (kappa'(r) / r) u_ad / ell_d
    psi_d(x)            = (ell_d / sqrt c) L^-1 d k_Z(x) / d x_d,        c = -lim_{r -> 0} kappa'(r) / r
    E   d f / d x_d     = (sqrt c / ell_d) psi_d' m
    Var d f / d x_d     = (c / ell_d^2) (s2 - |psi_d|^2 + |U psi_d|^2)
tests/test_predict_grad_reference_cpu.py proves these against difference quotients of the float64 posterior of f itself."""
import numpy as np

import kernels_reference as K

KINDS = (K.SE, K.MATERN32, K.MATERN52, K.RQ)  # Matern-1/2 is not mean-square differentiable


def drule(kind, r2, param=0.0):
    """kappa'(r) / r as a function of r^2 (csrc/agpl_kernel_rules.h: kernel_drule, restated), with its limit at r = 0."""
    r2 = np.asarray(r2, np.float64)
    r = np.sqrt(r2)
    if kind == K.SE:
        return -np.exp(-0.5 * r2)
    if kind == K.MATERN32:
        return -3.0 * np.exp(-np.sqrt(3.0) * r)
    if kind == K.MATERN52:
        return -(5.0 / 3.0) * (1.0 + np.sqrt(5.0) * r) * np.exp(-np.sqrt(5.0) * r)
    if kind == K.RQ:
        return -((1.0 + r2 / (2.0 * param)) ** (-param - 1.0))
    raise ValueError(kind)


def c_of(kind, param=0.0):
    """c = -lim kappa'(r) / r at r = 0: the prior variance of d f / d x_d is c s2 / ell_d^2."""
    return float(-drule(kind, 0.0, param))


def whitening(kind, z, ell, s2, jitter, param=0.0):
    """L^-1 of K_ZZ + jitter I = L L' (kernels_reference.phi_f64's)."""
    Lc = np.linalg.cholesky(K.kernel(kind, z, z, ell, s2, param) + jitter * np.eye(len(z)))
    return np.linalg.solve(Lc, np.eye(len(z)))


def dk(kind, x_s, z, ell, s2, d, param=0.0):
    """d k(x_i, z_a) / d x_d: [M, Ns]."""
    ell = np.asarray(ell, np.float64)
    u = (np.asarray(z, np.float64)[:, None, :] - np.asarray(x_s, np.float64)[None, :, :]) / ell  # (z - x) / ell: [M, Ns, D]
    return s2 * drule(kind, (u * u).sum(-1), param) * (-u[:, :, d]) / ell[d]


def psi(kind, x_s, z, ell, s2, jitter, d, param=0.0, Linv=None):
    """The normalised derivative feature psi_d: [M, Ns]."""
    Linv = whitening(kind, z, ell, s2, jitter, param) if Linv is None else Linv
    return (ell[d] / np.sqrt(c_of(kind, param))) * (Linv @ dk(kind, x_s, z, ell, s2, d, param))


def grad_moments(x_s, z, ell, s2, jitter, kind, param, U, v, dims=None):
    """(dmu, dvar), float64 [L, len(dims), Ns] (dims: every input dimension by default); U [L, M, M] lower triangular with
    S = U' U, v [L, M] with m = U' v (the plan's own state read back)."""
    x_s, ell = np.asarray(x_s, np.float64), np.asarray(ell, np.float64)
    U, v = np.asarray(U, np.float64), np.asarray(v, np.float64)
    if U.ndim == 2:
        U, v = U[None], v[None]
    dims = range(x_s.shape[1]) if dims is None else dims
    c = c_of(kind, param)
    Linv = whitening(kind, z, ell, s2, jitter, param)
    dmu = np.empty((len(U), len(dims), len(x_s)))
    dvar = np.empty_like(dmu)
    for j, d in enumerate(dims):
        P = psi(kind, x_s, z, ell, s2, jitter, d, param, Linv)
        for l in range(len(U)):
            T = U[l] @ P
            dmu[l, j] = (np.sqrt(c) / ell[d]) * ((U[l].T @ v[l]) @ P)
            dvar[l, j] = (c / ell[d] ** 2) * (s2 - (P * P).sum(0) + (T * T).sum(0))
    return dmu, dvar
