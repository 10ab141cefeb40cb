"""tests/predict_grad_reference.py proved independently of its closed form (CPU only): the mean and the variance of d f / d x_d are
compared with central difference quotients of the float64 posterior of f itself,
    q_h = (f(x + h e_d) - f(x - h e_d)) / (2 h),     E q_h = (mu(x+) - mu(x-)) / (2 h),
    Var q_h = (C(x+, x+) - 2 C(x+, x-) + C(x-, x-)) / (4 h^2),     C(a, b) = k(a, b) + phi(a)' (S - I) phi(b)
(the posterior covariance as tests/joint_reference.py states it), at two steps h and h / 2.

Steps.  h is in units of ell_d.  The truncation error of q_h is O(h^2) where kappa is smooth: the discrepancy falls 4x from h to h / 2.
Matern-3/2 has kappa = 1 - 3 r^2 / 2 + sqrt(3) |r|^3 - ...: Var q_h carries k(x+, x-) at distance 2 h, so (2 - 2 kappa(2 h)) / (4 h^2) =
3 - 4 sqrt(3) h: a relative error 2.31 h, first order (2x), which needs h / 2 <= 4e-4 for the 1e-3 bar; its mean is smooth away from the
inducing inputs.  Rounding: 1e-16 / (4 h^2) relative, 2e-10 at the smallest step -- far below every discrepancy measured here."""
import numpy as np
import pytest

import kernels_reference as K
import predict_grad_reference as G

M, NS, S2, JITTER = 12, 40, 2.5, 1e-6
H = {K.SE: 0.02, K.MATERN52: 0.02, K.RQ: 0.02, K.MATERN32: 8e-4}
IDS = [K.NAMES[k] for k in G.KINDS]


def problem(kind, D, seed=5):
    rng = np.random.default_rng(seed + 10 * D)
    z = rng.uniform(-3, 3, size=(M, D))
    xs = rng.uniform(-3.5, 3.5, size=(NS, D))  # some outside the hull of z
    ell = np.array([1.0, 1.4, 1.8][:D])
    U = np.tril(0.3 * rng.standard_normal((M, M)))
    U[np.diag_indices(M)] = rng.uniform(0.3, 1.0, M)  # S = U' U: a random SPD q(v)
    v = rng.standard_normal(M)
    return xs, z, ell, U, v


def posterior(kind, param, z, ell, U, v):
    """mu(a) and C(a, b) of f in float64."""
    Linv = G.whitening(kind, z, ell, S2, JITTER, param)
    phi = lambda a: Linv @ K.kernel(kind, z, a, ell, S2, param)  # [M, n]
    W = U.T @ U - np.eye(M)
    mu = lambda a: (U.T @ v) @ phi(a)
    # the diagonal of C(a, b) for paired points
    cov = lambda a, b: S2 * K.kappa(kind, (((a - b) / ell) ** 2).sum(1), param) + np.einsum("ai,ab,bi->i", phi(a), W, phi(b))
    return mu, cov


@pytest.mark.parametrize("D", [1, 3])
@pytest.mark.parametrize("kind", G.KINDS, ids=IDS)
def test_closed_form_is_the_limit_of_difference_quotients(kind, D):
    param = K.param_of(kind)
    xs, z, ell, U, v = problem(kind, D)
    dmu, dvar = G.grad_moments(xs, z, ell, S2, JITTER, kind, param, U, v)
    assert dmu.shape == dvar.shape == (1, D, NS)
    mu, cov = posterior(kind, param, z, ell, U, v)
    lo, hi = (1.7, 4.5) if kind == K.MATERN32 else (3.0, 5.0)
    for d in range(D):
        errs = []
        for h in (H[kind], H[kind] / 2):
            e = np.zeros(D)
            e[d] = h * ell[d]
            qm = (mu(xs + e) - mu(xs - e)) / (2 * e[d])
            qv = (cov(xs + e, xs + e) - 2 * cov(xs + e, xs - e) + cov(xs - e, xs - e)) / (4 * e[d] ** 2)
            errs.append((np.abs(qm - dmu[0, d]).max() / np.abs(dmu[0, d]).max(), np.abs(qv - dvar[0, d]).max() / np.abs(dvar[0, d]).max()))
        (m1, v1), (m2, v2) = errs
        print(f"{K.NAMES[kind]} D={D} d={d}: mean {m1:.3e} -> {m2:.3e} ({m1 / m2:.2f}x), var {v1:.3e} -> {v2:.3e} ({v1 / v2:.2f}x)")
        assert m2 < 1e-3 and v2 < 1e-3, (m2, v2)
        assert 3.0 <= m1 / m2 <= 5.0, m1 / m2  # (the mean is smooth away from the inducing inputs for every kind)
        assert lo <= v1 / v2 <= hi, v1 / v2
    assert (dvar > 0).all() and np.abs(dmu).max() > 1e-2


@pytest.mark.parametrize("D", [1, 3])
@pytest.mark.parametrize("kind", G.KINDS, ids=IDS)
def test_normalised_feature_is_bounded_by_sigma(kind, D):
    """|psi_d|^2 <= s2: the bound the plan's image scale relies on -- at random points, at the inducing inputs themselves and far away."""
    param = K.param_of(kind)
    xs, z, ell, _, _ = problem(kind, D)
    pts = np.concatenate([xs, z, z + 1e-3, 1e3 * ell * np.ones((1, D))])
    for d in range(D):
        P = G.psi(kind, pts, z, ell, S2, JITTER, d, param)
        assert np.isfinite(P).all()
        assert (P * P).sum(0).max() <= S2 * (1 + 1e-12), (d, (P * P).sum(0).max())
        assert (P * P).sum(0).max() > 0.1 * S2  # (not vacuous: near z the inducing set explains most of the derivative)


@pytest.mark.parametrize("kind", G.KINDS, ids=IDS)
def test_c_is_the_limit_of_the_rule_and_the_rule_is_the_derivative_of_kappa(kind):
    param = K.param_of(kind)
    assert G.c_of(kind, param) == -G.drule(kind, 0.0, param)
    assert G.c_of(kind, param) == {K.SE: 1.0, K.MATERN32: 3.0, K.MATERN52: 5.0 / 3.0, K.RQ: 1.0}[kind]
    # kappa'(r) / r against a central difference of kernels_reference.kappa, and its limit against kappa's curvature at 0
    r, dl = np.array([0.05, 0.3, 1.0, 2.7, 6.0]), 1e-5
    num = (K.kappa(kind, (r + dl) ** 2, param) - K.kappa(kind, (r - dl) ** 2, param)) / (2 * dl * r)
    assert np.abs(num - G.drule(kind, r * r, param)).max() < 1e-8
    assert abs((K.kappa(kind, 1e-8, param) - 1.0) / 0.5e-8 + G.c_of(kind, param)) < 1e-3  # kappa = 1 - c r^2 / 2 + ...
    # the prior variance of d f / d x_d: a fresh q(v) = N(0, I) gives c s2 / ell_d^2 and a zero mean
    xs, z, ell, _, _ = problem(kind, 3)
    dmu, dvar = G.grad_moments(xs, z, ell, S2, JITTER, kind, param, np.eye(M), np.zeros(M))
    assert (dmu == 0).all() and np.abs(dvar[0] * (ell ** 2)[:, None] / (G.c_of(kind, param) * S2) - 1).max() < 1e-12


def test_the_device_rule_states_the_same_limits():
    """csrc/agpl_kernel_rules.h documents kappa'(r) / r with these constants (the reference restates, the header is the source)."""
    import os

    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "augmentedgplikelihoods.jl_amd", "csrc",
                            "agpl_kernel_rules.h")).read()
    body = src[src.index("kernel_drule(double r2"):src.index("kernel_dvalue")]
    assert "(T)-3 * kernel_exp" in body and "(T)(-5.0 / 3.0)" in body and "return -kernel_exp((T)-0.5 * (T)r2);" in body
