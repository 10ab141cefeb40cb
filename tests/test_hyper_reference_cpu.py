"""tests/hyper_reference.py pinned on the CPU: its kappa is kernels_reference's, its autograd gradient agrees with central
differences of its own bound, its two halves add up to the whole, and the closed forms of include/agpl_hyper.h (the points' part
through C_l = L^-T (I - S_l - m_l m_l'), the K_ZZ part through the reverse rule of the Cholesky factorisation) reproduce both halves
in numpy."""
import numpy as np
import pytest
import torch

import hyper_reference as HR
import kernels_reference as KR


def _case(kind, D, L, seed=0, N=150, M=12):
    rng = np.random.default_rng(100 * kind + 10 * D + L + seed)
    x = rng.uniform(-3, 3, size=(N, D))
    z = rng.uniform(-3, 3, size=(M, D))
    ell = np.array([1.1, 1.7, 0.8][:D])
    m, S, beta, gamma, mu0 = HR.synthetic_q(M, L, N, seed + 7)
    return dict(kind=kind, param=KR.param_of(kind), x=x, z=z, ell=ell, s2=1.3, jitter=1e-6, m=m, S=S, beta=beta, gamma=gamma, mu0=mu0)


def test_kappa_is_the_kernels_reference():
    r2 = np.concatenate([[0.0], np.geomspace(1e-8, 50.0, 40)])
    for kind in KR.KINDS:
        got = HR.kappa(kind, torch.as_tensor(r2), KR.param_of(kind)).numpy()
        np.testing.assert_allclose(got, KR.kappa(kind, r2, KR.param_of(kind)), rtol=1e-14, atol=0)


@pytest.mark.parametrize("L", [1, 2])
@pytest.mark.parametrize("D", [1, 3])
@pytest.mark.parametrize("kind", KR.KINDS)
def test_autograd_against_central_differences(kind, D, L):
    c = _case(kind, D, L)
    ref = HR.gradient(**c)
    theta = np.concatenate([np.log(c["ell"]), [np.log(c["s2"])]])
    h = 1e-5
    f = lambda th: float(HR.bound(kind, c["param"], c["x"], c["z"], torch.as_tensor(th), c["jitter"], c["m"], c["S"], c["beta"],
                                  c["gamma"], c["mu0"]))
    for j in range(D + 1):
        e = np.zeros(D + 1)
        e[j] = h
        fd = (f(theta + e) - f(theta - e)) / (2 * h)
        assert abs(fd - ref["grad"][j]) <= 1e-6 * ref["scale"][j], (j, fd, ref["grad"][j], ref["scale"][j])
    # the halves (closed-form elementwise derivative of the kernel) add up to autograd's whole
    assert np.all(np.abs(ref["points"] + ref["kzz"] - ref["grad"]) <= 1e-10 * ref["scale"])


def header_formulas(kind, param, x, z, ell, s2, jitter, m, S, beta, gamma, mu0=None):
    """The two parts as include/agpl_hyper.h states them, in numpy float64: (points, kzz), [D + 1] each."""
    D, M = x.shape[1], z.shape[0]
    t = lambda a: torch.as_tensor(a)
    u2x = ((z[:, None, :] - x[None, :, :]) / ell) ** 2
    u2z = ((z[:, None, :] - z[None, :, :]) / ell) ** 2
    kx = s2 * HR.kappa(kind, t(u2x.sum(-1)), param).numpy()
    qx = -s2 * HR.dkappa_over_r(kind, t(u2x.sum(-1)), param).numpy()
    K0 = s2 * HR.kappa(kind, t(u2z.sum(-1)), param).numpy()
    qz = -s2 * HR.dkappa_over_r(kind, t(u2z.sum(-1)), param).numpy() * (1 - np.eye(M))
    Lc = np.linalg.cholesky(K0 + jitter * np.eye(M))
    Li = np.linalg.inv(Lc)
    phi = Li @ kx
    pts, A = np.zeros(D + 1), np.zeros((M, M))
    for l in range(m.shape[0]):
        b = beta[l] - gamma[l] * (mu0[l] if mu0 is not None else 0.0)
        C = Li.T @ (np.eye(M) - S[l] - np.outer(m[l], m[l]))
        p = Li.T @ m[l]
        Wk = gamma[l] * (C @ phi) + np.outer(p, b)
        for d in range(D):
            pts[d] += (Wk * qx * u2x[..., d]).sum()
        pts[D] += (Wk * kx).sum() - 0.5 * s2 * gamma[l].sum()
        G, gt = (phi * gamma[l]) @ phi.T, phi @ b
        A += (np.eye(M) - S[l]) @ G + np.outer(m[l], gt - G @ m[l])
    Lbar = -np.tril(Li.T @ A)
    P = np.tril(Lc.T @ Lbar)
    P[np.diag_indices(M)] *= 0.5
    Kbar = Li.T @ P @ Li
    Kbar = 0.5 * (Kbar + Kbar.T)
    kz = np.array([(Kbar * qz * u2z[..., d]).sum() for d in range(D)] + [(Kbar * K0).sum()])
    return pts, kz


@pytest.mark.parametrize("with_mu0", [False, True])
@pytest.mark.parametrize("kind", KR.KINDS)
def test_header_formulas_reproduce_both_halves(kind, with_mu0):
    c = _case(kind, 3, 2, seed=1)
    if not with_mu0:
        c["mu0"] = None
    ref = HR.gradient(**c)
    pts, kz = header_formulas(**c)
    assert np.all(np.abs(pts - ref["points"]) <= 1e-10 * ref["scale_points"]), (pts, ref["points"])
    assert np.all(np.abs(kz - ref["kzz"]) <= 1e-9 * ref["scale_kzz"]), (kz, ref["kzz"])


@pytest.mark.parametrize("broken", ["S=I", "no_kzz", "swap_ell"])
@pytest.mark.parametrize("kind", KR.KINDS)
def test_a_broken_gradient_misses_the_bar_a_hundredfold(kind, broken):
    """With the reference alone: each wrong gradient is at least 100 bars of scale away from the right one in some component
    (D = 3 inputs: 1.1e-2 of scale or more, measured; the bar is 1.44e-5)."""
    c = _case(kind, 3, 2)
    ref, bad = HR.gradient(**c), HR.gradient(**c, broken=broken)
    miss = np.max(np.abs(bad["grad"] - ref["grad"]) / ref["scale"])
    assert miss >= 100 * HR.HYPER_BAR, miss
