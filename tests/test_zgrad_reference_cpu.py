"""tests/zgrad_reference.py pinned on the CPU: its closed-form halves add up to autograd's gradient for z, autograd agrees with
central differences of its own bound, every deliberately wrong gradient misses the GPU bars a hundredfold, and a point placed
exactly on an inducing input (r = 0) gives a finite gradient with 0 for that term -- Matern-1/2 included; the points' part summed
over chunks of points (``points_part_chunked``, for N too large for [M, N, D] tensors) is ``gradient_z``'s."""
import numpy as np
import pytest
import torch

import hyper_reference as HR
import kernels_reference as KR
import zgrad_reference as ZR


def _case(kind, D, L, seed=0, N=150, M=12):
    rng = np.random.default_rng(100 * kind + 10 * D + L + seed)
    x = rng.uniform(-3, 3, size=(N, D))
    z = rng.uniform(-3, 3, size=(M, D))
    ell = np.array([1.1, 1.7, 0.8][:D])
    m, S, beta, gamma, mu0 = HR.synthetic_q(M, L, N, seed + 7)
    return dict(kind=kind, param=KR.param_of(kind), x=x, z=z, ell=ell, s2=1.3, jitter=1e-6, m=m, S=S, beta=beta, gamma=gamma, mu0=mu0)


@pytest.mark.parametrize("with_mu0", [False, True])
@pytest.mark.parametrize("L", [1, 2])
@pytest.mark.parametrize("D", [1, 3])
@pytest.mark.parametrize("kind", KR.KINDS)
def test_closed_form_is_autograd(kind, D, L, with_mu0):
    c = _case(kind, D, L)
    if not with_mu0:
        c["mu0"] = None
    ref = ZR.gradient_z(**c)
    err = np.abs(ref["points"] + ref["kzz"] - ref["grad"]) / ref["scale"]
    assert ref["grad"].shape == c["z"].shape and err.max() <= 1e-12, err.max()


@pytest.mark.parametrize("kind", KR.KINDS)
def test_autograd_against_central_differences(kind):
    c = _case(kind, 3, 2)
    ref = ZR.gradient_z(**c)
    args = {k: v for k, v in c.items() if k != "z"}
    f = lambda zz: float(ZR.bound_z(z=torch.as_tensor(zz), **args))
    h = 1e-5
    for a, d in [(0, 0), (3, 1), (7, 2), (11, 0)]:
        e = np.zeros_like(c["z"])
        e[a, d] = h
        fd = (f(c["z"] + e) - f(c["z"] - e)) / (2 * h)
        assert abs(fd - ref["grad"][a, d]) <= 1e-6 * ref["scale"][a, d], (a, d, fd, ref["grad"][a, d], ref["scale"][a, d])


@pytest.mark.parametrize("broken", ["S=I", "no_kzz", "sign", "ell_once"])
@pytest.mark.parametrize("kind", KR.KINDS)
def test_a_broken_gradient_misses_the_bar_a_hundredfold(kind, broken):
    """With the reference alone: each wrong gradient is at least 100 bars of scale away from the right one in some component.
    "no_kzz" is judged on the K_ZZ scale alone: with a synthetic q(v) the K_ZZ half is 1e-4 to 1e-2 of the points' half."""
    c = _case(kind, 3, 2)
    ref, bad = ZR.gradient_z(**c), ZR.gradient_z(**c, broken=broken)
    if broken == "no_kzz":
        miss, bar = np.max(np.abs(bad["grad"] - ref["grad"]) / ref["scale_kzz"]), ZR.ZGRAD_BAR_KZZ
    else:
        miss, bar = np.max(np.abs(bad["grad"] - ref["grad"]) / ref["scale"]), ZR.ZGRAD_BAR
    assert miss >= 100 * bar, (miss, bar)


@pytest.mark.parametrize("with_mu0", [False, True])
@pytest.mark.parametrize("kind", KR.KINDS)
def test_points_part_summed_over_chunks_is_gradient_z(kind, with_mu0):
    """N = 1000 in chunks of 128 (a ragged last chunk) and in one chunk of 1000.  The bar 1e-12 of scale_points: the two differ by
    the order of at most 1000 float64 additions per component, <= 1000 2^-53 = 1.1e-13 of the sum of |terms|."""
    c = _case(kind, 3, 2, N=1000)
    if not with_mu0:
        c["mu0"] = None
    ref = ZR.gradient_z(**c)
    for chunk in (128, 1000):
        got = ZR.points_part_chunked(**c, chunk=chunk)
        assert got["points"].shape == got["scale_points"].shape == c["z"].shape
        err = np.abs(got["points"] - ref["points"]) / ref["scale_points"]
        rel = np.abs(got["scale_points"] - ref["scale_points"]) / ref["scale_points"]
        assert err.max() <= 1e-12 and rel.max() <= 1e-12, (chunk, err.max(), rel.max())


@pytest.mark.parametrize("broken", ["S=I", "sign", "ell_once"])
@pytest.mark.parametrize("kind", KR.KINDS)
def test_a_broken_points_part_misses_the_bar_a_hundredfold_through_the_chunks(kind, broken):
    c = _case(kind, 3, 2, N=1000)
    ref, bad = ZR.gradient_z(**c), ZR.points_part_chunked(**c, broken=broken, chunk=128)
    miss = np.max(np.abs(bad["points"] - ref["points"]) / ref["scale_points"])
    assert miss >= 100 * ZR.ZGRAD_BAR_POINTS, (miss, ZR.ZGRAD_BAR_POINTS)
    with pytest.raises(ValueError):
        ZR.points_part_chunked(**c, broken="no_kzz")  # (the K_ZZ half is not part of this function)


@pytest.mark.parametrize("kind", KR.KINDS)
def test_a_point_on_an_inducing_input_contributes_zero(kind):
    c = _case(kind, 3, 1)
    c["z"][0] = c["x"][17]
    c["z"][5] = c["z"][2]  # two coincident inducing inputs (the jitter keeps K_ZZ positive definite)
    c["jitter"] = 1e-3
    ref = ZR.gradient_z(**c)
    for k in ("grad", "points", "kzz"):
        assert np.isfinite(ref[k]).all(), k
    err = np.abs(ref["points"] + ref["kzz"] - ref["grad"]) / ref["scale"]
    assert err.max() <= 1e-12, err.max()
    # the term of (a = 0, i = 17) is 0: row 0 of the points' part is the sum over every OTHER point of include/agpl_zgrad.h's terms,
    # with the weights W = gamma C phi + p b' of include/agpl_hyper.h formed here in numpy from all the points
    x, z, ell, s2, M = c["x"], c["z"], c["ell"], c["s2"], c["z"].shape[0]
    ux, uz = (z[:, None, :] - x[None, :, :]) / ell, (z[:, None, :] - z[None, :, :]) / ell
    r2x = (ux * ux).sum(-1)
    Li = np.linalg.inv(np.linalg.cholesky(s2 * HR.kappa(kind, torch.as_tensor((uz * uz).sum(-1)), c["param"]).numpy() + c["jitter"] * np.eye(M)))
    phi = Li @ (s2 * HR.kappa(kind, torch.as_tensor(r2x), c["param"]).numpy())
    b = c["beta"][0] - c["gamma"][0] * c["mu0"][0]
    W = c["gamma"][0] * (Li.T @ (np.eye(M) - c["S"][0] - np.outer(c["m"][0], c["m"][0])) @ phi) + np.outer(Li.T @ c["m"][0], b)
    others = np.arange(x.shape[0]) != 17
    assert r2x[0, 17] == 0.0
    with np.errstate(divide="ignore", invalid="ignore"):  # (not evaluated at r = 0: that point is left out)
        q0 = s2 * HR.dkappa_over_r(kind, torch.as_tensor(r2x[0, others]), c["param"]).numpy()
    row0 = ((W[0, others] * q0)[:, None] * ux[0, others] / ell).sum(0)
    assert np.all(np.abs(row0 - ref["points"][0]) <= 1e-9 * ref["scale_points"][0]), (row0, ref["points"][0])
