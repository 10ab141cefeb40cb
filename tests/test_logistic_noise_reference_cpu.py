"""tests/logistic_noise_reference.py held, without the device, to mpmath at 50 digits over the kind's domain grid, to scipy's own
adaptive rule where it reports a small error, to the Polya-Gamma identity through the product form of the PG(2) Laplace transform, to the symmetry of the
predictive about mu and to the exact variance of Gaussian plus logistic noise.

Bars: the reference serves device bars of 1e-4 (log p), 1e-4 relative (tails) and 2.5e-11 of max(1, |ref|) (expected
log-likelihood); its integrals are held, between two precisions, to 1e-9, 1e-9 relative down to 1e-300 and 2.5e-12, ten or more times tighter than each."""
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import logistic_noise_reference as R  # noqa: E402

pytest.importorskip("mpmath")


@pytest.fixture(scope="module")
def grid():
    return R.compute_grid()


def test_golden_grid_is_the_references(grid):
    """tests/golden/logistic_noise_grid.npy, which the GPU tests read, holds what the reference computes."""
    stored = R.grid()
    assert stored.shape == grid.shape and np.array_equal(stored[:, :3], grid[:, :3])
    assert np.allclose(stored[:, 3:], grid[:, 3:], rtol=1e-14, atol=0.0)


def test_grid_covers_the_domain(grid):
    assert len(grid) == 3 * 4 * 7
    r = np.sqrt(grid[:, 1]) / grid[:, 0]
    assert r.max() == 5e4 and (r == 0).sum() == 21  # s = 1e-3 under sqrt(var) = 50; var = 0


def test_reference_against_mpmath_on_the_grid(grid):
    """The 50-digit values against the same integrals at 65 digits (other nodes: the rule's degrees depend on the precision, so an
    integral that has not converged shows), every third point of the grid."""
    worst = dict(logp=0.0, tail=0.0, ell=0.0, dell=0.0)
    for s, var, y, lp, c, sf, ell, dell in grid[1::3]:
        worst["logp"] = max(worst["logp"], abs(R.logp(s, y, R.GRID_MU, var, 65) - lp))
        for got, want in zip(R.cdf(s, y, R.GRID_MU, var, 65), (c, sf)):
            if want >= 1e-300:
                worst["tail"] = max(worst["tail"], abs(got - want) / want)
        e, d = R.expected_loglik_point(s, y, R.GRID_MU, var, 65)
        worst["ell"] = max(worst["ell"], abs(e - ell) / max(1.0, abs(ell)))
        worst["dell"] = max(worst["dell"], abs(d - dell) / max(1.0, abs(dell)))
    print(f"LOGISTIC NOISE reference against mpmath, {len(grid)} points: {worst}")
    assert worst["logp"] <= 1e-9 and worst["tail"] <= 1e-9 and worst["ell"] <= 2.5e-12 and worst["dell"] <= 2.5e-12


def test_scipy_quadrature_agrees_where_it_reports_a_small_error(grid):
    """A second rule on the same integrals: wherever scipy reports a relative error below 1e-9 (and the value is a normal
    number), it agrees with the 50-digit value to 1e-7: its estimate covers truncation, not the rounding of some twenty pieces
    each asked for 1e-13, so a hundred times the reported figure is allowed; the device bars behind are 1e-4."""
    seen, worst = 0, 0.0
    for s, var, y, lp, c, sf, ell, dell in grid:
        if var == 0.0:
            continue
        vals, errs = R.scipy_terms(s, y, R.GRID_MU, var)
        for v, e, want in zip(vals, errs, (math.exp(lp) * s if lp > -650 else 0.0, c, sf)):
            if e < 1e-9 and want > 1e-290:
                seen += 1
                worst = max(worst, abs(v - want) / want)
    print(f"LOGISTIC NOISE scipy against mpmath: {seen} integrals, worst relative difference {worst:.3e}")
    assert seen >= 100 and worst <= 1e-7


def test_stein_form_of_the_gradient(grid):
    """d ell / d log s = -1 + m (2 e1 - 1) + 2 R^2 (e1 - e2), e1 - e2 = s p(y): the form the device uses, from the reference's own
    tails and density, against the directly integrated E[g tanh(g / 2)]."""
    for s, var, y, lp, c, sf, ell, dell in grid:
        m, R2 = (y - R.GRID_MU) / s, var / (s * s)
        stein = -1.0 + m * (c - sf) + 2.0 * R2 * s * math.exp(lp) if lp > -700 else -1.0 + m * (c - sf)
        assert abs(stein - dell) <= 1e-9 * max(1.0, abs(dell)), (s, var, y)


def test_symmetry_about_mu(grid):
    for s, var, y, lp, c, sf, ell, dell in grid:
        y2 = 2.0 * R.GRID_MU - y
        assert R.logp(s, y2, R.GRID_MU, var) == pytest.approx(lp, abs=1e-9)
        c2, sf2 = R.cdf(s, y2, R.GRID_MU, var)
        if c >= 1e-300:
            assert sf2 == pytest.approx(c, rel=1e-9)
        if sf >= 1e-300:
            assert c2 == pytest.approx(sf, rel=1e-9)


@pytest.mark.parametrize("z", [0.0, 0.3, -2.0, 7.5])
def test_polya_gamma_identity_through_the_product_form(z):
    s = 0.7
    lhs = math.exp(float(R.loglik(s, s * z + 0.2, 0.2)))
    rhs = R.pg2_laplace(z * z / 2.0) / (4.0 * s)
    assert lhs == pytest.approx(rhs, rel=1e-6)  # (the product's remainder beyond 2e6 factors is second order: t^2 / K^3)
    assert R.pg_mean2(abs(z)) == pytest.approx(0.5 if z == 0 else math.tanh(abs(z) / 2) / abs(z), rel=1e-15)
    # theta is minus the derivative of the log transform at t = c^2 / 2 (c = |z|)
    if z != 0.0:
        h = 1e-5 * z * z
        num = -(math.log(R.pg2_laplace(z * z / 2 + h)) - math.log(R.pg2_laplace(z * z / 2 - h))) / (2 * h)
        assert num == pytest.approx(float(R.pg_mean2(abs(z))), rel=1e-5)


def test_variance_is_gaussian_plus_logistic():
    from scipy import integrate

    s, mu, var = 0.6, 0.3, 1.7
    sd = math.sqrt(R.moments(s, mu, var)[1])
    dens = lambda y: math.exp(R.logp(s, y, mu, var))
    edges = [mu + k * sd for k in (-40, -12, -4, 0, 4, 12, 40)]
    tot = sum(integrate.quad(dens, a, b, epsabs=0, epsrel=1e-11)[0] for a, b in zip(edges, edges[1:]))
    second = sum(integrate.quad(lambda y: (y - mu) ** 2 * dens(y), a, b, epsabs=0, epsrel=1e-11)[0] for a, b in zip(edges, edges[1:]))
    assert tot == pytest.approx(1.0, abs=1e-9) and second == pytest.approx(var + s * s * math.pi ** 2 / 3.0, rel=1e-8)


def test_rules_and_the_elbo_cancellation():
    rng = np.random.default_rng(5)
    s = 0.4
    y, mu, var = rng.normal(size=50), rng.normal(size=50), rng.uniform(0.01, 3.0, size=50)
    c = R.aux_posterior(s, y, mu, var)
    single = float(np.sum(-math.log(4.0 * s) - 2.0 * R.logcosh(c / 2.0)))  # the fused kernel's form
    assert R.elbo_terms(s, y, mu, var) == pytest.approx(single, rel=1e-13)
    b, g = R.expected_potential_precision(s, y, c)
    assert np.allclose(b, g * y) and np.allclose(g * s * s * c, np.tanh(c / 2.0))
    u = rng.uniform(size=2000)
    e = (R.inverse_cdf(s, 0.0, u)) / s
    assert np.allclose(1.0 / (1.0 + np.exp(-e)), u, rtol=1e-12)
