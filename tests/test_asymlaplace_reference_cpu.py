"""The float64 reference of the asymmetric Laplace likelihood (tests/asymlaplace_reference.py) checked against itself, on the CPU:
the density is one, the closed forms of the prediction end agree with quadrature of the defining integrals and with mpmath at 50
digits over the grid the GPU test uses, tau = 1/2 is the Laplace likelihood at beta = 2 sigma as the project's own references
know it, the sweep built from the rules ascends its bound, and the fitted quantile curves are ordered.

Bars.  The GPU test holds the device to this reference at 1e-4 (log p, absolute), 1e-8 absolute and 1e-4 relative from 1e-12 up
(cdf, sf).  A reference is fit to judge at a bar if its own error is a thousandth of it: here the closed forms are held to mpmath
at 1e-7 (log p), 1e-11 absolute and 1e-7 relative from 1e-12 up (cdf, sf), and where scipy's quadrature reports a relative error
below 1e-9 the closed forms are held to it at the same bars."""
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import asymlaplace_reference as R  # noqa: E402

LOGP_BAR, CDF_ABS, CDF_REL, CDF_FLOOR = 1e-7, 1e-11, 1e-7, 1e-12
LEVELS = (0.1, 0.5, 0.9)


@pytest.mark.parametrize("tau", R.TAUS)
def test_density_is_one_and_the_location_is_the_tau_quantile(tau):
    from scipy import integrate

    for sigma in (0.3, 1.0, 7.0):
        f = -0.4
        w = 60.0 * sigma / min(tau, 1.0 - tau)
        dens = lambda y: math.exp(float(R.loglik(sigma, tau, y, f)))
        lo, _ = integrate.quad(dens, f - w, f, epsabs=0, epsrel=1e-13)
        hi, _ = integrate.quad(dens, f, f + w, epsabs=0, epsrel=1e-13)
        assert lo + hi == pytest.approx(1.0, abs=1e-12) and lo == pytest.approx(tau, rel=1e-12)
        c, s = R.cdf(sigma, tau, f, f, 0.0)
        assert c == pytest.approx(tau, rel=1e-15) and s == pytest.approx(1.0 - tau, rel=1e-15)
        # the closed moments
        m1, _ = integrate.quad(lambda y: y * dens(y), f - w, f + w, points=[f], epsabs=0, epsrel=1e-12)
        m2, _ = integrate.quad(lambda y: y * y * dens(y), f - w, f + w, points=[f], epsabs=0, epsrel=1e-12)
        me, va = R.moments(sigma, tau, f, 0.0)
        assert m1 == pytest.approx(me, rel=1e-9, abs=1e-9) and m2 - m1 * m1 == pytest.approx(va, rel=1e-8)


def _tail_ok(got, want):
    return abs(got - want) <= CDF_ABS and (want < CDF_FLOOR or abs(got - want) <= CDF_REL * want)


def test_closed_forms_against_mpmath_over_the_grid():
    g = R.grid()
    assert len(g) == len(R.SIGMAS) * len(R.TAUS) * len(R.VARS) * len(R.DS)
    worst = dict(logp=0.0, cdf=0.0, sf=0.0)
    for sigma, tau, var, y, lp, c, s in g:
        lp_c = R.logp(sigma, tau, y, R.GRID_MU, var)
        c_c, s_c = R.cdf(sigma, tau, y, R.GRID_MU, var)
        worst["logp"] = max(worst["logp"], abs(lp_c - lp))
        assert abs(lp_c - lp) <= LOGP_BAR, (sigma, tau, var, y, lp_c, lp)
        for k, got, want in (("cdf", c_c, c), ("sf", s_c, s)):
            worst[k] = max(worst[k], abs(got - want))
            assert _tail_ok(got, want), (k, sigma, tau, var, y, got, want)
    print(f"ASYMLAPLACE closed forms against mpmath, {len(g)} points: worst |log p| {worst['logp']:.3e}, cdf {worst['cdf']:.3e}, sf {worst['sf']:.3e}")


def test_closed_forms_against_quadrature_over_the_grid():
    n = dict(logp=0, tail=0)
    for sigma, tau, var, y, lp, c, s in R.grid():
        if var == 0.0:
            continue
        v, err = R.logp_quad(sigma, tau, y, R.GRID_MU, var)
        if err < 1e-9:
            n["logp"] += 1
            assert abs(R.logp(sigma, tau, y, R.GRID_MU, var) - v) <= LOGP_BAR, (sigma, tau, var, y)
        (cq, sq), errs = R.cdf_quad(sigma, tau, y, R.GRID_MU, var)
        for got, want, e in zip(R.cdf(sigma, tau, y, R.GRID_MU, var), (cq, sq), errs):
            if e < 1e-9:
                n["tail"] += 1
                assert _tail_ok(got, want), (sigma, tau, var, y, got, want)
    print(f"ASYMLAPLACE closed forms against scipy quad: {n['logp']} densities and {n['tail']} tails had a quadrature to be held to")
    assert n["logp"] >= 150 and n["tail"] >= 300


@pytest.mark.parametrize("case", [(1e-3, 0.99, 1e4, 40.0), (1e-3, 0.01, 1e4, -40.0), (1.0, 0.1, 1e-8, 8.0), (50.0, 0.9, 1.0, -1.0), (1.0, 0.5, 1.0, 0.0)])
def test_edge_densities_against_mpmath_quadrature(case):
    """The defining integral itself at 50 digits, where double-precision quadrature has nothing to say."""
    sigma, tau, var, u = case
    y = R.GRID_MU + u * math.sqrt(var + sigma * sigma)
    assert abs(R.mp_logp_quad(sigma, tau, y, R.GRID_MU, var) - R.mp_terms(sigma, tau, y, R.GRID_MU, var)[0]) <= LOGP_BAR


def test_tau_half_is_the_laplace_reference(oracle):
    """At tau = 1/2 every rule is the Laplace kind's at beta = 2 sigma: the oracle's operators, the quadrature references of the
    predictive, the distribution function and the expected log-likelihood."""
    import likgrad_reference as LG
    import predictive_reference as PR
    import quantile_reference as QR

    rng = np.random.default_rng(5)
    n = 64
    for sigma in (0.25, 3.0):
        lap = oracle.laplace(2.0 * sigma)
        y, f, mu, var = rng.normal(size=n), rng.normal(size=n), rng.normal(size=n), rng.uniform(0.05, 2.0, size=n)
        omega = rng.uniform(0.1, 3.0, size=n)
        o1 = R.aux_posterior(sigma, y, mu, var)
        assert np.allclose(o1, oracle.aux_posterior(lap, y, mu, var)[0], rtol=1e-14, atol=0)
        for got, want in zip(R.expected_potential_precision(sigma, 0.5, y, o1), oracle.expected_potential_precision(lap, y, o1)):
            assert np.allclose(got, np.ravel(want), rtol=1e-14, atol=1e-300)
        for got, want in zip(R.sampled_potential_precision(sigma, 0.5, y, omega), oracle.potential_precision(lap, y, omega)):
            assert np.allclose(got, np.ravel(want), rtol=1e-14, atol=1e-300)
        assert R.logtilt(sigma, 0.5, y, omega, f) == pytest.approx(oracle.logtilt(lap, y, omega, f), rel=1e-13)
        assert R.expected_logtilt(sigma, 0.5, y, o1, mu, var) == pytest.approx(oracle.expected_logtilt(lap, y, o1, None, mu, var), rel=1e-13)
        assert R.aux_kl(sigma, o1) == pytest.approx(oracle.aux_kl(lap, y, o1), rel=1e-13)
        assert R.aux_prior_logpdf(sigma, omega) == pytest.approx(oracle.aux_prior_logpdf(lap, y, omega), rel=1e-13)
        assert R.aug_loglik(sigma, 0.5, y, omega, f) == pytest.approx(oracle.aug_loglik(lap, y, omega, f), rel=1e-13)
        for i in range(6):
            lp = PR.ref_logp("laplace", (2.0 * sigma,), y[i], mu[i], var[i])[0]
            assert R.logp(sigma, 0.5, y[i], mu[i], var[i]) == pytest.approx(lp, abs=1e-9)
            c, s = QR.ref_cdf("laplace", (2.0 * sigma,), float(y[i]), float(mu[i]), float(var[i]))
            assert R.cdf(sigma, 0.5, y[i], mu[i], var[i]) == pytest.approx((c, s), abs=1e-10)
        ell, dell = R.expected_loglik(sigma, 0.5, y, mu, var)
        for i in range(n):
            ea = LG.laplace_closed(2.0 * sigma, y[i], mu[i], var[i]) / (2.0 * sigma)  # Laplace: ell = -E|y - f| / beta - log(2 beta)
            assert ell[i] == pytest.approx(-ea - math.log(4.0 * sigma), rel=1e-13) and dell[i] == pytest.approx(-1.0 + ea, rel=1e-12, abs=1e-13)
        me, va = R.moments(sigma, 0.5, mu, var)
        assert np.array_equal(me, mu) and np.allclose(va, var + 2.0 * (2.0 * sigma) ** 2, rtol=1e-15)
        u = rng.uniform(size=n)
        d = u - 0.5
        assert np.allclose(R.inverse_cdf(sigma, 0.5, f, u), f - 2.0 * sigma * np.sign(d) * np.log1p(-2.0 * np.abs(d)), rtol=1e-15)


@pytest.fixture(scope="module")
def problem():
    return R.heteroscedastic_problem()


@pytest.mark.parametrize("tau", [0.05, 0.5, 0.9])
def test_the_reference_sweep_ascends_its_bound(problem, tau):
    _, y, Phi, kd, _ = problem
    ref = R.cavi_sweeps(0.3, tau, Phi, kd, y, 11)
    e = ref["elbo"]
    assert len(e) == 11 and all(b >= a - 1e-12 * abs(a) for a, b in zip(e, e[1:])), e
    assert e[-1] > e[0]


def test_the_reference_gibbs_sweep_orders_the_levels(problem):
    """The sampler built from the same rules: with everything else equal (the generator's state included) the posterior mean of f
    under tau = 0.9 lies above the one under tau = 0.1 on average over the points, and the share of y below it is the larger."""
    _, y, Phi, kd, _ = problem
    lo, hi = (R.gibbs_sweeps(0.15, tau, Phi, kd, y, 300, np.random.default_rng(3))[100:].mean(0) for tau in (0.1, 0.9))
    assert np.isfinite(lo).all() and np.isfinite(hi).all()
    assert hi.mean() > lo.mean() and np.mean(y < hi) > np.mean(y < lo)


def test_quantile_curves_are_ordered(problem):
    """The curves for tau = 0.1, 0.5, 0.9 on the heteroscedastic data: ordered at every test input.  The share of the training y
    below each fitted curve is printed (DESIGN.md 4.30 records it); no coverage bar is fixed."""
    x, y, Phi, kd, feats = problem
    xs = np.linspace(-3.0, 3.0, 121)
    Ps = feats(xs)
    curves, shares = [], []
    for tau in LEVELS:
        fit = R.cavi_sweeps(0.15, tau, Phi, kd, y, 60)
        curves.append(Ps @ fit["m"][-1])
        shares.append(float(np.mean(y < Phi @ fit["m"][-1])))
    print("ASYMLAPLACE quantile curves, N = 600, M = 32: share of training y below the fitted curve for tau = 0.1, 0.5, 0.9: "
          + ", ".join(f"{s:.3f}" for s in shares))
    assert (curves[0] < curves[1]).all() and (curves[1] < curves[2]).all()
