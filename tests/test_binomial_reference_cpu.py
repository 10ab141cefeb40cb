"""CPU checks of tests/binomial_reference.py, the float64 reference the GPU tests of the binomial likelihood compare with: it
reduces to the Bernoulli formulas at n = 1, its mass function sums to one and carries the moments it reports, the Polya-Gamma
identity behind the augmentation holds numerically, and the quantile cases of tests/test_gpu_binomial.py stay clear of the
tolerance at their answers."""
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import binomial_reference as B  # noqa: E402
import predictive_reference as PR  # noqa: E402

# the cdf / quantile cases of the GPU test, (n, mu, s); its levels; the cdf tolerance of tests/test_gpu_quantile.py for the count kinds
QUANTILE_CASES = [(1, -0.3, 0.7), (7, 0.4, 1.2), (7, -2.0, 0.3), (1000, 0.2, 0.8), (1000, -1.5, 1.5)]
LEVELS = (0.025, 0.5, 0.975)
CDF_TOL = 1e-8


@pytest.mark.parametrize("mu,var", [(-3.0, 0.5), (0.0, 2.0), (1.7, 0.0), (4.0, 9.0)])
def test_n1_reduces_to_bernoulli(mu, var):
    for y in (0, 1):
        lp, _ = B.ref_logp(1, y, mu, var)
        lb, _ = PR.ref_logp("bernoulli", (), float(y), mu, var)
        assert lp == pytest.approx(lb, abs=1e-12)
        assert B.logC(1, y) == 0.0
    me, va = B.ref_moments(1, mu, var)
    mb, vb = PR.ref_moments("bernoulli", (), mu, var)
    assert me == pytest.approx(mb, rel=1e-12) and va == pytest.approx(vb, rel=1e-10)
    # the per-point rules at b = 1: beta = +-1/2, theta = tanh(c / 2) / (2 c), the single-logcosh ELBO term
    c = B.aux_posterior(np.array([mu]), np.array([var + 0.1]))
    beta, gamma = B.expected_potential_precision(1, np.array([0.0, 1.0]), c)
    assert list(beta) == [-0.5, 0.5] and gamma[0] == pytest.approx(math.tanh(c[0] / 2) / (2 * c[0]), rel=1e-15)
    for y in (0.0, 1.0):
        e = B.elbo_terms(1, np.array([y]), np.array([mu]), np.array([var + 0.1]))
        assert e == pytest.approx(-math.log(2.0) + (mu if y else -mu) / 2.0 - float(B.logcosh(c / 2.0)[0]), rel=1e-13)


@pytest.mark.parametrize("n,mu,s", [(1, 0.3, 1.0), (2, -1.0, 0.5), (7, 0.4, 1.2), (1000, 0.2, 0.8), (1000, -1.5, 1.5), (1000, 3.0, 0.1)])
def test_mass_function_sums_to_one_and_carries_the_moments(n, mu, s):
    p = B.pmf_all(n, mu, s)
    assert abs(p.sum() - 1.0) < 1e-12
    ys = np.arange(n + 1, dtype=np.float64)
    mean = float(p @ ys)
    var = float(p @ (ys - mean) ** 2)
    me, va = B.ref_moments(n, mu, s * s)
    assert mean == pytest.approx(me, rel=1e-10) and var == pytest.approx(va, rel=1e-9)
    md, vd = B.ref_moments_direct(n, mu, s * s)
    assert md == pytest.approx(me, rel=1e-12) and vd == pytest.approx(va, rel=1e-9)
    # the grid rule against the adaptive integration, at the ends and in the middle
    for y in (0, n // 2, n):
        lp, err = B.ref_logp(n, y, mu, s * s)
        assert err < 1e-9
        if lp > -30.0:  # (a mass this small or smaller comes from f beyond the grid's mu +- 12 s: below anything a cdf bar sees)
            assert math.log(p[y]) == pytest.approx(lp, abs=1e-9)
    cdf, sf = B.cdf_all(n, mu, s)
    assert cdf[-1] == pytest.approx(1.0, abs=1e-12) and sf[-1] == 0.0
    assert np.allclose(cdf + sf, 1.0, atol=1e-12)


def test_counts_outside_the_support():
    assert B.logC(7, -1) == -math.inf and B.logC(7, 8) == -math.inf
    assert B.ref_logp(7, 8, 0.0, 1.0)[0] == -math.inf and B.ref_logp(7, -1, 0.0, 0.0)[0] == -math.inf
    assert B.logtilt(7, np.array([3.0, 9.0]), np.array([0.2, 0.2]), np.array([0.1, 0.1])) == -math.inf


@pytest.mark.parametrize("n,y,f", [(1, 0, 0.7), (1, 1, -1.3), (2, 1, 2.0), (7, 3, -0.6), (7, 7, 1.1), (1000, 430, -0.25)])
def test_polya_gamma_identity(n, y, f):
    lhs, rhs = B.pg_identity_sides(n, y, f)
    assert lhs > 0.0
    assert rhs == pytest.approx(lhs, rel=1e-9)  # (the product form of the Laplace transform, 2e6 factors + the first-order tail)


def test_quantile_cases_are_clear_of_the_tolerance():
    """At the answer y* of every (case, level) of the GPU test the reference's cdf is not within the tolerance of the level,
    neither at y* nor at y* - 1: a device cdf inside the tolerance gives the same integer."""
    for n, mu, s in QUANTILE_CASES:
        cdf, _ = B.cdf_all(n, mu, s)
        for p in LEVELS:
            q = B.quantile(cdf, p)
            assert 0 <= q <= n
            assert cdf[q] - p > 100 * CDF_TOL, (n, mu, s, p, q, cdf[q])
            if q > 0:
                assert p - cdf[q - 1] > 100 * CDF_TOL, (n, mu, s, p, q, cdf[q - 1])
