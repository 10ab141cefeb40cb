"""CPU checks that hold tests/binomial_n_reference.py (the float64 restatement of the per-point binomial kind): the mass function
sums to one at every point, the moments are the mass function's, and the expansion identity -- n_i Bernoulli rows that share
(mu, var) carry n_i E PG(1, c) = E PG(n_i, c) and sum(y01 - 1/2) = y_i - n_i / 2, so the sweeps of the expanded data are the
sweeps of the counts."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import binomial_n_reference as R  # noqa: E402
import binomial_reference as B  # noqa: E402

POINTS = [(1, -0.7, 0.3), (2, 0.4, 1.0), (7, 2.5, 0.5), (64, -1.0, 2.0), (65, 0.2, 0.1), (1000, 1.5, 1.0)]


@pytest.mark.parametrize("n,mu,s", POINTS)
def test_mass_function_sums_to_one_and_gives_the_moments(n, mu, s):
    p = R.pmf(n, mu, s)
    assert p.shape == (n + 1,) and (p >= 0).all()
    assert abs(p.sum() - 1.0) < 1e-9
    ys = np.arange(n + 1.0)
    mean, var = R.moments(n, mu, s * s)
    m1 = float(p @ ys)
    assert abs(m1 - mean) <= 1e-8 * max(1.0, abs(mean))
    assert abs(float(p @ (ys - m1) ** 2) - var) <= 1e-7 * max(1.0, var)


def test_rules_per_point_are_the_constant_n_rules():
    rng = np.random.default_rng(5)
    trials = rng.choice([1, 2, 7, 1000], size=200)
    y = rng.integers(0, trials + 1).astype(np.float64)
    c = rng.uniform(0.0, 3.0, size=200)
    beta, gamma = R.expected_potential_precision(trials, y, c)
    for n, idx in R.by_trials(trials):
        b, g = B.expected_potential_precision(n, y[idx], c[idx])
        assert np.array_equal(beta[idx], b) and np.array_equal(gamma[idx], g)


def test_expansion_into_bernoulli_rows_gives_the_same_sweeps():
    rng = np.random.default_rng(11)
    N0, M = 120, 16
    trials = rng.integers(1, 6, size=N0)
    y = rng.integers(0, trials + 1)
    y[:2] = (0, trials[1])
    Phi = rng.normal(size=(N0, M)) / np.sqrt(M)
    kd = rng.uniform(0.05, 0.3, size=N0)
    y01, Phi_x, kd_x = R.expand(trials, y, Phi, kd)
    assert len(y01) == trials.sum() and np.array_equal(np.add.reduceat(y01.astype(int), np.cumsum(trials) - trials), y)
    a = R.cavi_sweeps(trials, Phi, kd, y, 10)
    b = B.cavi_sweeps(1, Phi_x, kd_x, y01, 10, bernoulli=True)
    for k in ("G", "g", "S", "m"):
        for it in (0, 9):
            assert np.abs(a[k][it] - b[k][it]).max() <= 1e-10 * max(1.0, np.abs(b[k][it]).max()), (k, it)
