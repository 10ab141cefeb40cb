"""The float64 reference of the predictive distribution function (tests/quantile_reference.py) on every point of
tests/quantile_domain.py, without a GPU: its two independent routes agree (the device's bar, 1e-8 absolute and 1e-4 relative, means
something only if they agree to 1e-10 and far below 1e-4), and the known answers hold.  DESIGN.md 4.25 records the worst
disagreement."""
import math

import numpy as np
import pytest
from scipy import special, stats

import quantile_domain as D
import quantile_reference as R


def test_the_grid():
    total = 0
    for kind in D.KINDS:
        names = [pt[0] for pt in D.GRID[kind]]
        assert len(set(names)) == len(names) and len(names) >= 24, (kind, len(names))
        total += sum(len(D.thresholds(kind, *pt[1:])) for pt in D.GRID[kind])
        flat = [(pt[2], pt[3]) if kind != "heterogauss" else (pt[2][0], pt[3][0]) for pt in D.GRID[kind]]
        s = {round(math.sqrt(v), 12) for _, v in flat}
        assert {0.0, 1e-6, 20.0} <= s and max(abs(m) for m, _ in flat) == 20.0  # var = 0, both ends of s, |mu| = 20
    assert total >= 700
    st = {pt[1] for pt in D.GRID["studentt"]}
    assert {nu for nu, _ in st} >= {0.5, 1e4} and {sg for _, sg in st} >= {0.01, 100.0}
    assert {pt[1][0] for pt in D.GRID["laplace"]} >= {1e-2, 10.0}
    het = D.GRID["heterogauss"]
    assert {pt[1][0] for pt in het} >= {1e-3, 1e3} and {pt[2][1] for pt in het} >= {-10.0, 10.0} and {pt[3][1] for pt in het} >= {0.0, 25.0}
    assert min(D.K) == -30.0 and max(D.K) == 30.0 and min(D.PROBS) == 1e-4 and max(D.PROBS) == 1.0 - 1e-4


@pytest.mark.parametrize("kind", D.KINDS)
def test_the_two_routes_agree_on_every_point(kind):
    worst_abs, worst_rel, n = (0.0, ""), (0.0, ""), 0
    for name, p, mu, var in D.GRID[kind]:
        prev = None
        for y in D.thresholds(kind, p, mu, var):
            a, b = R.ref_cdf(kind, p, y, mu, var, "a"), R.ref_cdf(kind, p, y, mu, var, "b")
            n += 1
            for u, v in zip(a, b):
                if abs(u - v) > worst_abs[0]:
                    worst_abs = (abs(u - v), f"{name} y={y:g}")
                if u >= 1e-12 and abs(u - v) / u > worst_rel[0]:
                    worst_rel = (abs(u - v) / u, f"{name} y={y:g}")
            assert abs(a[0] + a[1] - 1.0) <= 1e-14, (name, y, a)  # each tail integrated on its own
            assert 0.0 <= a[0] <= 1.0 + 1e-14 and 0.0 <= a[1] <= 1.0 + 1e-14
            if prev is not None:  # monotone in y
                assert a[0] >= prev[0] - 1e-15 and a[1] <= prev[1] + 1e-15, (name, y)
            prev = a
    print(f"{kind}: {n} (point, threshold) pairs, worst |a - b| {worst_abs[0]:.3e} at {worst_abs[1]}, worst relative (>= 1e-12) "
          f"{worst_rel[0]:.3e} at {worst_rel[1]}")
    assert worst_abs[0] <= 1e-10 and worst_rel[0] <= 1e-8


def test_count_grid_has_probs_well_inside_a_jump():
    """At least 90 % of the count kinds' (point, prob) pairs lie more than 1e-6 from both ends of their jump, so the 2e-8 band of the GPU
    test decides the neighbour for few of them."""
    tail = lambda ref, pj: ref[0] - pj if pj <= 0.5 else (1.0 - pj) - ref[1]
    for kind in D.COUNTS:
        n = inside = 0
        for name, p, mu, var in D.GRID[kind]:
            for pj in D.COUNT_PROBS:
                q = R.ref_count_quantile(kind, p, pj, mu, var, D.COUNT_CAP)
                if q is None:
                    continue
                n += 1
                up = tail(R.ref_cdf(kind, p, q, mu, var), pj)
                dn = -tail(R.ref_cdf(kind, p, q - 1, mu, var), pj)
                inside += up > 1e-6 and dn > 1e-6
        print(f"{kind}: {inside} of {n} (point, prob) pairs with a margin above 1e-6 to both sides")
        assert n >= 60 and inside >= 0.9 * n, (kind, inside, n)
    st = {pt[1][0] for pt in D.GRID["poisson"]}, {pt[1][0] for pt in D.GRID["negbinomial"]}
    assert st[0] >= {1e-3, 1e5} and st[1] >= {1e-2, 1e3} and D.COUNT_CAP == 100000


def test_named_tail_points_in_30_digits():
    """The relative bar is claimed in the tails: three named tail points against mpmath.quad at 30 digits."""
    import mpmath

    def mp_tail(fn, lo, hi, brk):
        with mpmath.workdps(30):
            return float(mpmath.quad(fn, [lo] + sorted(brk) + [hi]))

    # Student-t nu = 0.5, 30 scales out: the mixture over tau = log w
    kind, (name, p, mu, var) = "studentt", D.GRID["studentt"][1]
    y = D.thresholds(kind, p, mu, var)[-1]
    a, d = 0.5 * p[0], y - mu
    fn = lambda t: mpmath.exp(a * mpmath.log(a) - a - mpmath.loggamma(a) - a * (mpmath.expm1(t) - t)) * mpmath.ncdf(-d / mpmath.sqrt(var + p[1] ** 2 * mpmath.exp(-t)))
    want = mp_tail(fn, -400.0, 8.0, [-200.0, -100.0, -50.0, -25.0, -12.0, -6.0, -3.0, 0.0, 3.0])
    assert abs(R.ref_cdf(kind, p, y, mu, var)[1] - want) <= 1e-9 * want, (name, want)
    # heteroscedastic lambda = 1e-3, both 30-scale thresholds: over g
    kind = "heterogauss"
    for name, p, mu, var in D.GRID[kind][:2]:
        if var[1] == 0.0:
            continue
        for y, side in ((D.thresholds(kind, p, mu, var)[0], 0), (D.thresholds(kind, p, mu, var)[-1], 1)):
            sg, d = math.sqrt(var[1]), y - mu[0]
            fn = lambda x: mpmath.npdf(x) * mpmath.ncdf((-1) ** side * d / mpmath.sqrt(var[0] + (1 + mpmath.exp(-(mu[1] + sg * x))) / p[0]))
            want = mp_tail(fn, -14.0, 14.0, [-8.0, -4.0, -2.0, 0.0, 2.0, 4.0, 8.0])
            assert abs(R.ref_cdf(kind, p, y, mu, var)[side] - want) <= 1e-9 * want, (name, y, want)


def test_known_answers():
    # counts at var = 0: the likelihood's own distribution function; a count below 0
    for y in (0, 3, 40):
        c, s = R.ref_cdf("poisson", (30.0,), y, 0.4, 0.0)
        d = stats.poisson(30.0 * special.expit(0.4))
        assert abs(c - d.cdf(y)) <= 1e-14 and abs(s - d.sf(y)) <= 1e-14
        c, s = R.ref_cdf("negbinomial", (2.5,), y, 0.4, 0.0)
        d = stats.nbinom(2.5, special.expit(-0.4))
        assert abs(c - d.cdf(y)) <= 1e-14 and abs(s - d.sf(y)) <= 1e-14
    assert R.ref_cdf("poisson", (3.0,), -1, 0.0, 1.0) == (0.0, 1.0)
    # var = 0: the likelihood's own distribution function
    for y in (-3.0, 0.2, 7.0):
        c, s = R.ref_cdf("studentt", (3.0, 0.5), y, 0.4, 0.0)
        assert abs(c - stats.t.cdf(y, 3.0, loc=0.4, scale=0.5)) <= 1e-15 and abs(s - stats.t.sf(y, 3.0, loc=0.4, scale=0.5)) <= 1e-15
        c, s = R.ref_cdf("laplace", (0.7,), y, 0.4, 0.0)
        assert abs(c - stats.laplace.cdf(y, loc=0.4, scale=0.7)) <= 1e-15 and abs(s - stats.laplace.sf(y, loc=0.4, scale=0.7)) <= 1e-15
        c, s = R.ref_cdf("heterogauss", (2.0,), y, (0.4, -1.0), (0.3, 0.0))
        sd = math.sqrt(0.3 + (1.0 + math.e) / 2.0)
        assert abs(c - stats.norm.cdf(y, 0.4, sd)) <= 1e-15 and abs(s - stats.norm.sf(y, 0.4, sd)) <= 1e-15
    assert R.ref_cdf("bernoulli", (0.0,), 0, 1.0, 0.0) == (float(special.expit(-1.0)), float(special.expit(1.0)))
    # Laplace with beta small against s: the Gaussian q(f) itself; Student-t with nu large: N(mu, var + sigma^2)
    for route in ("a", "b"):
        c, s = R.ref_cdf("laplace", (1e-7,), 1.3, 0.4, 0.49, route)
        assert abs(c - stats.norm.cdf(0.9 / 0.7)) <= 1e-12 and abs(s - stats.norm.sf(0.9 / 0.7)) <= 1e-12
        c, _ = R.ref_cdf("studentt", (1e7, 0.5), 1.3, 0.4, 0.49, route)  # (Student-t and normal differ by O(1 / nu) = 1e-8 here)
        assert abs(c - stats.norm.cdf(0.9 / math.sqrt(0.74))) <= 1e-6
    # the quantile reference inverts the distribution function; Bernoulli: the jump
    for kind, idx in (("studentt", 2), ("laplace", 9), ("heterogauss", 5)):
        name, p, mu, var = D.GRID[kind][idx]
        for prob in D.PROBS:
            q = R.ref_quantile(kind, p, prob, mu, var, D.scale(kind, p, mu, var))
            c, s = R.ref_cdf(kind, p, q, mu, var)
            assert (abs(c - prob) if prob <= 0.5 else abs(s - (1.0 - prob))) <= 1e-13, (name, prob)
    assert R.ref_quantile("bernoulli", (0.0,), 0.2, 1.0, 0.0, 1.0) == 0.0 and R.ref_quantile("bernoulli", (0.0,), 0.3, 1.0, 0.0, 1.0) == 1.0
    q = np.array([R.ref_quantile("studentt", (1.5, 0.5), pr, 0.0, 1.0, 1.0) for pr in D.PROBS])
    assert (np.diff(q) > 0).all() and abs(q[2]) <= 1e-12
