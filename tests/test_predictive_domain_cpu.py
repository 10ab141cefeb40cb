"""CPU proof of the domain tests of agpl_predictive: the float64 reference of tests/predictive_domain_reference.py
against mpmath and against closed forms on every point of tests/predictive_domain.py; the numpy twin of the kernel's arithmetic
(tools/predictive_twin.py) over the whole grid at the bars of the GPU module; the twin's constants against the .hip source; the
evaluation count inside the old box; the rows the parent commit's rules fail; and named wrong variants.  No GPU."""
import os
import re
import sys

import numpy as np
import pytest
from scipy import stats

import predictive_domain as D
import predictive_domain_reference as Q
import predictive_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import predictive_twin as T  # noqa: E402

HIP = os.path.join(ROOT, "augmentedgplikelihoods.jl_amd", "csrc", "agpl_predictive.hip")


def _cls(x):
    return "nan" if np.isnan(x) else ("+inf" if x == np.inf else ("-inf" if x == -np.inf else "finite"))


def _bars(kind, p, y, mu, var, ref):
    """Every figure of one point in units of its bar; the classes of the moments must be the reference's."""
    lp_r, me_r, va_r = ref
    me, va, lp = T.twin(kind, p, y, mu, var)
    out = {"logp": abs(lp - lp_r) / 1e-4 if np.isfinite(lp) else np.inf}
    for key, got, want in (("mean", me, me_r), ("var", va, va_r)):
        out[key] = (abs(got - want) / (1e-5 * abs(want) + 1e-9) if np.isfinite(want) else 0.0) if _cls(got) == _cls(want) else np.inf
    return out


def _agree_bar(kind, p, y, lp):
    """The two references must agree to the issue's absolute 1e-10, plus what float64 cannot hold: the reference adds the count's
    constant (up to 4e10) to the rest of log p in float64, 16 roundings of M = |log p| + 2 |constant| at most (4.23)."""
    return 1e-10 + 16 * np.finfo(np.float64).eps * (abs(lp) + 2.0 * abs(Q.log_count_const(kind, p, y)))


@pytest.fixture(scope="module")
def reference():
    """(log p, mean, variance, error estimate) of every grid point, computed once."""
    out = {}
    for kind in R.KINDS:
        for name, p, y, mu, var in D.points(kind):
            lp, er = Q.ref_logp(kind, p, y, mu, var)
            out[kind, name] = (lp, *Q.ref_moments(kind, p, mu, var), er)
    return out


def test_constants_are_the_kernels():
    src = open(HIP).read()
    want = {"kGrid": T.GRID, "kRecentre": T.RECENTRE, "kNewton": T.NEWTON, "kMaxHalf": T.MAXHALF, "kSpan": T.SPAN, "kPoleCap": T.POLE_CAP,
            "kNewtonTol": T.NEWTON_TOL, "kBracket": T.BRACKET, "kStNewton": T.ST_NEWTON, "kStMaxHalf": T.ST_MAXHALF, "kStStep": T.ST_STEP, "kStDrop": T.ST_DROP}
    for name, value in want.items():
        m = re.search(r"^constexpr\s+(?:int|double)\s+" + name + r"\s*=\s*([-+.\deE]+);", src, flags=re.M)
        assert m, f"{name} is not stated in agpl_predictive.hip"
        assert float(m.group(1)) == float(value), (name, m.group(1), value)
    assert "kStPoints" not in src  # the fixed 96-point Student-t rule is gone


def test_the_grid():
    for kind in R.KINDS:
        names = [pt[0] for pt in D.GRID[kind]]
        assert len(set(names)) == len(names) and 40 <= len(names) <= 120, (kind, len(names))
        assert set(D.REMOVED[kind]) <= set(names) and len(D.REMOVED[kind]) <= 0.02 * len(names)
        # the corners of the old box
        have = {(pt[1], pt[3], pt[4]) for pt in D.GRID[kind]}
        for p, _, _, _ in R.box_cases(kind, 8, 0):
            for mu in (4.0, -4.0):
                for s in (0.05, 2.0):
                    if kind == "heterogauss":
                        assert any((p, (mu, mg), (s * s, sg * sg)) in have for mg in (4.0, -4.0) for sg in (0.05, 2.0)), (kind, p, mu, s)
                    else:
                        assert (p, mu, s * s) in have, (kind, p, mu, s)


@pytest.mark.parametrize("kind", R.KINDS)
def test_reference_against_mpmath(reference, kind):
    worst, werr = (0.0, ""), (0.0, "")
    for name, p, y, mu, var in D.points(kind):
        lp, _, _, er = reference[kind, name]
        d = abs(Q.mp_logp(kind, p, y, mu, var) - lp) / _agree_bar(kind, p, y, lp)
        worst, werr = max(worst, (d, name)), max(werr, (er, name))
    print(f"{kind}: worst |reference - mpmath| in units of 1e-10 + 16 eps M {worst[0]:.2e} at {worst[1]}, error estimate {werr[0]:.2e} at {werr[1]}")
    assert worst[0] <= 1.0 and werr[0] <= 1e-9


FAR_MODES = [("negbinomial", "r15_y60_mu-40_s2"), ("negbinomial", "r10000_y60_mu40_s50"), ("poisson", "lam1e+06_y500000_mu40_s2"),
             ("poisson", "lam3_y60_mu-40_s2"), ("bernoulli", "y1_mu-300_s50")]


def test_far_modes_without_the_float64_set_up(reference):
    """mp_logp takes its break points from the float64 mode search; here mpmath gets none of it: mu +- 40 s in steps of 2 s, and the
    likelihood's own maximum +- 4^k of its own width."""
    for kind, name in FAR_MODES:
        (_, p, y, mu, var), = [pt for pt in D.points(kind) if pt[0] == name]
        got = Q.mp_logp_unguided(kind, p, y, mu, var)
        lp = reference[kind, name][0]
        print(f"{kind} {name}: unguided mpmath - reference {got - lp:.2e}")
        assert abs(got - lp) <= _agree_bar(kind, p, y, lp), (kind, name, got, lp)


def test_reference_against_closed_forms(reference):
    # Student-t at nu = 1e6 against N(y; mu, var + sigma^2): log t_nu(z) - log N(z) = (z^4 / 4 - z^2 / 2 - 1 / 4) / nu + O(z^6 / nu^2) at
    # every f, z = (y - f) / sigma, and q(f) holds f within 8 s of mu up to exp(-32): the bound at the largest such |z|
    n = 0
    for name, p, y, mu, var in D.points("studentt"):
        z = (abs(y - mu) + 8.0 * np.sqrt(var)) / p[1]
        if p[0] == 1e6 and z <= 8.0:
            want = stats.norm.logpdf(y, mu, np.sqrt(var + p[1] ** 2))
            assert abs(reference["studentt", name][0] - want) <= (z ** 4 / 4 + z ** 2 / 2 + 0.25) / p[0] + z ** 6 / (3 * p[0] ** 2) + 1e-12, name
            n += 1
    assert n >= 3
    # var -> 0: the likelihood at mu, up to s^2 |d2 log p / df2| / 2 <= s^2 (A + B + Lam) / 8 for the logistic kinds
    for kind in ("bernoulli", "negbinomial", "poisson"):
        for name, p, y, mu, var in D.points(kind):
            if var == 1e-16:
                A, B, L = Q._abl(kind, p, float(y))
                want = Q.log_count_const(kind, p, y) + Q._core(kind, p, float(y), mu)
                assert abs(reference[kind, name][0] - want) <= var * (A + B + L) + 1e-13 * max(1.0, abs(want)), (kind, name)
    # the log-normal moments of the negative binomial against a direct integration, where nothing overflows
    for r, mu, var in ((15.0, -1.0, 4.0), (1e-3, 4.0, 0.0025)):
        m1 = Q._gauss_mean(np.exp, mu, np.sqrt(var))
        m2 = Q._gauss_mean(lambda f: np.exp(2.0 * f), mu, np.sqrt(var))
        me, va = Q.ref_moments("negbinomial", (r,), mu, var)
        assert abs(me - r * m1) <= 1e-11 * me and abs(va - (r * (m1 + m2) + r * r * (m2 - m1 * m1))) <= 1e-9 * va
    assert Q.ref_moments("negbinomial", (15.0,), -1.0, 2500.0) == (np.inf, np.inf)


@pytest.mark.parametrize("kind", R.KINDS)
def test_twin_over_grid(reference, kind):
    worst = {"logp": (0.0, ""), "mean": (0.0, ""), "var": (0.0, "")}
    bad = []
    for name, p, y, mu, var in D.points(kind):
        figs = _bars(kind, p, y, mu, var, reference[kind, name][:3])
        for key, f in figs.items():
            worst[key] = max(worst[key], (f, name))
            if not f <= 1.0:
                bad.append((name, key, f))
    print(f"{kind}: twin over {len(D.points(kind))} points, worst in units of the bar: " + ", ".join(f"{k} {f:.2e} at {w}" for k, (f, w) in worst.items()))
    assert not bad, bad


def test_evaluations_inside_the_old_box_do_not_grow():
    # the parent's counts: Student-t 96; the logistic / heteroscedastic kinds 65 per seed grid (at least as many grids as now) + 13
    # (Newton) + 2 nh + 1 with nh from the spacing min(w / 2, s / 4), plus 65 for the moments of Bernoulli and Poisson.  The twin
    # states that count beside its own for every point.  (The model was held once against the parent commit's own twin with its
    # evaluations counted, over box_cases(kind, 60, 5): equal at every point.)
    for kind in R.KINDS:
        most = 0
        for p, y, mu, var in R.box_cases(kind, 800, 7):
            for i in range(len(y)):
                T.twin(kind, p, y[i], mu[i], var[i])
                assert T.EVALS <= (T.ST_POINTS_PARENT if kind == "studentt" else T.PARENT_EVALS), (kind, p, T.EVALS, T.PARENT_EVALS)
                most = max(most, T.EVALS)
        print(f"{kind}: at most {most} evaluations per point inside the old box")


# the rows of the issue's table: (kind, p, y, mu, var, the variant that restates the parent's rule, the figure that fails)
PARENT_ROWS = [("studentt", (300.0, 0.5), 0.7, 0.2, 0.3, "parent_studentt", "logp"), ("studentt", (1e3, 0.5), 0.7, 0.2, 0.3, "parent_studentt", "logp"),
               ("studentt", (1e4, 0.5), 0.7, 0.2, 0.3, "parent_studentt", "logp"), ("studentt", (1e6, 0.5), 0.7, 0.2, 0.3, "parent_studentt", "logp"),
               ("studentt", (0.01, 0.5), 0.7, 0.2, 0.3, "parent_studentt", "logp"),
               ("bernoulli", (0.0,), 1, 0.0, 100.0, "spacing_s4", "logp"), ("bernoulli", (0.0,), 1, 0.0, 2500.0, "spacing_s4", "logp"),
               ("bernoulli", (0.0,), 1, 10.0, 100.0, "spacing_s4", "mean"), ("bernoulli", (0.0,), 1, 10.0, 2500.0, "spacing_s4", "mean"),
               ("poisson", (3.0,), 1, 1.0, 100.0, "spacing_s4", "mean"), ("poisson", (3.0,), 1, 1.0, 2500.0, "spacing_s4", "mean"),
               ("heterogauss", (2.0,), 1.0, (0.2, -1.0), (0.3, 100.0), "spacing_s4", "logp")]


def test_the_parents_rules_fail_the_tabled_rows():
    """The Student-t rows run the parent's rule itself (`parent_studentt`).  The logistic and heteroscedastic rows run `spacing_s4`:
    the parent's spacing on today's mode search (bracketed Newton, doubling grid), not the parent's twin; at these rows the mode is
    the same and the spacing is what fails."""
    for kind, p, y, mu, var, variant, key in PARENT_ROWS:
        ref = (Q.ref_logp(kind, p, y, mu, var)[0], *Q.ref_moments(kind, p, mu, var))
        assert max(_bars(kind, p, y, mu, var, ref).values()) <= 1.0, (kind, p, mu, var)
        T.VARIANT = variant
        try:
            figs = _bars(kind, p, y, mu, var, ref)
        finally:
            T.VARIANT = None
        print(f"parent's rule at {kind} {p} y {y} mu {mu} var {var}: {key} {figs[key]:.3g} bars")
        assert figs[key] > 1.0, (kind, p, mu, var, figs)
    # the negative binomial's variance where the mean overflows
    with np.errstate(all="ignore"):
        m1, m2 = np.exp(-1.0 + 1250.0), np.exp(-2.0 + 5000.0)
        assert np.isnan(15.0 * (m1 + m2) + 225.0 * (m2 - m1 * m1)) and T.negbinomial_moments(15.0, -1.0, 2500.0) == (np.inf, np.inf)


@pytest.mark.parametrize("variant", T.VARIANTS)
def test_wrong_variants_leave_the_bars(reference, variant):
    kinds = {"parent_studentt": ("studentt",), "centre_half": ("studentt",), "erfc_only": ("laplace",),
             "sigma_neg": ("bernoulli", "poisson")}.get(variant, ("bernoulli", "negbinomial", "poisson", "heterogauss"))
    worst, red = (0.0, ""), 0
    T.VARIANT = variant
    try:
        for kind in kinds:
            for name, p, y, mu, var in D.points(kind):
                f = max(_bars(kind, p, y, mu, var, reference[kind, name][:3]).values())
                f = np.inf if np.isnan(f) else f
                red += f > 1.0
                worst = max(worst, (f, f"{kind} {name}"))
    finally:
        T.VARIANT = None
    print(f"{variant}: {red} points leave their bars, the worst by a factor {worst[0]:.3g} at {worst[1]}")
    assert worst[0] > 10.0
