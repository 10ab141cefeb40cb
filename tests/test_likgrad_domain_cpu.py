"""CPU proof of the domain tests of agpl_expected_loglik: the float64 reference of
tests/likgrad_domain_reference.py against its second evaluation in mpmath on every point of tests/likgrad_domain.py; the numpy twin
of the kernel's rules (tools/likgrad_twin.py) over the whole grid at the bar of the GPU module; the twin's constants against the
.hip source; the rows the parent commit's rule fails; named wrong variants; and the evaluation counts.  No GPU."""
import math
import os
import re
import sys
import warnings

import numpy as np
import pytest

import likgrad_domain as D
import likgrad_domain_reference as Q
import likgrad_reference as R
import predictive_domain as PD

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import likgrad_twin as T  # noqa: E402

HIP = os.path.join(ROOT, "augmentedgplikelihoods.jl_amd", "csrc", "agpl_likgrad.hip")
PARENT_NODES = 2 * 2048 + 1


def _cls(x):
    return "nan" if math.isnan(x) else ("+inf" if x == math.inf else ("-inf" if x == -math.inf else "finite"))


def _factors(kind, p, y, mu, var, ref):
    """The twin's outputs in units of the reference bar (inf where the class differs)."""
    ell, dell, _ = T.twin(kind, p, y, mu, var)
    out = []
    for got, want, bar in zip([ell] + list(dell), ref.values, Q.bars(ref)):
        if _cls(got) != _cls(want):
            out.append(math.inf)
        else:
            out.append(abs(got - want) / bar if math.isfinite(want) else 0.0)
    return out


@pytest.fixture(scope="module")
def reference():
    """Ref of every grid point, computed once."""
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")  # (quad reports round-off where it has reached it; the error estimate is asserted below)
        return {(kind, pt[0]): Q.reference(kind, *pt[1:]) for kind in D.KINDS for pt in D.points(kind)}


def test_constants_are_the_kernels():
    src = open(HIP).read()
    want = {"kMaxHalf": T.MAXHALF, "kSpan": T.SPAN, "kSinhStep": T.SINH_STEP, "kSinhDensity": T.SINH_DENSITY, "kSinhPad": T.SINH_PAD,
            "kSinhMax": T.SINH_MAX, "kLn2": T.LN2}
    for name, value in want.items():
        m = re.search(r"^constexpr\s+(?:int|double)\s+" + name + r"\s*=\s*([-+.\deE]+);", src, flags=re.M)
        assert m, f"{name} is not stated in agpl_likgrad.hip"
        assert float(m.group(1)) == float(value), (name, m.group(1), value)
    assert T.SINH_STEP == math.pi / 16.0 and T.LN2 == math.log(2.0)


def test_the_grid():
    for kind in D.KINDS:
        names = [pt[0] for pt in D.GRID[kind]]
        assert len(set(names)) == len(names), kind
        assert set(PD.GRID[kind]) <= set(D.GRID[kind])  # every point of the predictive domain, GRID and not points()
        assert set(D.REMOVED[kind]) <= set(names) and len(D.REMOVED[kind]) <= 0.02 * len(names)
        edges = sorted(v for pt in D.GRID[kind] if pt[0].startswith("edge_") for v in np.ravel(pt[4]))
        assert {0.0, 1e-320, 1e-30} <= set(edges), kind
    st = {pt[0]: pt for pt in D.GRID["studentt"]}
    for nu in (0.01, 1.0, 100.0):
        for s in (0.05, 2.0, 20.0):
            for k in (0, 1, 3, 50):
                assert any(n.startswith(f"wide_nu{nu:g}_sg0.001_k{k}_") and n.endswith(f"_s{s:g}") for n in st), (nu, s, k)
    for nu in (0.01, 0.1):
        for k in (0, 1, 3, 50):
            assert f"wide_nu{nu:g}_sg0.5_k{k}_mu0_s50" in st
    for ratio in (63.9, 64.0, 64.1):
        for k in (0, 1):
            _, p, _, _, var = st[f"seam{ratio:g}_k{k}"]
            assert p == (3.0, 0.05) and math.sqrt(var) / (p[1] * math.sqrt(p[0])) == pytest.approx(ratio, rel=1e-14)
    # the Poisson point whose derivative is a difference of two numbers of 5e5: y within 1 of lambda E sigma, from the reference
    (_, p, y, mu, var), = [pt for pt in D.GRID["poisson"] if pt[0] == "lam1e+06_ynear_mu1_s0.05"]
    esig = Q.logistic_expectations(mu, var)[0][2]
    assert esig == pytest.approx(D.E_SIGMA_MU1_S005, abs=1e-13) and p == (1e6,) and abs(y - p[0] * esig) <= 1.0 and y > 5e5


@pytest.mark.parametrize("kind", D.KINDS)
def test_reference_against_mpmath(reference, kind):
    worst, werr = (0.0, ""), (0.0, "")
    for name, p, y, mu, var in D.points(kind):
        ref = reference[kind, name]
        second = Q.mp_reference(kind, p, y, mu, var)
        for v, m, bar, er in zip(ref.values, second, Q.agree_bars(ref), ref.err):
            worst = max(worst, (abs(v - m) / bar, name))
            werr = max(werr, (er / max(1.0, abs(v)), name))
    print(f"{kind}: {len(D.points(kind))} points, worst |quad - mpmath| in units of 1e-10 max(1, |value|) + 16 eps T_c {worst[0]:.2e} at {worst[1]}, "
          f"quad's error estimate {werr[0]:.2e} of max(1, |value|) at {werr[1]}")
    assert worst[0] <= 1.0 and werr[0] <= 1e-9


def test_reference_against_the_box_reference_and_closed_forms(reference):
    # inside the old box the new reference and tests/likgrad_reference.py (which integrates log p itself) give the same numbers
    for kind in D.KINDS:
        p, y, mu, var = R.cases(kind, 11)[0]
        for i in range(0, len(y), 16):
            ref = Q.reference(kind, p, y[i], mu[i], var[i])
            old = [R.ref_ell(kind, p, y[i], mu[i], var[i])[0], *R.ref_dell(kind, p, y[i], mu[i], var[i])[0]]
            for v, o in zip(ref.values, old):
                assert abs(v - o) <= 1e-11 * max(1.0, abs(o)), (kind, i, v, o)
    # var <= 1e-30 is the value at mu; var = 1e-16 differs from it by var |f''| / 2 at most
    for kind in ("bernoulli", "negbinomial", "poisson"):
        for name, p, y, mu, var in D.points(kind):
            if var == 1e-16:
                at_mu = Q.reference(kind, p, y, mu, 0.0)
                scale = float(y) + p[0] + 1.0  # |d2 log p / df2| <= (y + r) / 4, (y + lambda) / 4
                for v, o in zip(reference[kind, name].values, at_mu.values):
                    assert abs(v - o) <= var * scale + 1e-13 * max(1.0, abs(o)), (kind, name)


@pytest.mark.parametrize("kind", D.KINDS)
def test_twin_over_grid(reference, kind):
    worst, bad, most = (0.0, "", 0), [], 0
    for name, p, y, mu, var in D.points(kind):
        for k, f in enumerate(_factors(kind, p, y, mu, var, reference[kind, name])):
            worst = max(worst, (f, name, k))
            if not f <= 1.0:
                bad.append((name, k, f))
        most = max(most, T.EVALS)
        assert T.EVALS <= PARENT_NODES, (kind, name, T.EVALS)
    print(f"{kind}: twin over {len(D.points(kind))} points, worst {worst[0]:.2e} of the bar at {worst[1]} (output {worst[2]}), at most {most} nodes a point")
    assert not bad, bad


# The rows at which the rule before the sinh branch was found wrong: nu, sigma, mu, s, the residual in predictive
# standard deviations, and the errors first measured for ell and for the sigma-derivative in units of max(1, |value|), each at the
# lower end of its rounding, with the factor that cell is held to.  Two cells were recorded in other units and are held to what
# they are in these: the first row's sigma-derivative (0.10 is the absolute error of a derivative of 99.6: 1.0e-3), and the fourth
# row's ell (5.6e-5 of the quadrature term 6.3 alone; |ell| with its constant is 8.6: 4.1e-5, hence 0.7).  The other eight are
# held in full.
TABLED_ROWS = [(100.0, 1e-3, 10.0, 20.0, 0, 1.25e-4, 1.0, 0.95e-3), (0.01, 1e-3, 10.0, 20.0, 0, 6.45e-4, 1.0, 1.55e-3),
               (0.01, 1e-3, 0.0, 0.05, 0, 1.05e-5, 1.0, 2.05e-4), (0.01, 0.5, 0.0, 50.0, 0, 5.55e-5, 0.7, 6.25e-4),
               (0.01, 0.5, 0.0, 50.0, 3, 3.55e-7, 1.0, 6.65e-6)]


def test_the_parents_rule_fails_the_tabled_rows():
    """The first term of the bar is 1e-6 max(1, |value|), so a recorded error e means a factor of e / 1e-6 (less what the other two
    terms add to the bar: below 1e-3 of it at these rows).  The last row's ell (3.6e-7) stays inside; its sigma-derivative leaves."""
    for nu, sg, mu, s, k, e_ell, ell_units, e_dsg in TABLED_ROWS:
        _, p, y, mu, var = D.st_point("", nu, sg, k, mu, s)
        ref = Q.reference("studentt", p, y, mu, var)
        assert max(_factors("studentt", p, y, mu, var, ref)) <= 1.0, (p, mu, var)
        T.VARIANT = "parent_wide"
        try:
            f = _factors("studentt", p, y, mu, var, ref)
        finally:
            T.VARIANT = None
        assert T.EVALS == PARENT_NODES
        print(f"parent's rule at nu {nu:g} sigma {sg:g} mu {mu:g} s {s:g} k {k}: ell {f[0]:.3g}, d/dlog nu {f[1]:.3g}, d/dlog sigma {f[2]:.3g} bars")
        assert f[2] >= 0.999 * e_dsg / 1e-6 and f[2] > 1.0, (nu, sg, f)
        assert f[0] >= 0.999 * ell_units * e_ell / 1e-6, (nu, sg, f)


def test_the_sinh_rule_to_rounding():
    """The header's promise for the rule above the seam: the two expectations within 1e-12 max(1, |value|) of the 30-digit integral
    at every wide and seam point that takes the sinh rule (what the 1e-6 bar cannot see: a spacing slightly too coarse).  The other
    wide and seam points (s / a <= 64, or y outside mu +- 8 s) are held to four times the trapezoid rule's design error e^{-8 pi},
    so the two rules join at the seam without a step above that."""
    n, worst, other = 0, (0.0, ""), (0.0, "")
    for name, p, y, mu, var in D.points("studentt"):
        if name.startswith(("wide_", "seam")):
            s, a = math.sqrt(var), p[1] * math.sqrt(p[0])
            got = T.studentt_expectations(p[0], p[1], y, mu, var)
            want = Q.mp_studentt_expectations(p[0], p[1], y, mu, var)[0]
            err = max(abs(g - w) / max(1.0, abs(w)) for g, w in zip(got, want))
            if T.make_rule(s, a)[2] and abs(y - mu) < T.SPAN * s:
                worst, n = max(worst, (err, name)), n + 1
            else:
                other = max(other, (err, name))
    print(f"{n} sinh-rule points: worst |twin - mpmath| / max(1, |value|) of an expectation {worst[0]:.2e} at {worst[1]}; "
          f"the other wide and seam points {other[0]:.2e} at {other[1]}")
    assert n == 29 and worst[0] <= 1e-12 and other[0] <= 4.0 * Q.DESIGN_ERROR


WRONG = {"parent_wide": ("studentt",), "centre_half": ("bernoulli", "negbinomial", "studentt", "poisson", "heterogauss"), "nb_swap": ("negbinomial",),
         "no_half_over_nu": ("studentt",), "nu_for_nu_plus_1": ("studentt",), "spacing_half": ("bernoulli", "negbinomial", "studentt", "poisson", "heterogauss"),
         "no_lambda": ("poisson",)}


@pytest.mark.parametrize("variant", T.VARIANTS)
def test_wrong_variants_leave_the_bars(reference, variant):
    worst, red, n = (0.0, ""), 0, 0
    T.VARIANT = variant
    try:
        for kind in WRONG[variant]:
            for name, p, y, mu, var in D.points(kind):
                f = max(_factors(kind, p, y, mu, var, reference[kind, name]))
                f = math.inf if math.isnan(f) else f
                red, n = red + (f > 1.0), n + 1
                worst = max(worst, (f, f"{kind} {name}"))
    finally:
        T.VARIANT = None
    print(f"{variant}: {red} of {n} points leave their bars, the worst by a factor {worst[0]:.3g} at {worst[1]}")
    assert red >= 1 and worst[0] > 1.0


def test_evaluation_counts_are_bounded():
    """Inside the old box the rule is the parent's (s / a <= 50 < 64), so the count per point must not be above the parent's; the
    grid's bound of 2 * 2048 + 1 is asserted point by point in test_twin_over_grid."""
    for kind in D.KINDS:
        most = 0
        for p, y, mu, var in R.cases(kind, R.SEED + R.KINDS.index(kind)):
            for i in range(len(y)):
                T.twin(kind, p, y[i], mu[i], var[i])
                now = T.EVALS
                T.VARIANT = "parent_wide"
                try:
                    T.twin(kind, p, y[i], mu[i], var[i])
                finally:
                    T.VARIANT = None
                assert now <= T.EVALS <= PARENT_NODES, (kind, p, i, now, T.EVALS)
                most = max(most, now)
        print(f"{kind}: at most {most} nodes a point inside the old box")
