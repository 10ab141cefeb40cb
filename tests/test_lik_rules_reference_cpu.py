"""tests/lik_rules_reference.py held against the project's oracle, against itself and against the sources, without a GPU.

  * the mpmath reference agrees with the float64 oracle to 1e-13 relative, point by point, on the typical draw of
    test_gpu_parity.py::test_aux_posterior_and_expectations (the first 300 of its 2500 points, every likelihood of that test; the ELBO terms as the sums the oracle states);
  * the numpy model of every rule stays inside the derived bars at every grid point, or is in the expected non-finite class;
  * every named wrong variant leaves the bars (or the class) at one or more points, the named one among them;
  * the logistic cut-offs and the c == T(0) branch are read from agpl_random.h.

Measured here.  Worst |model - mpmath| / bar: operators float32 <= 1.0 (exactly 1 where 1 / coshf overflows to a 0 whose true value
is below the smallest normal number: the bar there is that value), otherwise <= 0.84; float64 <= 0.96 (few-rounding outputs such as
beta = 2 m y: a correctly rounded model may use all of one rounding); ELBO terms <= 0.36; elbo_point <= 0.18.  Smallest ratio by which
a variant leaves a bar, at its named point (smallest over all points in brackets): tanh_from_exp 906 (906; float32, gamma at
c = 1e-4), cutoffs_of_other_type 2.5e5 (20), sech_from_exp 1.1e5 (1.1e5; float32, c = 178, the only point between the overflow of
expf and that of coshf), studentt_quirk_fixed 2.1e7 (44), pg_kl_terms_swapped 1.2e15 (1.3e13), elbo_shortcut_c_for_half_c 5.9e14 (5.8e6);
no_c0_branch, p0_reversed and zero_log_zero_is_zero change the class (NaN for 1/4; a finite gamma where the rule's order of summation
gives p0 = 0 and +inf; a finite KL where the rule gives NaN)."""
import numpy as np
import pytest

import lik_rules_reference as R

NAMES = {"bernoulli": ("bernoulli", {}), "negbin": ("negbin", {"r": 15.0}), "negbin_real": ("negbin", {"r": 5.5}),
         "studentt": ("studentt", {"nu": 3.5, "sigma": 2.0}), "poisson": ("poisson", {"lam": 10.0}), "laplace": ("laplace", {"beta": 1.3}),
         "cat": ("cat", {"logtheta": [0.1, -0.2, 0.3, 0.0]}), "catbij": ("catbij", {"logtheta": [0.1, -0.2, 0.3, 0.0]}),
         "hetero": ("hetero", {"lam": 5.0})}


def test_the_cutoffs_and_the_zero_branch_are_the_header_s():
    c = R.header_constants()
    assert c["f32"] == (float(R.F32.lo), float(R.F32.hi)) and c["f64"] == (float(R.F64.lo), float(R.F64.hi))
    assert c["pg_mean_zero_branch"]


def _oracle_lik(O, name):
    return {"bernoulli": O.bernoulli(), "negbin": O.negbinomial(15.0), "negbin_real": O.negbinomial(5.5), "studentt": O.studentt(3.5, 2.0),
            "poisson": O.poisson(10.0), "laplace": O.laplace(1.3), "cat": O.categorical([0.1, -0.2, 0.3, 0.0]),
            "catbij": O.categorical([0.1, -0.2, 0.3, 0.0], bijective=True), "hetero": O.heterogauss(5.0)}[name]


def _typical_draw(O, olik, n=2500):
    """The inputs of test_aux_posterior_and_expectations (same generator, same order of draws)."""
    rng = np.random.default_rng(6)
    L = olik.nlatent
    mu = rng.normal(size=(n, L)) * 1.5
    var = rng.uniform(0.05, 2.0, size=(n, L))
    if olik.kind == O.BERNOULLI:
        y = (rng.uniform(size=n) < 0.5).astype(np.uint8)
    elif olik.kind in (O.NEGBINOMIAL, O.POISSON):
        y = rng.poisson(4.0, size=n).astype(np.int32)
    elif olik.kind in (O.CATEGORICAL, O.CATEGORICAL_BIJ):
        lab = rng.integers(0, L + (1 if olik.kind == O.CATEGORICAL_BIJ else 0), size=n)
        y = (lab[:, None] == np.arange(L)[None, :]).astype(np.uint8)
    else:
        y = rng.normal(size=n)
    return y, mu, var


@pytest.mark.parametrize("name", list(NAMES))
def test_the_reference_is_the_oracle_s_statement_of_the_rules(oracle, name):
    O = oracle
    kind, params = NAMES[name]
    olik = _oracle_lik(O, name)
    y, mu, var = _typical_draw(O, olik)
    n, L = 300, olik.nlatent
    y, mu, var = y[:n], mu[:n], var[:n]
    o1, o2, o3 = O.aux_posterior(olik, y, mu if L > 1 else mu.ravel(), var if L > 1 else var.ravel())
    gb = O.expected_potential_precision(olik, y, o1, o2, mu_g=mu[:, 1] if name == "hetero" else None)
    ref = R.Ref(kind, R.F64, params)
    worst = 0.0

    def close(got, x, what):
        nonlocal worst
        assert not x.bad, what
        rel = abs(R.mpf(float(got)) - x.v) / max(abs(x.v), R.mpf(10) ** -300)
        worst = max(worst, float(rel))
        assert rel <= 1e-13, (what, float(got), R.mp.nstr(x.v, 20))

    La = 1 if name == "hetero" else L
    sums = {"elt": R.mpf(0), "kl": R.mpf(0), "eal": R.mpf(0)}
    for i in range(n):
        yi = [float(v) for v in np.atleast_1d(y[i])]
        r1, r2, r3 = ref.aux_posterior(yi, mu[i], var[i])
        q1 = np.atleast_1d(o1.reshape(n, La)[i])
        q2 = np.atleast_1d(o2.reshape(n, La)[i]) if o2 is not None else []
        for k in range(La):
            close(q1[k], r1[k], (i, "out1", k))
            if len(r2):
                close(q2[k], r2[k], (i, "out2", k))
        if r3 is not None:
            close(o3[i], r3, (i, "out3"))
        g, b = ref.expected_pp(yi, q1, q2, mu[i, 1] if name == "hetero" else None)
        for k in range(L):
            close(gb[1][k][i], g[k], (i, "gamma", k))
            close(gb[0][k][i], b[k], (i, "beta", k))
        if name != "hetero":
            sums["elt"] += ref.expected_logtilt(yi, q1, q2, mu[i], var[i]).v
        if name not in ("cat", "hetero"):
            sums["kl"] += ref.aux_kl(yi, q1, q2).v
        if name != "cat":
            sums["eal"] += ref.expected_aug_loglik(yi, q1, q2, mu[i], var[i]).v
    # the ELBO terms: the oracle states them as sums over the points, so the sums of the per-point reference are compared
    flat = lambda a: a if L > 1 else a.ravel()
    if name != "hetero":
        close(O.expected_logtilt(olik, y, o1, o2, flat(mu), flat(var)), R.X(sums["elt"]), "sum expected_logtilt")
    if name not in ("cat", "hetero"):
        close(O.aux_kl(olik, y, o1, o2), R.X(sums["kl"]), "sum aux_kl")
    if name != "cat":
        close(O.expected_aug_loglik(olik, y, o1, o2, flat(mu), flat(var)), R.X(sums["eal"]), "sum expected_aug_loglik")
    print(f"LIK_RULES_ORACLE {name}: worst relative difference {worst:.3g}")


# the number of unresolved outputs per (likelihood, type): each is an assertion of the model's class (module docstring of the
# reference), and a grid or a rule that changes moves these figures
UNRESOLVED = {("bernoulli", "f32"): 1, ("bernoulli", "f64"): 1, ("negbin", "f32"): 2, ("negbin", "f64"): 2, ("studentt", "f32"): 18,
              ("studentt", "f64"): 0, ("cat", "f32"): 49, ("cat", "f64"): 33, ("catbij", "f32"): 17, ("catbij", "f64"): 17,
              ("poisson", "f32"): 1, ("poisson", "f64"): 1, ("laplace", "f32"): 15, ("laplace", "f64"): 12, ("hetero", "f32"): 13,
              ("hetero", "f64"): 1}


@pytest.mark.parametrize("fmt", ["f32", "f64"])
@pytest.mark.parametrize("kind", R.KINDS)
def test_the_model_stays_inside_the_bars(kind, fmt):
    recs = R.evaluate_operators(kind, R.FMT[fmt], R.ModelImpl())
    worst, fails, unres = R.summarize(recs)
    print(f"LIK_RULES_MODEL {kind} {fmt}: {len(recs)} outputs, worst ratio {worst:.3f}, unresolved {unres}")
    assert not fails, "\n".join(fails)
    assert unres == UNRESOLVED[kind, fmt]


@pytest.mark.parametrize("kind", R.KINDS)
def test_the_float64_elbo_terms_of_the_model_stay_inside_the_bars(kind):
    worst, fails, unres = R.summarize(R.evaluate_elbo(kind, R.ModelImpl()))
    print(f"LIK_RULES_MODEL {kind} elbo terms: worst ratio {worst:.3f}, unresolved {unres}")
    assert not fails, "\n".join(fails)
    if kind not in ("cat", "hetero"):
        worst, fails, unres = R.summarize(R.evaluate_elbo_point(kind))
        print(f"LIK_RULES_MODEL {kind} elbo_point: worst ratio {worst:.3f}, unresolved {unres}")
        assert not fails, "\n".join(fails)


def test_the_grid_reaches_the_classes_it_was_built_for():
    """The non-finite and zero classes the grid exists for, by name, from the model (= the expected class of an unresolved output)."""
    def out(kind, fmt, point, name):
        r = [r for r in R.evaluate_operators(kind, R.FMT[fmt], R.ModelImpl()) if r.point == point and r.out == name]
        assert len(r) == 1, (kind, point, name)
        return r[0]

    for fmt in ("f32", "f64"):
        assert R.classify(out("laplace", fmt, "mu=y,var=0,beta=1.3", "gamma[0]").got) == "+inf"
        assert R.classify(out("bernoulli", fmt, "q1=denormal", "gamma[0]").got) == "nan"  # b / (2c) overflows, tanh(c / 2) is 0
        assert out("bernoulli", fmt, "c=0", "gamma[0]").got == 0.25
        assert R.classify(out("cat", fmt, "sum q2 rounds to 1 forwards only", "gamma[2]").got) == "+inf"
        assert out("cat", fmt, "one=+800,var=2e6", "out2[0]").got == 0.0
    assert R.classify(out("cat", "f32", "all=-17", "gamma[0]").got) == "+inf" and R.classify(out("cat", "f64", "all=-17", "gamma[0]").got) == "fin"
    assert R.classify(out("cat", "f64", "all=-40", "gamma[0]").got) == "+inf"
    assert R.classify(out("cat", "f32", "all=-17", "beta[0]").got) == "-inf"
    assert R.classify(out("studentt", "f32", "res=2e+19,nu=3.5,sg=2", "out1[0]").got) == "+inf"
    assert out("studentt", "f32", "res=2e+19,nu=3.5,sg=2", "gamma[0]").got == 0.0
    assert np.isfinite(out("studentt", "f32", "res=1e+19,nu=3.5,sg=2", "out1[0]").got)
    kl = [r for r in R.evaluate_elbo("catbij", R.ModelImpl()) if r.point == "one=+800,var=2e6" and r.out == "kl"]
    assert len(kl) == 1 and R.classify(kl[0].got) == "nan" and kl[0].ref.unresolved  # 0 (log 0 - log p): the reference's own


# variant -> (evaluation, likelihood, type, the point and output at which it must leave the bar, the least ratio required there:
# a tenth of the measured figure of the module docstring, or inf for a change of class)
INF = float("inf")
VARIANT_CASES = {
    "tanh_from_exp": ("op", "bernoulli", "f32", "c=1e-4", "gamma[0]", 90.0),
    "no_c0_branch": ("op", "bernoulli", "f32", "c=0", "gamma[0]", INF),
    "cutoffs_of_other_type": ("op", "poisson", "f32", "-mu=hicut+1ulp", "out2[0]", 2.5e4),
    "sech_from_exp": ("op", "poisson", "f32", "c=178", "out2[0]", 1.1e4),
    "p0_reversed": ("op", "cat", "f32", "sum q2 rounds to 1 forwards only", "gamma[2]", INF),
    "studentt_quirk_fixed": ("op", "studentt", "f32", "var=1", "out1[0]", 2.0e6),
    "pg_kl_terms_swapped": ("elbo", "bernoulli", "f64", "c=20", "kl", 1.2e14),
    "elbo_shortcut_c_for_half_c": ("point", "bernoulli", "f64", "c=20", "elbo_point", 5.9e13),
    "zero_log_zero_is_zero": ("elbo", "catbij", "f64", "one=+800,var=2e6", "kl", INF),
}


@pytest.mark.parametrize("variant", R.VARIANTS)
def test_every_wrong_variant_leaves_the_bars(variant):
    how, kind, fmt, point, name, required = VARIANT_CASES[variant]
    if how == "op":
        recs = R.evaluate_operators(kind, R.FMT[fmt], R.ModelImpl(variant))
    elif how == "elbo":
        recs = R.evaluate_elbo(kind, R.ModelImpl(variant))
    else:
        recs = R.evaluate_elbo_point(kind, variant)
    out = []
    for r in recs:
        ok, ratio, why = R.verdict(r.got, r.ref, r.model)
        if not ok:
            out.append((r.point, r.out, ratio))
    assert out, f"{variant} stays inside every bar: the grid or the bar is too weak"
    at = [ratio for p, o, ratio in out if (p, o) == (point, name)]
    print(f"LIK_RULES_VARIANT {variant}: leaves the bar at {len(out)} outputs, smallest ratio {min(x[2] for x in out):.3g}, "
          f"at {point} / {name}: {at[0] if at else None}")
    assert at and at[0] >= required, (variant, at, out[:5])
