"""agpl_predictive on the device over its whole supported domain (tests/predictive_domain.py): every grid point
against the float64 reference of tests/predictive_domain_reference.py at the project's bars (log p 1e-4 absolute; mean and variance
1e-5 relative + 1e-9 absolute; the class -- finite, +inf, NaN -- of every moment equal), and against the numpy twin of the kernel's
arithmetic (tools/predictive_twin.py) at a bar derived from the roundings: nothing is excluded, one launch per parameter set.

Device against twin, per kind, derived from the roundings (both run the same rule in float64 without contraction):
  log p: 64 eps M, M = the sum of the magnitudes of the terms log p is added up from, as the twin reports them (|h(m)|, |log sum|,
    |log spacing|, |log s|, log sqrt 2 pi; Laplace: d^2 / 2 var, var / 2 beta^2, |d| / beta, the larger term, |log 4 beta|; Student-t:
    |g(m)|, |log sum|, |log h|, lgamma(a)) plus the lgamma terms of the count's constant and y log lambda: one ulp for each exp / log /
    lgamma / erfcx behind a term, 64 for their number and for a library that is two ulps off.  No floor for the logistic,
    heteroscedastic and Laplace kinds: where device and twin stop the Newton iteration one step apart the centre moves by 1e-3 widths,
    which the rule sees at exp(-2 pi pi / 0.5) = 7e-18 and exp(-2 pi^2 w^2 / (w / 2)^2) = exp(-79) only.  Student-t alone has a floor,
    1e-8: a centre moved by a different Newton stop changes the rule by its aliasing error, exp(-pi^2 / h) = 3e-9 at h = 1/2.
    Above a tenth of the reference bar only where M > 7e8: the counts of 2^31 - 1, whose lgamma terms are 4.4e10 each.
  moments: E sigma, E sigma^2 are sums of n = 2 nh + 1 positive terms added in a different order by device and numpy, (n - 1) eps
    relative each for numerator and denominator, plus the ulps of exp and sigma: (2 n + 8) eps of E y for the mean; for the variance the
    same factor times the magnitudes behind it (Bernoulli: E sigma; Poisson: lambda E sigma + lambda^2 (E sigma^2 + 2 (E sigma)^2)).
    Closed forms: 4 eps (|x| + 4) times the magnitudes, x the argument of the exponential in them (NegBinomial 2 mu + 2 var,
    heteroscedastic -mu_g + var_g / 2, none for Student-t and Laplace).
DESIGN.md 4.23 records the bars and what was measured."""
import os
import sys

import numpy as np
import pytest

import predictive_domain as D
import predictive_domain_reference as Q

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import predictive_twin as T  # noqa: E402

pytestmark = pytest.mark.gpu
EPS = np.finfo(np.float64).eps


@pytest.fixture(scope="module")
def A():
    import agpl_amd

    return agpl_amd


@pytest.fixture(scope="module")
def ctx(A):
    return A.Context(seed=1234)


def _lik(A, kind, p):
    return {"bernoulli": lambda: A.BernoulliLikelihood(), "negbinomial": lambda: A.NegativeBinomialLikelihood(p[0]),
            "studentt": lambda: A.StudentTLikelihood(p[0], p[1]), "poisson": lambda: A.PoissonLikelihood(p[0]),
            "laplace": lambda: A.LaplaceLikelihood(p[0]), "heterogauss": lambda: A.HeteroscedasticGaussianLikelihood(p[0])}[kind]()


def _dev(a):
    import torch

    return torch.as_tensor(np.ascontiguousarray(a)).cuda()


def _cls(x):
    return np.where(np.isnan(x), 2, np.where(np.isinf(x), np.sign(x), 0))


def _logp_bar(kind, p, y):
    """After T.twin(...) of the point: the bar of |device - twin| in log p."""
    from scipy import special

    m = T.MAG
    if kind == "negbinomial":
        m += abs(special.gammaln(y + p[0])) + abs(special.gammaln(y + 1.0)) + abs(special.gammaln(p[0]))
    if kind == "poisson":
        m += abs(y * np.log(p[0])) + abs(special.gammaln(y + 1.0))
    if kind == "studentt":
        m += abs(special.gammaln(0.5 * (p[0] + 1.0))) + abs(special.gammaln(0.5 * p[0])) + abs(np.log(p[1]))  # (var = 0: the density itself)
    return 64 * EPS * max(m, 1.0) + (1e-8 if kind == "studentt" else 0.0)


def _moment_bars(kind, p, mu, var, me_t, va_t):
    """The bars of |device - twin| in (E y, Var y)."""
    if kind in ("bernoulli", "poisson"):
        n = 2 * int(min(max(32.0, np.ceil(T.SPAN * np.sqrt(var) / T.POLE_CAP)), T.MAXHALF)) + 1
        k = (2 * n + 8) * EPS
        if kind == "bernoulli":
            return k * me_t, k * me_t
        lam = p[0]
        e1 = me_t / lam
        e2 = (va_t - me_t) / (lam * lam) + e1 * e1
        return k * me_t, k * (lam * e1 + lam * lam * (abs(e2) + 2.0 * e1 * e1))
    x = {"negbinomial": lambda: abs(2.0 * mu + 2.0 * var), "heterogauss": lambda: abs(-mu[1] + 0.5 * var[1])}.get(kind, lambda: 0.0)()
    k = 4 * EPS * (x + 4.0)
    if kind == "negbinomial":
        with np.errstate(over="ignore"):
            m1, m2 = np.exp(mu + 0.5 * var), np.exp(2.0 * mu + 2.0 * var)
            return k * abs(me_t), k * (p[0] * (m1 + m2) + p[0] * p[0] * (m2 + m1 * m1))
    return k * abs(me_t if np.isfinite(me_t) else 0.0), k * abs(va_t if np.isfinite(va_t) else 0.0)


@pytest.mark.parametrize("kind", Q.R.KINDS)
def test_whole_domain(A, ctx, kind):
    ydt = {"bernoulli": np.uint8, "negbinomial": np.int32, "poisson": np.int32}.get(kind, np.float64)
    worst = {k: (0.0, "") for k in ("logp", "mean", "var", "twin", "twin_abs", "mean_twin", "var_twin")}
    bad, n = [], 0
    for p, pts in D.groups(kind):
        y = np.array([pt[2] for pt in pts], dtype=ydt)
        mu = np.array([pt[3] for pt in pts], dtype=np.float64)
        var = np.array([pt[4] for pt in pts], dtype=np.float64)
        out = A.predictive(_lik(A, kind, p), (_dev(mu), _dev(var)), _dev(y), ctx=ctx)
        mean, v, lp = (o.cpu().numpy() for o in out)
        for i, (name, _, yi, mi, vi) in enumerate(pts):
            n += 1
            lp_r, err = Q.ref_logp(kind, p, yi, mi, vi)
            me_r, va_r = Q.ref_moments(kind, p, mi, vi)
            me_t, va_t, lp_t = T.twin(kind, p, yi, mi, vi)
            assert err <= 1e-9, (name, err)  # (the CPU module proves this; a point that fails it is removed there by name)
            figs = dict(logp=abs(lp[i] - lp_r) / 1e-4, twin=abs(lp[i] - lp_t) / _logp_bar(kind, p, float(yi)), twin_abs=abs(lp[i] - lp_t))
            mbars = _moment_bars(kind, p, mi, vi, me_t, va_t)
            for key, got, ref, tw, tb in (("mean", mean[i], me_r, me_t, mbars[0]), ("var", v[i], va_r, va_t, mbars[1])):
                if _cls(got) != _cls(ref) or _cls(got) != _cls(tw):
                    bad.append((name, key, "class", got, ref, tw))
                elif np.isfinite(ref):
                    figs[key] = abs(got - ref) / (1e-5 * abs(ref) + 1e-9)
                    figs[key + "_twin"] = abs(got - tw) / tb if tb > 0.0 else (0.0 if got == tw else np.inf)
            for key, f in figs.items():
                if not f <= worst[key][0]:
                    worst[key] = (float(f), name)
                if key != "twin_abs" and not f <= 1.0:
                    bad.append((name, key, float(f)))
    print(f"{kind}: {n} points, worst in units of the bar: " + ", ".join(f"{k} {f:.3e} at {w}" for k, (f, w) in worst.items()))
    assert n == len(D.points(kind)) >= 40
    assert not bad, bad
