"""Float64 references of the expected log-likelihood E_{q(f)} log p(y | f; theta) and of its derivatives for the logarithms of the
likelihood's parameters, for tests/test_gpu_likgrad.py: `loglik` of tests/predictive_reference.py for the value, hand-written
analytic derivatives of log p for the gradient, both integrated against q(f) = N(mu, s^2) with scipy.integrate.quad (epsrel 1e-13,
split at mu and at y), and the random cases of the test box.  No GPU, no library code: nothing here imports the package."""
import functools
import math

import numpy as np
from scipy import integrate, special

from predictive_reference import loglik

KINDS = ("bernoulli", "negbinomial", "studentt", "poisson", "laplace", "heterogauss")
NPARAMS = {"bernoulli": 0, "negbinomial": 1, "studentt": 2, "poisson": 1, "laplace": 1, "heterogauss": 1}
WIDTH = 14.0  # the integrals run over mu +- WIDTH s: the weight beyond is exp(-98)
NCASES = 512  # per kind
NGROUPS = 8   # parameter settings per kind (one device call each)


def _expit(x):
    return 1.0 / (1.0 + math.exp(-x)) if x >= 0.0 else math.exp(x) / (1.0 + math.exp(x))


def _logsig(x):
    return -math.log1p(math.exp(-x)) if x >= 0.0 else x - math.log1p(math.exp(x))


def dloglik(kind, p, y, f, g=None):
    """d log p(y | f) / d log theta_p, p = 0 .. P - 1 (a tuple), in the order of the descriptor's parameters."""
    if kind == "negbinomial":
        r = p[0]
        return (r * (special.digamma(y + r) - special.digamma(r) + _logsig(-f)),)
    if kind == "studentt":
        nu, sg = p[0], p[1]
        z2 = ((y - f) / sg) ** 2
        dnu = nu * (0.5 * special.digamma(0.5 * (nu + 1.0)) - 0.5 * special.digamma(0.5 * nu) - 0.5 / nu
                    - 0.5 * math.log1p(z2 / nu) + 0.5 * (nu + 1.0) * z2 / (nu * (nu + z2)))
        return (dnu, -1.0 + (nu + 1.0) * z2 / (nu + z2))
    if kind == "poisson":
        return (y - p[0] * _expit(f),)
    if kind == "laplace":
        return (-1.0 + abs(y - f) / p[0],)
    if kind == "heterogauss":
        return (0.5 - 0.5 * p[0] * _expit(g) * (y - f) ** 2,)
    raise ValueError(kind)


def gauss_expect(fun, mu, var, split=()):
    """(E fun(f), quad's absolute error estimate) under N(mu, var); var = 0 gives fun(mu)."""
    if var == 0.0:
        return float(fun(mu)), 0.0
    s = math.sqrt(var)
    a, b = mu - WIDTH * s, mu + WIDTH * s
    c = 1.0 / (s * math.sqrt(2.0 * math.pi))
    g = lambda f: fun(f) * math.exp(-0.5 * ((f - mu) / s) ** 2) * c
    edges = [a] + sorted({mu, *[e for e in split if a < e < b]}) + [b]
    tot = err = 0.0
    for lo, hi in zip(edges[:-1], edges[1:]):
        v, e = integrate.quad(g, lo, hi, epsabs=0.0, epsrel=1e-13, limit=400)
        tot += v
        err += e
    return tot, err


def _point(kind, mu, var):
    """(the latent quad integrates over: its mean and variance; for the heteroscedastic kind the f-latent's too)."""
    if kind == "heterogauss":
        return float(mu[1]), float(var[1]), float(mu[0]), float(var[0])
    return float(mu), float(var), None, None


def _integrand(kind, p, y, mf, vf, fun):
    """fun(f) or, heteroscedastic, g -> E_f fun(f, g): log p and its derivative are quadratic in f, for which the two-point rule
    (fun(mu_f + s_f) + fun(mu_f - s_f)) / 2 is exact."""
    if kind != "heterogauss":
        return lambda f: fun(f, None)
    sf = math.sqrt(vf)
    return lambda g: 0.5 * (fun(mf + sf, g) + fun(mf - sf, g))


def ref_ell(kind, p, y, mu, var):
    """(E_q log p(y | f), quad's absolute error estimate) of one point; mu, var scalars (heteroscedastic: pairs (f, g))."""
    m, v, mf, vf = _point(kind, mu, var)
    y = float(y)
    fun = _integrand(kind, p, y, mf, vf, lambda f, g: float(loglik(kind, p, y, f, g)))
    return gauss_expect(fun, m, v, split=(y,) if kind in ("studentt", "laplace") else ())


def ref_dell(kind, p, y, mu, var):
    """(d ell / d log theta [P], quad's absolute error estimates [P]) of one point."""
    m, v, mf, vf = _point(kind, mu, var)
    y = float(y)
    P = NPARAMS[kind]
    out, err = np.empty(P), np.empty(P)
    for k in range(P):
        fun = _integrand(kind, p, y, mf, vf, lambda f, g, k=k: dloglik(kind, p, y, f, g)[k])
        out[k], err[k] = gauss_expect(fun, m, v, split=(y,) if kind in ("studentt", "laplace") else ())
    return out, err


def laplace_closed(beta, y, mu, var):
    """E|y - f| under N(mu, var): s sqrt(2 / pi) exp(-d^2 / 2 s^2) + d erf(d / (s sqrt 2)), d = y - mu."""
    d, s = y - mu, math.sqrt(var)
    return s * math.sqrt(2.0 / math.pi) * math.exp(-0.5 * d * d / var) + d * math.erf(d / (s * math.sqrt(2.0)))


def ref_sums(kind, p, y, mu, var):
    """(sum_i ell_i, sum_i dell_i [P], error estimate) over MANY points of one latent at once, for marginals of a fit (thousands of
    points, var > 0, features no narrower than s): scipy.integrate.quad_vec (the same adaptive Gauss-Kronrod rule, epsrel 1e-13) on
    the vector of all points' integrands in t = (f - mu) / s over +- WIDTH, split at t = 0.  Laplace, whose kink sits at another t
    in every point, takes the closed form instead.  tests/test_likgrad_reference_cpu.py holds this to the per-point functions."""
    y, mu, var = np.asarray(y, dtype=np.float64), np.asarray(mu, dtype=np.float64), np.asarray(var, dtype=np.float64)
    if kind == "laplace":
        d, s = y - mu, np.sqrt(var)
        ea = (s * np.sqrt(2.0 / np.pi) * np.exp(-0.5 * d * d / var) + d * special.erf(d / (s * np.sqrt(2.0)))) / p[0]
        return float(np.sum(-ea - np.log(2.0 * p[0]))), np.array([np.sum(-1.0 + ea)]), 0.0
    if kind == "heterogauss":
        raise ValueError("ref_sums covers the one-latent kinds")
    s, P = np.sqrt(var), NPARAMS[kind]

    def dvec(f):  # dloglik, vectorised over the points
        if kind == "negbinomial":
            return [p[0] * (special.digamma(y + p[0]) - special.digamma(p[0]) - np.logaddexp(0.0, f))]
        if kind == "poisson":
            return [y - p[0] * special.expit(f)]
        if kind == "studentt":
            nu, z2 = p[0], ((y - f) / p[1]) ** 2
            return [nu * (0.5 * special.digamma(0.5 * (nu + 1.0)) - 0.5 * special.digamma(0.5 * nu) - 0.5 / nu
                          - 0.5 * np.log1p(z2 / nu) + 0.5 * (nu + 1.0) * z2 / (nu * (nu + z2))), -1.0 + (nu + 1.0) * z2 / (nu + z2)]
        return []

    def integrand(t):
        f = mu + s * t
        w = math.exp(-0.5 * t * t) / math.sqrt(2.0 * math.pi)
        return w * np.array([np.sum(loglik(kind, p, y, f))] + [np.sum(d) for d in dvec(f)])

    tot, err = np.zeros(1 + P), 0.0
    for lo, hi in ((-WIDTH, 0.0), (0.0, WIDTH)):
        v, e = integrate.quad_vec(integrand, lo, hi, epsabs=0.0, epsrel=1e-13, norm="max", limit=2000)
        tot += v
        err += e
    return float(tot[0]), tot[1:], err


def _loguniform(rng, lo, hi, size=None):
    return np.exp(rng.uniform(np.log(lo), np.log(hi), size=size))


def cases(kind, seed):
    """The random case box: a list of NGROUPS groups (p, y [m], mu, var) that together hold NCASES points.  mu uniform in +-8,
    s log-uniform in [1e-3, 6] (Student-t: at most 50 sigma sqrt(nu)), counts 0 .. 200, nu in [0.6, 50], sigma and beta in
    [0.05, 5], r in [0.3, 40], lambda in [0.2, 20], all log-uniform; real y within about three predictive standard deviations."""
    rng = np.random.default_rng(seed)
    m = NCASES // NGROUPS
    out = []
    for _ in range(NGROUPS):
        if kind == "bernoulli":
            p = (0.0,)
        elif kind == "negbinomial":
            p = (float(_loguniform(rng, 0.3, 40.0)),)
        elif kind == "studentt":
            p = (float(_loguniform(rng, 0.6, 50.0)), float(_loguniform(rng, 0.05, 5.0)))
        elif kind == "laplace":
            p = (float(_loguniform(rng, 0.05, 5.0)),)
        else:
            p = (float(_loguniform(rng, 0.2, 20.0)),)
        L = 2 if kind == "heterogauss" else 1
        smax = min(6.0, 50.0 * p[1] * math.sqrt(p[0])) if kind == "studentt" else 6.0
        mu = rng.uniform(-8.0, 8.0, size=(m, L))
        s = _loguniform(rng, 1e-3, smax, size=(m, L))
        var = s * s
        if kind == "bernoulli":
            y = rng.integers(0, 2, size=m).astype(np.uint8)
        elif kind in ("negbinomial", "poisson"):
            y = rng.integers(0, 201, size=m).astype(np.int32)
        elif kind == "studentt":
            y = mu[:, 0] + 3.0 * rng.standard_normal(m) * np.sqrt(var[:, 0] + p[1] ** 2)
        elif kind == "laplace":
            y = mu[:, 0] + 3.0 * rng.standard_normal(m) * np.sqrt(var[:, 0] + 2.0 * p[0] ** 2)
        else:
            y = mu[:, 0] + 3.0 * rng.standard_normal(m) * np.sqrt(var[:, 0] + (1.0 + np.exp(-mu[:, 1])) / p[0])
        if L == 1:
            mu, var = mu[:, 0], var[:, 0]
        out.append((p, y, mu, var))
    return out


def reference(kind, p, y, mu, var):
    """(ell [n], dell [n, P], ell_err [n], dell_err [n, P]) for one group."""
    n, P = len(y), NPARAMS[kind]
    ell, eerr, dell, derr = np.empty(n), np.empty(n), np.empty((n, P)), np.empty((n, P))
    for i in range(n):
        ell[i], eerr[i] = ref_ell(kind, p, y[i], mu[i], var[i])
        dell[i], derr[i] = ref_dell(kind, p, y[i], mu[i], var[i])
    return ell, dell, eerr, derr


SEED = 20261019


@functools.lru_cache(maxsize=None)
def box(kind):
    """The case box of `kind` with its reference, computed once per process: a list of (p, y, mu, var, ell, dell, ell_err, dell_err)."""
    return [grp + reference(kind, *grp) for grp in cases(kind, SEED + KINDS.index(kind))]
