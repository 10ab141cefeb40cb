"""References of E_q log p(y | f; theta) and of its derivatives for the logarithms of the likelihood's parameters that can be
trusted on the whole grid of tests/likgrad_domain.py (tests/likgrad_reference.py serves the old box and keeps its results).  Every
output is assembled from the expectations the kernel also forms -- E log sigma(+-f), E sigma(f), E log1p(z^2 / nu),
E z^2 / (nu + z^2), E|y - f| under q(f) = N(mu, s^2) -- and from closed-form constants:
  - scipy.integrate.quad at epsrel 1e-13 in t = (f - mu) / s over +- 14 (so s = 1e-8 at |mu| = 40 keeps the Gaussian factor), with
    break points at mu, at y and at y +- a 4^k (a = sigma sqrt(nu) for Student-t, beta for Laplace's kink), at 0 +- 4^k for the
    logistic terms;
  - the constants (lgamma and psi terms, y log lambda) from mpmath at 40 digits, so that lgamma(y + r) - lgamma(y + 1) - lgamma(r)
    at y = 2^31 - 1 and lgamma((nu + 1) / 2) - lgamma(nu / 2) at nu = 1e6 keep their digits;
  - var <= 1e-30: the value at mu (the second-order term var f'' / 2 is below rounding);
  - two magnitudes per output: T_q, the sum of |coefficient x expectation| over the terms that go through quadrature, and T_c, the
    sum of the magnitudes of the closed-form terms.
A second evaluation in mpmath at 30 digits, independent in the quadrature of the expectations only (the assembly of the outputs from
them and the constants are shared; tests/test_likgrad_domain_cpu.py holds the assembly to tests/likgrad_reference.py, which integrates
log p itself, inside the old box): tanh-sinh on the same integrals with break points of its own (every 2 s,
and the feature +- 2^k of its width) for the logistic and Student-t terms, with E log sigma(-f) = E log sigma(f) - mu; the erf form
for Laplace; the product form for the heteroscedastic kind.  No GPU, nothing imports the package."""
import collections
import math

import mpmath as mp
import numpy as np
from scipy import integrate

WIDTH = 14.0  # the integrals run over mu +- WIDTH s: the weight beyond is exp(-98)
TINY_VAR = 1e-30
EPS = float(np.finfo(np.float64).eps)
DESIGN_ERROR = math.exp(-8.0 * math.pi)  # of the trapezoid rule at spacing a / 4: exp(-2 pi a / spacing)
NPARAMS = {"bernoulli": 0, "negbinomial": 1, "studentt": 2, "poisson": 1, "laplace": 1, "heterogauss": 1}
_INV_SQRT_2PI = 1.0 / math.sqrt(2.0 * math.pi)

Ref = collections.namedtuple("Ref", "values tq tc err")  # each a list of 1 + P numbers: ell, then the derivatives


def bars(ref):
    """The device's (and the twin's) bar against the reference, per output: what a sound rule may leave."""
    return [1e-6 * max(1.0, abs(v)) + 4.0 * DESIGN_ERROR * q + 64.0 * EPS * c for v, q, c in zip(ref.values, ref.tq, ref.tc)]


def bar_terms(ref, k):
    """The three terms of bars(ref)[k]."""
    return 1e-6 * max(1.0, abs(ref.values[k])), 4.0 * DESIGN_ERROR * ref.tq[k], 64.0 * EPS * ref.tc[k]


def agree_bars(ref):
    """The bar between the two evaluations of the reference."""
    return [1e-10 * max(1.0, abs(v)) + 16.0 * EPS * c for v, c in zip(ref.values, ref.tc)]


def _logsig(x):
    return -math.log1p(math.exp(-x)) if x >= 0.0 else x - math.log1p(math.exp(x))


def _expit(x):
    return 1.0 / (1.0 + math.exp(-x)) if x >= 0.0 else math.exp(x) / (1.0 + math.exp(x))


def _quad_t(fun, breaks):
    """(integral of fun(t) N(t; 0, 1) over +- WIDTH, quad's absolute error estimate), split at 0 and at `breaks`."""
    edges = sorted({-WIDTH, 0.0, WIDTH, *[b for b in breaks if -WIDTH < b < WIDTH]})
    tot = err = 0.0
    for lo, hi in zip(edges[:-1], edges[1:]):
        v, e = integrate.quad(lambda t: fun(t) * math.exp(-0.5 * t * t) * _INV_SQRT_2PI, lo, hi, epsabs=0.0, epsrel=1e-13, limit=400)
        tot, err = tot + v, err + e
    return tot, err


def _ladder(centre, width, s, base):
    ks = [width * base ** k for k in range(-2, 60) if width * base ** k < 2.0 * WIDTH * s + abs(centre)]
    return [(centre + sgn * k) / s for k in ks for sgn in (-1.0, 1.0)] + [centre / s]


def logistic_expectations(mu, var):
    """((E log sigma(f), E log sigma(-f), E sigma(f)), their error estimates)."""
    if var <= TINY_VAR:
        return (_logsig(mu), _logsig(-mu), _expit(mu)), (0.0, 0.0, 0.0)
    s = math.sqrt(var)
    br = _ladder(-mu, 1.0, s, 4.0)
    out = [_quad_t(lambda t, g=g: g(mu + s * t), br) for g in (_logsig, lambda f: _logsig(-f), _expit)]
    if s <= 0.25:
        # E sigma(f) = sigma(mu) + E [sigma(f) - sigma(mu) - sigma'(mu) (f - mu)]: the integrand is O(s^2), and so is quad's error.
        # Poisson's y - lambda E sigma(f) at lambda = 1e6 is a difference of two numbers of 5e5 and needs E sigma to 1e-15.
        s0 = _expit(mu)
        v, e = _quad_t(lambda t: _expit(mu + s * t) - s0 - s0 * (1.0 - s0) * s * t, br)
        out[2] = (s0 + v, e)
    return tuple(o[0] for o in out), tuple(o[1] for o in out)


def studentt_expectations(nu, sg, y, mu, var):
    """((E log1p(u), E u / (1 + u)), error estimates), u = (y - f)^2 / (nu sg^2)."""
    a, d = sg * math.sqrt(nu), y - mu
    if var <= TINY_VAR:
        u = (d / a) ** 2
        return (math.log1p(u), u / (1.0 + u)), (0.0, 0.0)
    s = math.sqrt(var)
    br = _ladder(d, a, s, 4.0)
    usq = lambda t: ((d - s * t) / a) ** 2
    out = [_quad_t(lambda t: math.log1p(usq(t)), br), _quad_t(lambda t: usq(t) / (1.0 + usq(t)), br)]
    return tuple(o[0] for o in out), tuple(o[1] for o in out)


def expected_abs(beta, y, mu, var):
    """(E|y - f|, error estimate)."""
    d = y - mu
    if var <= TINY_VAR:
        return abs(d), 0.0
    s = math.sqrt(var)
    return _quad_t(lambda t: abs(d - s * t), _ladder(d, beta, s, 4.0))


def _f(x):
    return float(x)


def _constants(kind, p, y):
    """The closed-form terms of ell and of each derivative, in mpmath: lists of signed terms per output."""
    with mp.workdps(40):
        m = lambda x: mp.mpf(float(x))
        if kind == "negbinomial":
            r, yy = m(p[0]), m(y)
            return [[mp.loggamma(yy + r), -mp.loggamma(yy + 1), -mp.loggamma(r)], [r * mp.digamma(yy + r), -r * mp.digamma(r)]]
        if kind == "poisson":
            lam, yy = m(p[0]), m(y)
            return [[yy * mp.log(lam), -mp.loggamma(yy + 1)], [yy]]
        if kind == "studentt":
            nu, sg = m(p[0]), m(p[1])
            return [[mp.loggamma((nu + 1) / 2), -mp.loggamma(nu / 2), -mp.log(nu * mp.pi) / 2, -mp.log(sg)],
                    [nu * mp.digamma((nu + 1) / 2) / 2, -nu * mp.digamma(nu / 2) / 2, -mp.mpf(1) / 2], [mp.mpf(-1)]]
        if kind == "laplace":
            return [[-mp.log(2 * m(p[0]))], [mp.mpf(-1)]]
        if kind == "heterogauss":
            return [[mp.log(m(p[0])) / 2, -mp.log(2 * mp.pi) / 2], [mp.mpf(1) / 2]]
        return [[]]


def _assemble(kind, consts, quads):
    """consts: the closed-form terms per output (mpmath); quads: per output a list of (coefficient, expectation, error estimate).
    Poisson's y, the -1 and the 1/2 of the derivatives count as closed-form terms: y - lambda E sigma is formed in float64, which
    holds lambda E sigma to eps times its size, the size of y where the two cancel."""
    values, tq, tc, err = [], [], [], []
    for k, (cs, qs) in enumerate(zip(consts, quads)):
        with mp.workdps(40):
            v = mp.fsum(cs) + mp.fsum(mp.mpf(float(c)) * mp.mpf(float(e)) for c, e, _ in qs)
            values.append(float(v))
            tc.append(float(mp.fsum(abs(c) for c in cs)))
        tq.append(sum(abs(c * e) for c, e, _ in qs))
        err.append(sum(abs(c) * er for c, _, er in qs))
    return Ref(values, tq, tc, err)


def _classes(kind, y):
    """A count y < 0 and a non-finite real y: ell = -inf (NaN for NaN), NaN derivatives."""
    P = NPARAMS[kind]
    nan = float("nan")
    if kind in ("negbinomial", "poisson") and y < 0:
        return Ref([-math.inf] + [nan] * P, [0.0] * (1 + P), [0.0] * (1 + P), [0.0] * (1 + P))
    if kind in ("studentt", "laplace", "heterogauss") and not math.isfinite(y):
        return Ref([nan if math.isnan(y) else -math.inf] + [nan] * P, [0.0] * (1 + P), [0.0] * (1 + P), [0.0] * (1 + P))
    return None


def _terms(kind, p, y, mu, var, logistic, studentt, eabs):
    """The quadrature terms per output from the three expectation functions (float64 quad or mpmath)."""
    if kind == "bernoulli":
        (lsp, lsn, _), (e0, e1, _) = logistic(mu, var)
        return [[(1.0, lsp, e0) if y else (1.0, lsn, e1)]]
    if kind == "negbinomial":
        (lsp, lsn, _), (e0, e1, _) = logistic(mu, var)
        return [[(float(y), lsp, e0), (p[0], lsn, e1)], [(p[0], lsn, e1)]]
    if kind == "poisson":
        (lsp, _, sig), (e0, _, e2) = logistic(mu, var)
        return [[(float(y), lsp, e0), (-p[0], sig, e2)], [(-p[0], sig, e2)]]
    if kind == "studentt":
        nu = p[0]
        (el, ef), (e0, e1) = studentt(nu, p[1], y, mu, var)
        return [[(-0.5 * (nu + 1.0), el, e0)], [(-0.5 * nu, el, e0), (0.5 * (nu + 1.0), ef, e1)], [(nu + 1.0, ef, e1)]]
    if kind == "laplace":
        ea, e0 = eabs(p[0], y, mu, var)
        return [[(-1.0 / p[0], ea, e0)], [(1.0 / p[0], ea, e0)]]
    (mf, mg), (vf, vg) = mu, var
    (lsp, _, sig), (e0, _, e2) = logistic(mg, vg)
    c = 0.5 * p[0] * ((y - mf) ** 2 + vf)  # E (y - f)^2 in closed form
    return [[(0.5, lsp, e0), (-c, sig, e2)], [(-c, sig, e2)]]


def reference(kind, p, y, mu, var):
    """Ref(values, tq, tc, err) of one point: ell and the derivatives in the order of the descriptor's parameters."""
    cls = _classes(kind, y)
    if cls is not None:
        return cls
    quads = _terms(kind, p, y, mu, var, logistic_expectations, studentt_expectations, expected_abs)
    ref = _assemble(kind, _constants(kind, p, y), quads)
    if kind == "laplace":  # no quadrature in the kernel: E|y - f| / beta is a closed-form term there
        return Ref(ref.values, [0.0, 0.0], [c + q for c, q in zip(ref.tc, ref.tq)], ref.err)
    return ref


# ---- the second evaluation: mpmath at 30 digits

def _mp_quad_t(fun, breaks, dps):
    edges = sorted({mp.mpf(-WIDTH), mp.mpf(WIDTH), *[mp.mpf(2 * k) for k in range(-6, 7)], *[mp.mpf(b) for b in breaks if -WIDTH < b < WIDTH]})
    c = 1 / mp.sqrt(2 * mp.pi)
    return mp.quad(lambda t: fun(t) * mp.exp(-t * t / 2) * c, edges)


def _mp_ladder(centre, width, s):
    out = [centre / s]
    k = width
    while k < 2 * WIDTH * s + abs(centre):
        out += [(centre + k) / s, (centre - k) / s]
        k = 2 * k
    return out


def mp_logistic_expectations(mu, var, dps=30):
    with mp.workdps(dps):
        m = mp.mpf(float(mu))
        ls = lambda f: -mp.log1p(mp.exp(-f)) if f >= 0 else f - mp.log1p(mp.exp(f))
        sg = lambda f: 1 / (1 + mp.exp(-f)) if f >= 0 else mp.exp(f) / (1 + mp.exp(f))
        if var <= TINY_VAR:
            return (_f(ls(m)), _f(ls(-m)), _f(sg(m))), (0.0, 0.0, 0.0)
        s = mp.sqrt(mp.mpf(float(var)))
        z = _mp_quad_t(lambda t: mp.mpc(ls(m + s * t), sg(m + s * t)), _mp_ladder(-m, mp.mpf(1) / 2, s), dps)
        return (_f(z.real), _f(z.real - m), _f(z.imag)), (0.0, 0.0, 0.0)  # log sigma(-f) = log sigma(f) - f


def mp_studentt_expectations(nu, sg, y, mu, var, dps=30):
    with mp.workdps(dps):
        a, d = mp.mpf(float(sg)) * mp.sqrt(mp.mpf(float(nu))), mp.mpf(float(y)) - mp.mpf(float(mu))
        if var <= TINY_VAR:
            u = (d / a) ** 2
            return (_f(mp.log1p(u)), _f(u / (1 + u))), (0.0, 0.0)
        s = mp.sqrt(mp.mpf(float(var)))

        def fun(t):
            u = ((d - s * t) / a) ** 2
            return mp.mpc(mp.log1p(u), u / (1 + u))

        z = _mp_quad_t(fun, _mp_ladder(d, a / 2, s), dps)
        return (_f(z.real), _f(z.imag)), (0.0, 0.0)


def mp_expected_abs(beta, y, mu, var, dps=30):
    """The erf form."""
    with mp.workdps(dps):
        d, v = mp.mpf(float(y)) - mp.mpf(float(mu)), mp.mpf(float(var))
        if var == 0.0:
            return _f(abs(d)), 0.0
        s = mp.sqrt(v)
        return _f(s * mp.sqrt(2 / mp.pi) * mp.exp(-d * d / (2 * v)) + d * mp.erf(d / (s * mp.sqrt(2)))), 0.0


def mp_reference(kind, p, y, mu, var):
    """The values of reference(...) from the second evaluation."""
    cls = _classes(kind, y)
    if cls is not None:
        return cls.values
    quads = _terms(kind, p, y, mu, var, mp_logistic_expectations, mp_studentt_expectations, mp_expected_abs)
    return _assemble(kind, _constants(kind, p, y), quads).values
