"""float64 references of the predictive distribution function P(Y <= y), its upper tail P(Y > y) and its quantiles under
q(f) = N(mu, var), for tests/test_quantile_reference_cpu.py and tests/test_gpu_quantile.py.  No GPU, no package import.

Every (cdf, sf) has two independent routes, and each tail is integrated as such (never 1 - the other):
  route "a": adaptive Gauss-Kronrod (scipy.integrate.quad, piecewise between break points at mu and at the transition) of
             phi(x) F(y | mu + s x) over x in [-12, 12], with the likelihood's own distribution function F(y | f) from scipy.special
             (Student-t: stdtr; Laplace: the two exponentials; Bernoulli: expit; heteroscedastic: f integrated analytically, over g);
  route "b": an identity -- Bernoulli: by parts, E sigma(-+f) = int Phi(+-(f - mu) / s) sigma(f) sigma(-f) df; Student-t: the Gamma
             scale mixture E_w Phi(d / sqrt(var + sigma^2 / w)) over log w; Laplace: the closed form in 60-digit mpmath;
             heteroscedastic: the same expectation over g by composite 64-point Gauss-Legendre panels (another quadrature family);
             counts: by parts, P(Y <= y) = [Q(y + 1, lambda)] + int Phi((f - mu) / s) k_y(f) df, P(Y > y) = int Phi((mu - f) / s) k_y(f) df
             with k_y = -dF(y | f) / df = Pois(y; lambda sigma) lambda sigma sigma(-f) and sigma^(y+1) sigma(-f)^r / B(r, y + 1)
             (route "a" takes F(y | f) from gammaincc / gammainc and betainc / betaincc; var = 0: scipy.stats against them).
ref_cdf returns route "a"; the CPU test proves the two agree on every point of tests/quantile_domain.py."""
import functools
import math

import mpmath
import numpy as np
from scipy import integrate, optimize, special, stats

XMAX = 12.0  # the mass of N(0, 1) beyond is 3.6e-33
_GL_X, _GL_W = np.polynomial.legendre.leggauss(64)


def _phi(x):
    return np.exp(-0.5 * x * x) / math.sqrt(2.0 * math.pi)


def _quad(fn, lo, hi, pts=()):
    """Piecewise adaptive quadrature between the break points inside (lo, hi), each piece to its own relative 1e-13."""
    edges = [lo] + sorted({float(p) for p in pts if lo < p < hi}) + [hi]
    return sum(integrate.quad(fn, a, b, epsabs=0.0, epsrel=1e-13, limit=400)[0] for a, b in zip(edges[:-1], edges[1:]))


def _over_x(F, s, xstar, width):
    """int phi(x) F(x) dx; F changes around x = xstar over `width` (both in units of x)."""
    pts = [0.0, xstar] + [xstar + sg * k * width for sg in (-1.0, 1.0) for k in (3.0, 30.0, 300.0)]
    return _quad(lambda x: _phi(x) * F(x), -XMAX, XMAX, pts)


# ---- the likelihoods' own distribution functions: (cdf, sf)[tail](t) of the standardised residual ------------------------------------
def _lap_tail(t, upper):
    t = -t if upper else t
    return 0.5 * math.exp(t) if t < 0.0 else 1.0 - 0.5 * math.exp(-t)


def _both(fn):
    return fn(False), fn(True)


@functools.lru_cache(maxsize=None)
def ref_cdf(kind, p, y, mu, var, route="a"):
    """(P(Y <= y), P(Y > y)) of the predictive; heteroscedastic: mu = (mu_f, mu_g), var = (var_f, var_g)."""
    if kind == "bernoulli":
        if y >= 1:
            return 1.0, 0.0
        s = math.sqrt(var)
        if s == 0.0:
            return float(special.expit(-mu)), float(special.expit(mu))
        if route == "a":
            return _both(lambda up: _over_x(lambda x: special.expit((1.0 if up else -1.0) * (mu + s * x)), s, -mu / s, 1.0 / s))

        def parts(up):
            sgn = -1.0 if up else 1.0  # cdf(0) = E sigma(-f) = int Phi((f - mu) / s) sigma sigma(-f) df
            fn = lambda f: special.ndtr(sgn * (f - mu) / s) * special.expit(f) * special.expit(-f)
            return _quad(fn, -60.0, 60.0, [0.0, mu] + [mu + k * s for k in (-40.0, -8.0, 8.0, 40.0)])
        return _both(parts)
    if kind == "studentt":
        nu, sg = p
        s, d = math.sqrt(var), y - mu
        if route == "a":
            if s == 0.0:
                return float(special.stdtr(nu, d / sg)), float(special.stdtr(nu, -d / sg))
            return _both(lambda up: _over_x(lambda x: special.stdtr(nu, (-1.0 if up else 1.0) * (d - s * x) / sg), s, d / s, sg / s))
        a = 0.5 * nu
        lc = a * math.log(a) - a - special.gammaln(a)
        # tau = log w: the weight exp(-a (e^tau - 1 - tau)) is below exp(-90) of its largest outside [lo, hi]
        hi = optimize.brentq(lambda t: a * (math.expm1(t) - t) - 90.0, 0.0, 50.0)
        lo = optimize.brentq(lambda t: a * (math.expm1(t) - t) - 90.0, -90.0 / a - 5.0, 0.0)
        brk = [0.0] + ([math.log(sg * sg / var)] if var > 0.0 else []) + [math.log(sg * sg / (d * d)) + k for k in (-3.0, 0.0, 3.0) if d != 0.0]
        brk += [lo / 2 ** k for k in range(1, 8)]

        def mix(up):
            sgn = -1.0 if up else 1.0
            fn = lambda t: math.exp(lc - a * (math.expm1(t) - t)) * special.ndtr(sgn * d / math.sqrt(var + sg * sg * math.exp(-t)))
            return _quad(fn, lo, hi, brk)
        return _both(mix)
    if kind == "laplace":
        beta, = p
        s, d = math.sqrt(var), y - mu
        if s == 0.0:
            return _lap_tail(d / beta, False), _lap_tail(d / beta, True)
        if route == "a":
            return _both(lambda up: _over_x(lambda x: _lap_tail((d - s * x) / beta, up), s, d / s, beta / s))
        with mpmath.workdps(60):
            def closed(dd):
                dd, ss, b = mpmath.mpf(dd), mpmath.mpf(s), mpmath.mpf(beta)
                e0 = ss * ss / (2 * b * b)
                return (mpmath.ncdf(dd / ss) - mpmath.exp(e0 - dd / b) * mpmath.ncdf(dd / ss - ss / b) / 2
                        + mpmath.exp(e0 + dd / b) * mpmath.ncdf(-dd / ss - ss / b) / 2)
            F = closed(d)
            return float(F), float(1 - F)
    if kind == "heterogauss":
        lam, = p
        (mf, mg), (vf, vg) = mu, var
        sg, d = math.sqrt(vg), y - mf
        tail = lambda x, up: special.ndtr((-1.0 if up else 1.0) * d / np.sqrt(vf + (1.0 + np.exp(-(mg + sg * x))) / lam))
        if sg == 0.0:
            return float(tail(0.0, False)), float(tail(0.0, True))
        if route == "a":
            return _both(lambda up: _over_x(lambda x: tail(x, up), sg, 0.0, 1.0 / sg))
        edges = np.linspace(-XMAX, XMAX, 97)  # panels of s_g / 4
        x = (0.5 * (edges[1:] + edges[:-1])[:, None] + 0.5 * (edges[1] - edges[0]) * _GL_X[None, :]).ravel()
        w = np.tile(0.5 * (edges[1] - edges[0]) * _GL_W, 96)
        if sg > 2.0:  # the logistic's poles at distance pi / s_g: finer panels
            edges = np.linspace(-XMAX, XMAX, 16 * 96 + 1)
            x = (0.5 * (edges[1:] + edges[:-1])[:, None] + 0.5 * (edges[1] - edges[0]) * _GL_X[None, :]).ravel()
            w = np.tile(0.5 * (edges[1] - edges[0]) * _GL_W, 16 * 96)
        return _both(lambda up: float(np.sum(w * _phi(x) * tail(x, up))))
    if kind in ("poisson", "negbinomial"):
        pois, s, y = kind == "poisson", math.sqrt(var), int(y)
        if y < 0:
            return 0.0, 1.0
        sig = lambda f: special.expit(f)
        if pois:
            G = lambda f, up: float(special.gammainc(y + 1.0, p[0] * sig(f)) if up else special.gammaincc(y + 1.0, p[0] * sig(f)))
        else:
            G = lambda f, up: float(special.betaincc(p[0], y + 1.0, sig(-f)) if up else special.betainc(p[0], y + 1.0, sig(-f)))
        if s == 0.0:
            if route == "a":
                return (1.0 - G(mu, True), G(mu, True)) if G(mu, False) > 0.5 else (G(mu, False), 1.0 - G(mu, False))
            d = stats.poisson(p[0] * sig(mu)) if pois else stats.nbinom(p[0], sig(-mu))
            return float(d.cdf(y)), float(d.sf(y))
        A, B, L = y + 1.0, (1.0 if pois else p[0]), (p[0] if pois else 0.0)
        S_ = A + B + L
        sg = 2.0 * A / (S_ + math.sqrt(S_ * S_ - 4.0 * L * A))
        fs = math.log(sg) - math.log1p(-sg)
        with mpmath.workdps(40):  # log k at its maximum in 40 digits (its terms are up to 1e6 each); float64 only for the differences
            m = mpmath.mpf
            sm = 1 / (1 + mpmath.exp(-m(fs)))
            lc = (A * mpmath.log(m(p[0])) - mpmath.loggamma(A)) if pois else (mpmath.loggamma(A + m(p[0])) - mpmath.loggamma(A) - mpmath.loggamma(m(p[0])))
            K0 = float(A * mpmath.log(sm) + B * mpmath.log(1 - sm) - L * sm + lc)
        lsp = lambda f: -np.logaddexp(0.0, -f)
        logk = lambda f: A * (lsp(f) - lsp(fs)) + B * (lsp(-f) - lsp(-fs)) - L * (sig(f) - sig(fs)) + K0
        w = min(1.0, 1.0 / math.sqrt((A + B) * sg * (1 - sg) + L * sg * (1 - sg) * (1 - 2 * sg)))
        # (the smaller tail is kept as integrated; the larger is its complement: scipy's betainc and betaincc differ by 5e-14 at r = 1e3)
        comp = lambda c_, s_: (1.0 - s_, s_) if c_ > s_ else (c_, 1.0 - c_)
        if route == "a":
            return comp(*_both(lambda up: _over_x(lambda x: G(mu + s * x, up), s, (fs - mu) / s, w / s)))
        ends = []
        for sgn in (-1.0, 1.0):
            step = w
            while logk(fs + sgn * step) > logk(fs) - 90.0 and step < 1e6:
                step *= 2.0
            ends.append(fs + sgn * step)
        brk = [fs, mu] + [fs + q * k * w for q in (-1.0, 1.0) for k in (3.0, 10.0, 30.0, 300.0)] + [mu + k * s for k in (-40.0, -8.0, 8.0, 40.0)]

        def parts(up):
            sgn = -1.0 if up else 1.0
            return _quad(lambda f: special.ndtr(sgn * (f - mu) / s) * math.exp(logk(f)), ends[0], ends[1], brk)
        return comp(float(special.gammaincc(A, p[0])) * pois + parts(False), parts(True))
    raise KeyError(kind)


def ref_count_quantile(kind, p, prob, mu, var, cap):
    """The smallest integer y <= cap with F(y) >= prob on the tail prob is in (integer bisection on route "a"), or None beyond cap."""
    reached = lambda y: ref_cdf(kind, p, y, mu, var)[0] >= prob if prob <= 0.5 else ref_cdf(kind, p, y, mu, var)[1] <= 1.0 - prob
    if not reached(cap):
        return None
    lo, hi = -1, cap
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (lo, mid) if reached(mid) else (mid, hi)
    return hi


def ref_quantile(kind, p, prob, mu, var, scale):
    """inf {y : F(y) >= prob} by brentq on the reference distribution function (the tail that prob is in); Bernoulli: 0 or 1."""
    if kind == "bernoulli":
        return 0.0 if prob <= ref_cdf(kind, p, 0, mu, var)[0] else 1.0
    loc = mu[0] if kind == "heterogauss" else mu
    resid = (lambda y: ref_cdf(kind, p, y, mu, var)[0] - prob) if prob <= 0.5 else (lambda y: (1.0 - prob) - ref_cdf(kind, p, y, mu, var)[1])
    lo = hi = loc
    step = scale
    while resid(lo) > 0.0:
        lo, step = lo - step, 2.0 * step
    step = scale
    while resid(hi) < 0.0:
        hi, step = hi + step, 2.0 * step
    return optimize.brentq(resid, lo, hi, xtol=1e-300, rtol=8.9e-16, maxiter=500)
