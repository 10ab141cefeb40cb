"""References of log p(y*) and of the predictive moments that can be trusted on the whole grid of tests/predictive_domain.py: the same
integral as tests/predictive_reference.py (whose likelihoods it uses), with
  - a mode search that has no +- 40 s limit: candidates on a geometric ladder out to 4e4 s and at the observation, then a bounded
    refinement between the neighbours of the best;
  - the integrand scaled by its value AT the mode and evaluated as a difference, log p(y | f) - log p(y | m) through log1p / expm1
    (the three logistic likelihoods), so that a count of 2^31 - 1 -- where log p(y | f) itself is 1e7 to 1e10 -- keeps its digits;
  - the count's constant log C(y + r - 1, y) in mpmath where float64 lgamma cancels (y + r > 1e3), and the Student-t density's
    lgamma((nu + 1) / 2) - lgamma(nu / 2) likewise;
  - break points at the mode +- 4^k widths, so that a peak 1e-5 s wide is found by quad's bisection;
  - moments by their class: a negative-binomial mean that overflows has variance +inf.
A second, independent evaluation in mpmath (30 digits, tanh-sinh): the same integral for the logistic and heteroscedastic kinds, the
Gamma scale mixture (not the integral over f) for Student-t, the erfc closed form for Laplace.  No GPU, nothing imports the package."""
import mpmath as mp
import numpy as np
from scipy import integrate, optimize, special

import predictive_reference as R

LOG_SQRT_2PI = R.LOG_SQRT_2PI
_LADDER = np.concatenate([np.linspace(-40.0, 40.0, 801), np.geomspace(40.0, 4e4, 400)[1:], -np.geomspace(40.0, 4e4, 400)[1:]])


def log_count_const(kind, p, y):
    """The factor of p(y | f) that does not depend on f."""
    if kind == "negbinomial":
        r = p[0]
        if y + r > 1e3:
            with mp.workdps(40):
                return float(mp.loggamma(mp.mpf(y) + mp.mpf(r)) - mp.loggamma(mp.mpf(y) + 1) - mp.loggamma(mp.mpf(r)))
        return float(special.gammaln(y + r) - special.gammaln(y + 1.0) - special.gammaln(r))
    if kind == "poisson":
        with mp.workdps(40):
            return float(mp.mpf(y) * mp.log(mp.mpf(p[0])) - mp.loggamma(mp.mpf(y) + 1))
    if kind == "studentt":
        # lgamma((nu + 1) / 2) - lgamma(nu / 2) cancels in float64 (6e6 each at nu = 1e6: 1e-9): the correction of R.loglik's value
        nu = p[0]
        with mp.workdps(40):
            exact = mp.loggamma((mp.mpf(nu) + 1) / 2) - mp.loggamma(mp.mpf(nu) / 2)
            return float(exact - mp.mpf(float(special.gammaln(0.5 * (nu + 1.0)) - special.gammaln(0.5 * nu))))
    return 0.0


def _abl(kind, p, y):
    return {"bernoulli": (y, 1.0 - y, 0.0), "negbinomial": (y, p[0], 0.0), "poisson": (y, 0.0, p[0])}[kind]


def _core(kind, p, y, f):
    """log p(y | f) without the constant of y."""
    if kind in ("bernoulli", "negbinomial", "poisson"):
        A, B, L = _abl(kind, p, y)
        return A * R.logsig(f) + B * R.logsig(-f) - L * special.expit(f)
    return R.loglik(kind, p, y, f)


def _core_diff(kind, p, y, f, m):
    """_core(f) - _core(m) without cancellation: log sigma(f) - log sigma(m) = -log1p(sigma(-m) expm1(m - f)), and so on."""
    if kind in ("bernoulli", "negbinomial", "poisson"):
        A, B, L = _abl(kind, p, y)
        with np.errstate(all="ignore"):
            e = np.expm1(np.minimum(m - f, 700.0))
            q = special.expit(-m) * e
            # (where the argument of log1p is not small the plain difference has no cancellation left to avoid)
            dpos = np.where(np.abs(q) < 0.5, -np.log1p(np.where(np.abs(q) < 0.5, q, 0.0)), R.logsig(f) - R.logsig(m))
            dneg = dpos - (f - m)  # log sigma(-f) - log sigma(-m)
            return A * dpos + B * dneg + L * special.expit(f) * special.expit(-m) * e
    return _core(kind, p, y, f) - _core(kind, p, y, m)


def _find_mode(h, mu, s, extra):
    cand = np.sort(np.concatenate([mu + s * _LADDER, np.asarray(extra, dtype=np.float64)]))
    with np.errstate(all="ignore"):
        hv = np.where(np.isnan(hc := h(cand)), -np.inf, hc)
    k = int(np.argmax(hv))
    lo, hi = cand[max(k - 1, 0)], cand[min(k + 1, len(cand) - 1)]
    r = optimize.minimize_scalar(lambda f: -h(f), bounds=(lo, hi), method="bounded", options={"xatol": 1e-13 * max(1.0, abs(cand[k])) + 1e-300})
    m = float(r.x) if h(r.x) >= hv[k] else float(cand[k])
    return m


def _width(hdiff, m, s):
    """(-h'')^-1/2 at the mode from a central difference of h(f) - h(m), at most s."""
    w = s
    for _ in range(60):
        d2 = (hdiff(m + 0.25 * w) + hdiff(m - 0.25 * w)) / (0.25 * w) ** 2
        if not np.isfinite(d2) or d2 >= 0.0:
            return w
        w2 = min(s, 1.0 / np.sqrt(-d2))
        if w2 > 0.7 * w:
            return w2
        w = w2
    return w


def _breaks(m, w, a, b, extra):
    ks = w * 4.0 ** np.arange(0, 40)
    pts = {m, *[e for e in extra if a < e < b], *[m + k for k in ks if m + k < b], *[m - k for k in ks if m - k > a]}
    return [a] + sorted(pts) + [b]


def _setup(kind, p, y, mu, var):
    """(h(f) - h(m) as a function, m, h(m) without the constant, s, break points)."""
    if kind == "heterogauss":
        (mf, mg), (vf, vg) = mu, var
        lam, dd = p[0], (y - mf) ** 2

        def core(g):
            with np.errstate(over="ignore"):
                v = vf + (1.0 + np.exp(-g)) / lam
            return -0.5 * np.log(2.0 * np.pi * v) - 0.5 * dd / v

        mu, var, extra = mg, vg, ()
        cdiff = lambda f, m: core(f) - core(m)
    else:
        core = lambda f: _core(kind, p, float(y), f)
        cdiff = lambda f, m: _core_diff(kind, p, float(y), f, m)
        extra = (float(y),) if kind in ("studentt", "laplace") else ()
    s = np.sqrt(var)
    h = lambda f: core(f) - 0.5 * ((f - mu) / s) ** 2
    m = _find_mode(h, mu, s, extra)
    # in the offset d = f - m, so that s = 1e-8 at |mu| = 40 does not lose the Gaussian factor to the rounding of f
    hdiff = lambda d: cdiff(m + d, m) - 0.5 * d * (d + 2.0 * (m - mu)) / var
    w = _width(hdiff, 0.0, s)
    a, b = min(mu - m, 0.0) - 16.0 * s, max(mu - m, 0.0) + 16.0 * s
    return hdiff, m, float(core(m) - 0.5 * ((m - mu) / s) ** 2), s, _breaks(0.0, w, a, b, tuple(e - m for e in (mu,) + extra)), core, mu


def ref_logp(kind, p, y, mu, var):
    """(log p(y), quad's error estimate relative to the integral)."""
    zero = var[1] == 0.0 if kind == "heterogauss" else var == 0.0
    c0 = log_count_const(kind, p, y)
    if zero:
        if kind == "heterogauss":
            return float(R.loglik(kind, p, y, mu[0], mu[1]) if var[0] == 0.0 else
                         -0.5 * np.log(2 * np.pi * (var[0] + (1 + np.exp(-mu[1])) / p[0])) - 0.5 * (y - mu[0]) ** 2 / (var[0] + (1 + np.exp(-mu[1])) / p[0])), 0.0
        return c0 + float(_core(kind, p, float(y), mu)), 0.0
    hdiff, m, hm, s, edges, _, _ = _setup(kind, p, y, mu, var)
    tot, err = 0.0, 0.0
    with np.errstate(over="ignore", under="ignore"):
        for lo, hi in zip(edges[:-1], edges[1:]):
            v, e = integrate.quad(lambda f: np.exp(hdiff(f)), lo, hi, epsabs=1e-300, epsrel=1e-13, limit=200)
            tot, err = tot + v, err + e
    return c0 + hm + np.log(tot) - np.log(s) - LOG_SQRT_2PI, err / tot


def _mpf(x):
    return mp.mpf(float(x))


def _mp_logsig(f):
    return -mp.log1p(mp.exp(-f)) if f >= 0 else f - mp.log1p(mp.exp(f))


def mp_logp(kind, p, y, mu, var, dps=30):
    """The second reference: mpmath at `dps` digits.  Break points come from the float64 set-up (they only cut the range)."""
    with mp.workdps(dps):
        if kind == "laplace":
            beta, d, v = _mpf(p[0]), _mpf(y) - _mpf(mu), _mpf(var)
            if var == 0.0:
                return float(-abs(d) / beta - mp.log(2 * beta))
            s = mp.sqrt(v)
            z1, z2 = (s / beta - d / s) / mp.sqrt(2), (s / beta + d / s) / mp.sqrt(2)
            e0 = v / (2 * beta * beta)
            t1, t2 = e0 - d / beta + mp.log(mp.erfc(z1)), e0 + d / beta + mp.log(mp.erfc(z2))
            hi = max(t1, t2)
            return float(hi + mp.log(mp.exp(t1 - hi) + mp.exp(t2 - hi)) - mp.log(4 * beta))
        if kind == "studentt":
            nu, sg = _mpf(p[0]), _mpf(p[1])
            if var == 0.0:
                z = (_mpf(y) - _mpf(mu)) / sg
                return float(mp.loggamma((nu + 1) / 2) - mp.loggamma(nu / 2) - mp.log(nu * mp.pi) / 2 - mp.log(sg) - (nu + 1) / 2 * mp.log1p(z * z / nu))
            a, c, dd, v0 = nu / 2, nu * sg * sg / 2, (_mpf(y) - _mpf(mu)) ** 2, _mpf(var)
            g = lambda t: a * t - mp.exp(t) - mp.log(v0 + c * mp.exp(-t)) / 2 - dd / (2 * (v0 + c * mp.exp(-t)))
            fa, fc, fd, fv = float(a), float(c), float(dd), float(var)
            ts = np.concatenate([np.linspace(-400.0, 20.0, 8401), np.log(fa) + np.linspace(-60.0, 60.0, 4001) / np.sqrt(fa)])
            with np.errstate(all="ignore"):
                gv = fa * ts - np.exp(ts) - 0.5 * np.log(fv + fc * np.exp(-ts)) - 0.5 * fd / (fv + fc * np.exp(-ts))
            t0 = float(ts[np.nanargmax(gv)])
            t0 = float(optimize.minimize_scalar(lambda t: -float(fa * t - np.exp(t) - 0.5 * np.log(fv + fc * np.exp(-t)) - 0.5 * fd / (fv + fc * np.exp(-t))),
                                                bounds=(t0 - 0.06, t0 + 0.06), method="bounded", options={"xatol": 1e-10}).x)
            w = min(1.0, 1.0 / np.sqrt(fa))
            ks = w * 2.0 ** np.arange(0, 12)
            pts = sorted({t0, *[t0 + k for k in ks if k < 60], *[t0 - k for k in ks if k < 600]})
            gm = g(_mpf(t0))
            tot = mp.quad(lambda t: mp.exp(g(t) - gm), [_mpf(q) for q in pts])
            return float(gm + mp.log(tot) - mp.loggamma(a) - mp.log(2 * mp.pi) / 2)
        if kind == "heterogauss":
            (mf, mg), (vf, vg) = mu, var
            lam, dd, vf_ = _mpf(p[0]), (_mpf(y) - _mpf(mf)) ** 2, _mpf(vf)

            def core(g):
                v = vf_ + (1 + mp.exp(-g)) / lam
                return -mp.log(2 * mp.pi * v) / 2 - dd / (2 * v)

            if vg == 0.0:
                return float(core(_mpf(mg)))
            c0, m_, v_ = mp.mpf(0), _mpf(mg), _mpf(vg)
        else:
            yy = _mpf(y)
            if kind == "negbinomial":
                r = _mpf(p[0])
                c0 = mp.loggamma(yy + r) - mp.loggamma(yy + 1) - mp.loggamma(r)
                core = lambda f: yy * _mp_logsig(f) + r * _mp_logsig(-f)
            elif kind == "poisson":
                lam = _mpf(p[0])
                c0 = yy * mp.log(lam) - mp.loggamma(yy + 1)
                core = lambda f: yy * _mp_logsig(f) - lam / (1 + mp.exp(-f))
            else:
                c0 = mp.mpf(0)
                core = lambda f: _mp_logsig(f) if y else _mp_logsig(-f)
            if var == 0.0:
                return float(c0 + core(_mpf(mu)))
            m_, v_ = _mpf(mu), _mpf(var)
        _, m, _, s, edges, _, _ = _setup(kind, p, y, mu, var)
        h = lambda f: core(f) - (f - m_) ** 2 / (2 * v_)
        hm = h(_mpf(m))
        tot = mp.quad(lambda f: mp.exp(h(f) - hm), [_mpf(m) + _mpf(e) for e in edges])
        return float(c0 + hm + mp.log(tot) - mp.log(v_) / 2 - mp.log(2 * mp.pi) / 2)


def mp_logp_unguided(kind, p, y, mu, var, dps=30):
    """log p(y) of a logistic kind in mpmath with nothing from the float64 set-up: break points mu + 2 k s, |k| <= 20, and -- where
    the likelihood has a maximum of its own, sigma(f) = y / (y + r) or y / lambda -- that point +- 4^k of the likelihood's width there."""
    with mp.workdps(dps):
        yy, m_, v_ = _mpf(y), _mpf(mu), _mpf(var)
        s = mp.sqrt(v_)
        if kind == "negbinomial":
            r = _mpf(p[0])
            c0 = mp.loggamma(yy + r) - mp.loggamma(yy + 1) - mp.loggamma(r)
            core = lambda f: yy * _mp_logsig(f) + r * _mp_logsig(-f)
            fstar, curv = (mp.log(yy / r), yy * r / (yy + r)) if y > 0 else (None, None)
        elif kind == "poisson":
            lam = _mpf(p[0])
            c0 = yy * mp.log(lam) - mp.loggamma(yy + 1)
            core = lambda f: yy * _mp_logsig(f) - lam / (1 + mp.exp(-f))
            fstar, curv = (mp.log(yy / (lam - yy)), yy * (1 - yy / lam)) if 0 < y < p[0] else (None, None)
        else:
            c0, fstar, curv = mp.mpf(0), None, None
            core = lambda f: _mp_logsig(f) if y else _mp_logsig(-f)
        h = lambda f: core(f) - (f - m_) ** 2 / (2 * v_)
        pts = {m_ + 2 * k * s for k in range(-20, 21)}
        if fstar is not None and abs(fstar - m_) < 40 * s:
            w = 1 / mp.sqrt(curv)
            for k in range(0, 30):
                for t in (fstar - w * 4 ** k, fstar + w * 4 ** k):
                    if abs(t - m_) < 40 * s:
                        pts.add(t)
            pts.add(fstar)
        pts = sorted(pts)
        hm = max(h(t) for t in pts)
        tot = mp.quad(lambda f: mp.exp(h(f) - hm), pts)
        return float(c0 + hm + mp.log(tot) - mp.log(v_) / 2 - mp.log(2 * mp.pi) / 2)


def _gauss_mean(fun, mu, s):
    """E fun(mu + s x), x ~ N(0, 1), over +- 16; split where the logistic bends."""
    edges = sorted({-16.0, 0.0, 16.0, *[(e - mu) / s for e in (-30.0, -8.0, -2.0, 0.0, 2.0, 8.0, 30.0) if abs(e - mu) < 16.0 * s]})
    tot = 0.0
    for lo, hi in zip(edges[:-1], edges[1:]):
        tot += integrate.quad(lambda x: fun(mu + s * x) * np.exp(-0.5 * x * x), lo, hi, epsabs=1e-300, epsrel=1e-13, limit=200)[0]
    return tot / np.sqrt(2.0 * np.pi)


def ref_moments(kind, p, mu, var):
    """(E y, Var y); a value beyond float64 is +inf."""
    if kind == "negbinomial":
        with mp.workdps(30):
            r, m1 = _mpf(p[0]), mp.exp(_mpf(mu) + _mpf(var) / 2)
            m2 = mp.exp(2 * _mpf(mu) + 2 * _mpf(var))
            big = mp.mpf(np.finfo(np.float64).max)
            mean, v = r * m1, r * (m1 + m2) + r * r * (m2 - m1 * m1)
            return (float(mean) if mean <= big else np.inf), (float(v) if v <= big else np.inf)
    if kind in ("bernoulli", "poisson") and var > 0.0:
        s = np.sqrt(var)
        e1 = _gauss_mean(special.expit, mu, s)
        if kind == "bernoulli":
            return e1, e1 * _gauss_mean(lambda f: special.expit(-f), mu, s)
        lam = p[0]
        # Var sigma as E (sigma - E sigma)^2: no cancellation where sigma is almost constant under q(f)
        return lam * e1, lam * e1 + lam * lam * _gauss_mean(lambda f: (special.expit(f) - e1) ** 2, mu, s)
    with np.errstate(over="ignore"):
        return R.ref_moments(kind, p, mu, var)
