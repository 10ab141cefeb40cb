"""Float64 reference of the asymmetric Laplace likelihood (AGPL_LIK_ASYMLAPLACE = 9, include/agpl.h): the per-point rules of
agpl_lik_rules.h restated in numpy, the closed forms of the prediction end, and the means to check those closed forms themselves:
adaptive quadrature of the defining integrals (scipy quad, split at f = y as tests/predictive_reference.py does) and mpmath at 50
digits.  No GPU and no library of the package is used here.

ALD(y | f; sigma, tau) = tau (1 - tau) / sigma exp(-rho_tau((y - f) / sigma)),  rho_tau(u) = u (tau - 1[u < 0])
                       = 4 tau (1 - tau) exp(kappa (y - f)) Laplace(y | f; beta = 2 sigma),  kappa = (1 - 2 tau) / (2 sigma)."""
import math

import numpy as np
from scipy import integrate, optimize, special

KIND = 9
SQRT_HALF = math.sqrt(0.5)


def kappa(sigma, tau):
    return (1.0 - 2.0 * tau) / (2.0 * sigma)


def logconst(tau):
    return math.log(4.0 * tau * (1.0 - tau))


# ---- the per-point rules (agpl_lik_rules.h, agpl_operators.hip) ----------------------------------------------------------------
def aux_posterior(sigma, y, mu, var):
    """o1 of aux_posterior!: Laplace's at beta = 2 sigma (tau is not read)."""
    return 1.0 / (2.0 * (2.0 * sigma) * np.sqrt((mu - y) ** 2 + var))


def expected_potential_precision(sigma, tau, y, o1):
    return 2.0 * o1 * y - kappa(sigma, tau), 2.0 * o1


def sampled_potential_precision(sigma, tau, y, omega):
    return 2.0 * omega * y - kappa(sigma, tau), 2.0 * omega


def logtilt_terms(sigma, tau, y, omega, f):
    d = y - f
    return -math.log(2.0 * (2.0 * sigma)) - d * d * omega + kappa(sigma, tau) * d + logconst(tau)


def logtilt(sigma, tau, y, omega, f):
    return float(np.sum(logtilt_terms(sigma, tau, y, omega, f)))


def expected_logtilt_terms(sigma, tau, y, o1, mu, var):
    return -math.log(2.0 * (2.0 * sigma)) - ((mu - y) ** 2 + var) * o1 + kappa(sigma, tau) * (y - mu) + logconst(tau)


def expected_logtilt(sigma, tau, y, o1, mu, var):
    return float(np.sum(expected_logtilt_terms(sigma, tau, y, o1, mu, var)))


def aux_kl_terms(sigma, o1):
    """laplace.jl:96-104 as the package codes it, lambda = (2 beta)^-2, beta = 2 sigma."""
    lam = 1.0 / (4.0 * sigma) ** 2
    return math.log(2.0 * lam) / 2.0 - math.log(2.0 * math.pi) / 2.0 - math.log(lam) / 2.0 + math.lgamma(0.5) + lam / o1


def aux_kl(sigma, o1):
    return float(np.sum(aux_kl_terms(sigma, o1)))


def aux_prior_logpdf(sigma, omega):
    """InverseGamma(1/2, (2 beta)^-2) at beta = 2 sigma."""
    lam = 1.0 / (4.0 * sigma) ** 2
    return float(np.sum(0.5 * math.log(lam) - math.lgamma(0.5) - 1.5 * np.log(omega) - lam / omega))


def aug_loglik(sigma, tau, y, omega, f):
    return logtilt(sigma, tau, y, omega, f) + aux_prior_logpdf(sigma, omega)


def elbo_terms(sigma, tau, y, mu, var):
    o1 = aux_posterior(sigma, y, mu, var)
    return float(np.sum(expected_logtilt_terms(sigma, tau, y, o1, mu, var) - aux_kl_terms(sigma, o1)))


def loglik(sigma, tau, y, f):
    """log ALD(y | f)."""
    u = (np.asarray(y, dtype=np.float64) - f) / sigma
    return math.log(tau * (1.0 - tau) / sigma) - np.where(u < 0, (tau - 1.0) * u, tau * u)


# ---- the prediction end: closed forms ------------------------------------------------------------------------------------------
def moments(sigma, tau, mu, var):
    tt = tau * (1.0 - tau)
    return mu + sigma * (1.0 - 2.0 * tau) / tt, var + sigma * sigma * (1.0 - 2.0 * tau + 2.0 * tau * tau) / (tt * tt)


def logp(sigma, tau, y, mu, var):
    """log of the predictive density at one point, through erfcx."""
    d, a, b = y - mu, tau / sigma, (1.0 - tau) / sigma
    lc = math.log(tau * (1.0 - tau) / sigma)
    if var == 0.0:
        return lc - (-b * d if d < 0 else a * d)
    s = math.sqrt(var)
    q = 0.5 * d * d / var
    z1, z2 = (a * s - d / s) * SQRT_HALF, (b * s + d / s) * SQRT_HALF
    t1 = -q + math.log(special.erfcx(z1)) if z1 > 0 else 0.5 * var * a * a - a * d + math.log(special.erfc(z1))
    t2 = -q + math.log(special.erfcx(z2)) if z2 > 0 else 0.5 * var * b * b + b * d + math.log(special.erfc(z2))
    hi, lo = max(t1, t2), min(t1, t2)
    return hi + math.log1p(math.exp(lo - hi)) + lc - math.log(2.0)


def _tail(t, var, r1, w1, r2, w2):
    """The tail on the side of t <= 0 (include/agpl_quantile.h): r1, w1 the rate and weight of the term that stays scaled."""
    if var == 0.0:
        return w2 * math.exp(r2 * t)
    s = math.sqrt(var)
    q = 0.5 * t * t / var
    eq = math.exp(-q)
    z0, z1, z2 = -t / s * SQRT_HALF, (r1 * s - t / s) * SQRT_HALF, (r2 * s + t / s) * SQRT_HALF
    third = 0.5 * w2 * eq * special.erfcx(z2) if z2 > 0 else 0.5 * w2 * math.exp(0.5 * var * r2 * r2 + r2 * t) * special.erfc(z2)
    return eq * (0.5 * special.erfcx(z0) - 0.5 * w1 * special.erfcx(z1)) + third


def cdf(sigma, tau, y, mu, var):
    """(P(Y <= y), P(Y > y)) at one point: the tail on y's side of mu as such, the other as what is left."""
    d, a, b = y - mu, tau / sigma, (1.0 - tau) / sigma
    if d < 0:
        t = _tail(d, var, a, 1.0 - tau, b, tau)
        return t, 1.0 - t
    t = _tail(-d, var, b, tau, a, 1.0 - tau)
    return 1.0 - t, t


def quantile(sigma, tau, p, mu, var):
    """brentq on the closed-form tail that p is in."""
    sc = math.sqrt(moments(sigma, tau, mu, var)[1])
    fn = (lambda y: cdf(sigma, tau, y, mu, var)[0] - p) if p <= 0.5 else (lambda y: (1.0 - p) - cdf(sigma, tau, y, mu, var)[1])
    lo, hi = mu - sc, mu + sc
    while fn(lo) > 0:
        lo = mu - 2.0 * (mu - lo)
    while fn(hi) < 0:
        hi = mu + 2.0 * (hi - mu)
    return optimize.brentq(fn, lo, hi, xtol=1e-300, rtol=8.9e-16)


def expected_loglik(sigma, tau, y, mu, var):
    """(ell, d ell / d log sigma) per point: E of the pinball loss = E|y - f| / (2 sigma) + (tau - 1/2)(y - mu) / sigma."""
    d = np.asarray(y, dtype=np.float64) - mu
    s = np.sqrt(var)
    with np.errstate(divide="ignore", invalid="ignore"):
        ea = np.where(var == 0.0, np.abs(d), s * math.sqrt(2.0 / math.pi) * np.exp(-0.5 * d * d / var) + d * special.erf(d / s * SQRT_HALF))
    pin = ea / (2.0 * sigma) + (tau - 0.5) * d / sigma
    return math.log(tau * (1.0 - tau) / sigma) - pin, -1.0 + pin


def inverse_cdf(sigma, tau, f, u):
    """The rule of include/agpl_sample_y.h on given uniforms."""
    d = u - tau
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(d < 0, f + sigma * np.log1p(d / tau) / (1.0 - tau), f - sigma * np.log1p(-d / (1.0 - tau)) / tau)


# ---- the closed forms' own check: quadrature of the defining integrals -------------------------------------------------------
def _edges(sigma, tau, y, mu, s, width=40.0):
    """Break points of an integral over f: where the Gaussian and the likelihood's two exponentials die out, the kink at f = y, and
    the stationary points of their products on either side of it (mu - b var above y, mu + a var below)."""
    w = 60.0 * sigma / min(tau, 1.0 - tau)
    e = {mu - width * s, mu, mu + width * s, y - w, y, y + w}
    up, dn = mu - s * s * (1.0 - tau) / sigma, mu + s * s * tau / sigma
    if up > y:
        e |= {up, up + 8.0 * s, max(up - 8.0 * s, y)}
    if dn < y:
        e |= {dn, dn - 8.0 * s, min(dn + 8.0 * s, y)}
    return sorted(e)


def _quad(fun, edges):
    import warnings

    tot = err = 0.0
    for lo, hi in zip(edges, edges[1:]):
        with warnings.catch_warnings():  # (a piece that cannot reach epsrel says so in its error estimate, which the caller reads)
            warnings.simplefilter("ignore", integrate.IntegrationWarning)
            v, e = integrate.quad(fun, lo, hi, epsabs=0.0, epsrel=1e-13, limit=400)
        tot, err = tot + v, err + e
    return tot, err


def _lognorm(f, mu, s):
    return -0.5 * ((f - mu) / s) ** 2 - math.log(s) - 0.5 * math.log(2.0 * math.pi)


def logp_quad(sigma, tau, y, mu, var):
    """(log p, relative error estimate) of p(y) = int ALD(y | f) N(f; mu, var) df."""
    s = math.sqrt(var)
    edges = _edges(sigma, tau, y, mu, s)
    lf = lambda f: float(loglik(sigma, tau, y, f)) + _lognorm(f, mu, s)
    top = max(lf(c) for c in edges)  # (concave on each side of y: the largest value is at y or at a stationary point, both edges)
    v, e = _quad(lambda f: math.exp(lf(f) - top), edges)
    return top + math.log(v), e / v


def cdf_quad(sigma, tau, y, mu, var):
    """((cdf, sf), (relative error estimates)): each tail the integral of its own positive integrand."""
    s = math.sqrt(var)
    a, b = tau / sigma, (1.0 - tau) / sigma
    edges = _edges(sigma, tau, y, mu, s)

    def lower(f):  # P(Y <= y | f)
        return tau * math.exp(b * (y - f)) if y < f else -math.expm1(-a * (y - f)) + tau * math.exp(-a * (y - f))

    def upper(f):
        return (1.0 - tau) * math.exp(-a * (y - f)) if y >= f else -math.expm1(b * (y - f)) + (1.0 - tau) * math.exp(b * (y - f))

    out, errs = [], []
    for g in (lower, upper):
        v, e = _quad(lambda f: g(f) * math.exp(_lognorm(f, mu, s)), edges)
        out.append(v)
        errs.append(e / v if v > 0 else math.inf)
    return tuple(out), tuple(errs)


# ---- ... and mpmath at 50 digits (the defining formulas as the issue states them: no rearrangement is needed there) ---------
def _mp():
    import mpmath

    mpmath.mp.dps = 50
    return mpmath


def mp_terms(sigma, tau, y, mu, var):
    """(log p, cdf, sf) at 50 digits from Phi and exp directly (mpmath has no overflow and 50 digits outlast the cancellation)."""
    mp = _mp()
    sg, ta, d, v = mp.mpf(sigma), mp.mpf(tau), mp.mpf(y) - mp.mpf(mu), mp.mpf(var)
    a, b = ta / sg, (1 - ta) / sg
    if var == 0.0:
        dens = ta * (1 - ta) / sg * (mp.exp(-a * d) if d >= 0 else mp.exp(b * d))
        c = ta * mp.exp(b * d) if d < 0 else 1 - (1 - ta) * mp.exp(-a * d)
        sf = 1 - ta * mp.exp(b * d) if d < 0 else (1 - ta) * mp.exp(-a * d)
        return float(mp.log(dens)), float(c), float(sf)
    s = mp.sqrt(v)
    Phi = lambda x: mp.erfc(-x / mp.sqrt(2)) / 2
    A = mp.exp(-a * d + a * a * v / 2) * Phi(d / s - a * s)
    B = mp.exp(b * d + b * b * v / 2) * Phi(-d / s - b * s)
    lp = mp.log(ta * (1 - ta) / sg) + mp.log(A + B)
    c = Phi(d / s) - (1 - ta) * A + ta * B
    sf = Phi(-d / s) + (1 - ta) * A - ta * B
    return float(lp), float(c), float(sf)


def mp_logp_quad(sigma, tau, y, mu, var):
    """log p by mpmath's own quadrature of the defining integral, split at f = y and where the two factors die out."""
    mp = _mp()
    sg, ta, yy, m, s = mp.mpf(sigma), mp.mpf(tau), mp.mpf(y), mp.mpf(mu), mp.sqrt(mp.mpf(var))
    a, b = ta / sg, (1 - ta) / sg
    dens = lambda f: (mp.exp(-a * (yy - f)) if yy >= f else mp.exp(b * (yy - f))) * mp.exp(-((f - m) / s) ** 2 / 2)
    # the break points of the double-precision quadrature, and the reach of each of the likelihood's exponentials about y
    pts = {mp.mpf(e) for e in _edges(sigma, tau, y, mu, math.sqrt(var), width=45.0)} | {yy - 130 / a, yy - 8 / a, yy + 8 / b, yy + 130 / b}
    val = mp.quad(dens, sorted(pts), maxdegree=10)
    return float(mp.log(ta * (1 - ta) / sg) + mp.log(val) - mp.log(s) - mp.log(2 * mp.pi) / 2)


# ---- the domain grid of the issue, with its 50-digit values (computed once per process) -----------------------------------
TAUS = (0.01, 0.1, 0.5, 0.9, 0.99)
SIGMAS = (1e-3, 1.0, 50.0)
VARS = (0.0, 1e-8, 1.0, 1e4)
DS = (0.0, 1.0, -1.0, 8.0, -8.0, 40.0, -40.0)  # d / sqrt(var + sigma^2)
GRID_MU = 0.75
_GRID = []


def grid():
    """Rows (sigma, tau, var, y, log p, cdf, sf), the last three from mpmath at 50 digits, at mu = GRID_MU."""
    if not _GRID:
        for sigma in SIGMAS:
            for tau in TAUS:
                for var in VARS:
                    for u in DS:
                        y = GRID_MU + u * math.sqrt(var + sigma * sigma)
                        _GRID.append((sigma, tau, var, y) + mp_terms(sigma, tau, y, GRID_MU, var))
    return np.array(_GRID)


# ---- sweeps, float64 --------------------------------------------------------------------------------------------------------
def cavi_sweeps(sigma, tau, Phi, kdiag, y, nsweeps, mu0=None):
    """``nsweeps`` CAVI sweeps on float64 features Phi [N, M] with the Nystrom residual kdiag [N], from q(v) = N(0, I), as the
    package's sweep runs them: the marginals (mu = mu0 + Phi m, var = kdiag + phi' S phi), aux_posterior!, the expected
    potential / precision, G = Phi' Diag(gamma) Phi, g = Phi' beta, S = (I + G)^-1, m = S g.  Returns the lists of G, g, S, m and
    of the ELBO of the q(v) each sweep used (its per-point terms minus KL(q(v) || N(0, I)))."""
    N, M = Phi.shape
    S, m = np.eye(M), np.zeros(M)
    y = y.astype(np.float64)
    m0 = 0.0 if mu0 is None else mu0.astype(np.float64)
    out = dict(G=[], g=[], S=[], m=[], elbo=[], mu=[], var=[], beta=[], gamma=[])
    for _ in range(nsweeps):
        mu = m0 + Phi @ m
        var = kdiag + np.einsum("ia,ab,ib->i", Phi, S, Phi)
        o1 = aux_posterior(sigma, y, mu, var)
        beta, gamma = expected_potential_precision(sigma, tau, y, o1)
        klv = 0.5 * (np.trace(S) + m @ m - M - np.linalg.slogdet(S)[1])
        out["elbo"].append(elbo_terms(sigma, tau, y, mu, var) - klv)
        G = (Phi * gamma[:, None]).T @ Phi
        g = Phi.T @ beta
        S = np.linalg.inv(np.eye(M) + G)
        S = 0.5 * (S + S.T)
        m = S @ g
        for k, v in (("G", G), ("g", g), ("S", S), ("m", m), ("mu", mu), ("var", var), ("beta", beta), ("gamma", gamma)):
            out[k].append(v)
    return out


def rand_invgaussian(rng, mean, lam):
    """Michael, Schucany and Haas."""
    nu = rng.normal(size=np.shape(mean)) ** 2
    x = mean + mean * mean * nu / (2.0 * lam) - mean / (2.0 * lam) * np.sqrt(4.0 * mean * lam * nu + (mean * nu) ** 2)
    return np.where(rng.uniform(size=np.shape(mean)) <= mean / (mean + x), x, mean * mean / x)


def gibbs_sweeps(sigma, tau, Phi, kdiag, y, nsweeps, rng):
    """``nsweeps`` sweeps of the blocked Gibbs sampler built from the same rules (numpy's generator, not the package's streams):
    f | v, omega | f ~ InverseGaussian(1 / (2 beta |y - f|), 2 (2 beta)^-2) at beta = 2 sigma, v | omega ~ N(S g, S).  Returns the
    draws of f [nsweeps, N]."""
    N, M = Phi.shape
    y = y.astype(np.float64)
    v = rng.normal(size=M)
    lam = 2.0 / (4.0 * sigma) ** 2
    fs = []
    for _ in range(nsweeps):
        f = Phi @ v + np.sqrt(kdiag) * rng.normal(size=N)
        omega = rand_invgaussian(rng, 1.0 / (4.0 * sigma * np.abs(y - f)), lam)
        beta, gamma = sampled_potential_precision(sigma, tau, y, omega)
        A = np.eye(M) + (Phi * gamma[:, None]).T @ Phi
        L = np.linalg.cholesky(A)
        v = np.linalg.solve(A, Phi.T @ beta) + np.linalg.solve(L.T, rng.normal(size=M))
        fs.append(f)
    return np.array(fs)


# ---- the quantile-regression problem of the CPU test ----------------------------------------------------------------------------
def heteroscedastic_problem(N=600, M=32, seed=11):
    """1-D inputs on [-3, 3], y = sin(1.5 x) + (0.15 + 0.35 (x + 3) / 6) noise with a skewed (Gumbel) noise; whitened Nystrom
    features of a squared-exponential kernel (lengthscale 0.8) on M inducing inputs.  Returns (x, y, Phi, kdiag, features_at)."""
    rng = np.random.default_rng(seed)
    x = np.sort(rng.uniform(-3.0, 3.0, size=N))
    y = np.sin(1.5 * x) + (0.15 + 0.35 * (x + 3.0) / 6.0) * rng.gumbel(size=N)
    z = np.linspace(-3.0, 3.0, M)
    k = lambda p, q: np.exp(-0.5 * ((p[:, None] - q[None, :]) / 0.8) ** 2)
    Lz = np.linalg.cholesky(k(z, z) + 1e-6 * np.eye(M))
    feats = lambda p: np.linalg.solve(Lz, k(z, p)).T
    Phi = feats(x)
    return x, y, Phi, np.maximum(1.0 - (Phi * Phi).sum(1), 0.0), feats
