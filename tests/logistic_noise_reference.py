"""Float64 reference of the logistic-noise likelihood (AGPL_LIK_LOGISTIC_NOISE = 10, include/agpl.h): the per-point rules of
agpl_lik_rules.h restated in numpy, the prediction end by quadrature of the DEFINING integrals over q(f) = N(mu, var)
(mpmath's tanh-sinh rule at 50 digits in the standardised latent g = (y - f) / s, split where the logistic and the Gaussian each have
their structure, rounded to float64), with the same integrals at 65 digits and by scipy's adaptive rule to hold them.  No GPU and no library of the package is used here.

y = f + s eps, eps ~ Logistic(0, 1):  p(y | f) = sech^2(z / 2) / (4 s) = sigma(z) sigma(-z) / s,  z = (y - f) / s
                                               = 1 / (4 s) E_{omega ~ PG(2, 0)} exp(-omega z^2 / 2)."""
import math
import os
import warnings

import numpy as np
from scipy import integrate

KIND = 10
VAR_LOGISTIC = math.pi ** 2 / 3.0


def logcosh(x):
    ax = np.abs(x)
    return ax + np.log1p(np.exp(-2.0 * ax)) - math.log(2.0)


def pg_mean2(c):
    """E PG(2, c) = tanh(c / 2) / c, 1/2 at c = 0."""
    c = np.asarray(c, dtype=np.float64)
    safe = np.where(c == 0.0, 1.0, c)
    return np.where(c == 0.0, 0.5, np.tanh(safe / 2.0) / safe)


# ---- the per-point rules (agpl_lik_rules.h, agpl_operators.hip) ----------------------------------------------------------------
def aux_posterior(s, y, mu, var):
    """c of q(omega) = PG(2, c)."""
    return np.sqrt((mu - y) ** 2 + var) / s


def expected_potential_precision(s, y, c):
    w = pg_mean2(c) / (s * s)
    return w * y, w


def sampled_potential_precision(s, y, omega):
    w = omega / (s * s)
    return w * y, w


def logtilt(s, y, omega, f):
    d = y - f
    return float(np.sum(-math.log(4.0 * s) - d * d * omega / (2.0 * s * s)))


def expected_logtilt_terms(s, y, c, mu, var):
    return -math.log(4.0 * s) - ((mu - y) ** 2 + var) * pg_mean2(c) / (2.0 * s * s)


def expected_logtilt(s, y, c, mu, var):
    return float(np.sum(expected_logtilt_terms(s, y, c, mu, var)))


def aux_kl_terms(c):
    """KL(PG(2, c) || PG(2, 0)) = 2 logcosh(c / 2) - c^2 E[omega] / 2."""
    return 2.0 * logcosh(c / 2.0) - c * c * pg_mean2(c) / 2.0


def aux_kl(c):
    return float(np.sum(aux_kl_terms(c)))


def elbo_terms(s, y, mu, var):
    c = aux_posterior(s, y, mu, var)
    return float(np.sum(expected_logtilt_terms(s, y, c, mu, var) - aux_kl_terms(c)))


def loglik(s, y, f):
    """log p(y | f) = -log(4 s) - 2 logcosh(z / 2)."""
    return -math.log(4.0 * s) - 2.0 * logcosh((np.asarray(y, dtype=np.float64) - f) / (2.0 * s))


def pg2_laplace(t):
    """E_{w ~ PG(2, 0)} exp(-w t) from the product form prod_k (1 + t / (2 pi^2 (k - 1/2)^2))^-2, not from cosh^-2."""
    k = np.arange(1, 2_000_001, dtype=np.float64)
    d = 2.0 * math.pi ** 2 * (k - 0.5) ** 2
    tail = t / (2.0 * math.pi ** 2 * k[-1])
    return math.exp(-2.0 * (float(np.sum(np.log1p(t / d))) + tail))


def inverse_cdf(s, f, u):
    """The rule of include/agpl_sample_y.h on given uniforms."""
    return f + s * (np.log(u) - np.log1p(-u))


def moments(s, mu, var):
    return mu, var + s * s * VAR_LOGISTIC


# ---- the prediction end: quadrature of the defining integrals over g ~ N(m, R^2), m = (y - mu) / s, R = sqrt(var) / s -----------
def _lsig(g):
    return -np.logaddexp(0.0, -g)


def _breaks(m, R):
    """Break points over g: the Gaussian's own reach m +- 38 R together with the logistic's |g| <= 745 (at 50 standard deviations
    with R large the density's mass sits at the logistic's peak, far outside the Gaussian's reach); what is cut carries less than
    exp(-700) of either factor's mass."""
    lo, hi = min(m - 38.0 * R, -745.0), max(m + 38.0 * R, 745.0)
    pts = {lo, hi, m} | {m + k * R for k in (-38.0, -12.0, -6.0, -2.0, 2.0, 6.0, 12.0, 38.0)}
    pts |= {p for p in (0.0, -2.0, 2.0, -8.0, 8.0, -40.0, 40.0, -745.0, 745.0) if lo < p < hi}
    if abs(m) > R * R:  # the stationary point of exp(-|g|) N(g; m, R^2)
        c = m - math.copysign(R * R, m)
        pts |= {p for p in (c, c - 6.0 * R, c + 6.0 * R) if lo < p < hi}
    return sorted(pts)


def _std(s, y, mu, var):
    return (y - mu) / s, math.sqrt(var) / s


_CACHE = {}


def _mp_point(s, y, mu, var, which, dps):
    """One of the defining integrals over g ~ N(m, R^2) by mpmath's tanh-sinh rule between the break points above, at ``dps`` digits:
    which = "dens" (E sigma(g) sigma(-g)), "cdf" (E sigma(g)), "sf" (E sigma(-g)), "lse" (E[log sigma(g) + log sigma(-g)]) or "gt"
    (E[g tanh(g / 2)], integrated as it stands: no use of Stein's lemma).  Returned as an mpf; var = 0 is the integrand at m."""
    key = (s, y, mu, var, which, dps)
    if key not in _CACHE:
        import mpmath as mp

        with mp.workdps(dps):
            m = (mp.mpf(y) - mp.mpf(mu)) / mp.mpf(s)
            sig = lambda g: 1 / (1 + mp.exp(-g))
            fun = {"dens": lambda g: sig(g) * sig(-g), "cdf": sig, "sf": lambda g: sig(-g),
                   "lse": lambda g: -(abs(g) + 2 * mp.log1p(mp.exp(-abs(g)))), "gt": lambda g: g * mp.tanh(g / 2)}[which]
            if var == 0.0:
                _CACHE[key] = fun(m)
            else:
                R = mp.sqrt(mp.mpf(var)) / mp.mpf(s)
                edges = [mp.mpf(e) for e in _breaks(float(m), float(R))]
                _CACHE[key] = mp.quad(lambda g: fun(g) * mp.exp(-((g - m) / R) ** 2 / 2), edges, maxdegree=10) / (R * mp.sqrt(2 * mp.pi))
    return _CACHE[key]


REF_DPS = 50  # (at 30 digits the rule's degree limit is reached before the narrow Gaussians of R = 1e-5 converge: 3e-8 off)


def logp(s, y, mu, var, dps=REF_DPS):
    import mpmath as mp

    return float(mp.log(_mp_point(s, y, mu, var, "dens", dps)) - mp.log(mp.mpf(s)))


def cdf(s, y, mu, var, dps=REF_DPS):
    """(P(Y <= y), P(Y > y)): each tail the integral of its own positive integrand."""
    return float(_mp_point(s, y, mu, var, "cdf", dps)), float(_mp_point(s, y, mu, var, "sf", dps))


def tail(s, y, mu, var, upper, dps=REF_DPS):
    return float(_mp_point(s, y, mu, var, "sf" if upper else "cdf", dps))


def expected_loglik_point(s, y, mu, var, dps=REF_DPS, value=True):
    """(ell, d ell / d log s) at one point: ell = -log s + E[log sigma(g) + log sigma(-g)], d ell / d log s = -1 + E[g tanh(g / 2)]."""
    import mpmath as mp

    ell = float(_mp_point(s, y, mu, var, "lse", dps) - mp.log(mp.mpf(s))) if value else math.nan
    return ell, float(-1 + _mp_point(s, y, mu, var, "gt", dps))


def expected_loglik(s, y, mu, var, value=True):
    out = np.array([expected_loglik_point(s, float(y[i]), float(mu[i]), float(var[i]), value=value) for i in range(len(y))])
    return out[:, 0], out[:, 1]


# ---- ... held to scipy's adaptive quadrature of the same integrals where it reports a small error, and to 50 digits -----------
def _quad(fun, edges):
    tot = err = 0.0
    for a, b in zip(edges, edges[1:]):
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", integrate.IntegrationWarning)
            v, e = integrate.quad(fun, a, b, epsabs=0.0, epsrel=1e-13, limit=400)
        tot, err = tot + v, err + e
    return tot, err


def scipy_terms(s, y, mu, var):
    """((E sigma sigma(-), E sigma, E sigma(-)), (relative error estimates)) by scipy quad, var > 0, without rescaling: only where
    the integrand does not underflow."""
    m, R = _std(s, y, mu, var)
    edges = _breaks(m, R)
    w = lambda g: math.exp(-0.5 * ((g - m) / R) ** 2) / (R * math.sqrt(2.0 * math.pi))
    sg = lambda g: math.exp(-np.logaddexp(0.0, -g))
    out = [_quad(lambda g, f=f: f(g) * w(g), edges) for f in (lambda g: sg(g) * sg(-g), sg, lambda g: sg(-g))]
    return tuple(v for v, _ in out), tuple(e / v if v > 0 else math.inf for v, e in out)


def mp_terms(s, y, mu, var):
    """(log p, cdf, sf, ell, d ell / d log s) at 50 digits."""
    return (logp(s, y, mu, var, 50),) + cdf(s, y, mu, var, 50) + expected_loglik_point(s, y, mu, var, 50)


# ---- the domain grid of the issue, with its 50-digit values (computed once per process) -----------------------------------
SCALES = (1e-3, 1.0, 1e3)
SDS = (0.0, 1e-8, 1.0, 50.0)                   # sqrt(var)
DEVS = (0.0, 1.0, -1.0, 8.0, -8.0, 50.0, -50.0)  # (y - mu) / the predictive's standard deviation
GRID_MU = 0.75
_GRID = []


GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "logistic_noise_grid.npy")


def grid():
    """The grid's rows as stored in tests/golden (5 KB; the 315 integrals at 50 digits take half a minute): what the GPU tests read.
    tests/test_logistic_noise_reference_cpu.py holds the file to compute_grid()."""
    return np.load(GOLDEN)


def compute_grid():
    """Rows (s, var, y, log p, cdf, sf, ell, d ell / d log s), the last five from mpmath at 50 digits, at mu = GRID_MU."""
    if not _GRID:
        for s in SCALES:
            for sd in SDS:
                for u in DEVS:
                    var = sd * sd
                    y = GRID_MU + u * math.sqrt(var + s * s * VAR_LOGISTIC)
                    _GRID.append((s, var, y) + mp_terms(s, y, GRID_MU, var))
    return np.array(_GRID)


# ---- sweeps, float64 --------------------------------------------------------------------------------------------------------
def cavi_sweeps(s, Phi, kdiag, y, nsweeps, mu0=None):
    """``nsweeps`` CAVI sweeps on float64 features Phi [N, M] with the Nystrom residual kdiag [N], from q(v) = N(0, I), as the
    package's sweep runs them.  Returns the lists of G, g, S, m, the marginals, the sites and the ELBO of the q(v) each sweep used."""
    N, M = Phi.shape
    S, m = np.eye(M), np.zeros(M)
    y = y.astype(np.float64)
    m0 = 0.0 if mu0 is None else mu0.astype(np.float64)
    out = dict(G=[], g=[], S=[], m=[], elbo=[], mu=[], var=[], beta=[], gamma=[])
    for _ in range(nsweeps):
        mu = m0 + Phi @ m
        var = kdiag + np.einsum("ia,ab,ib->i", Phi, S, Phi)
        beta, gamma = expected_potential_precision(s, y, aux_posterior(s, y, mu, var))
        klv = 0.5 * (np.trace(S) + m @ m - M - np.linalg.slogdet(S)[1])
        out["elbo"].append(elbo_terms(s, y, mu, var) - klv)
        G = (Phi * gamma[:, None]).T @ Phi
        g = Phi.T @ beta
        S = np.linalg.inv(np.eye(M) + G)
        S = 0.5 * (S + S.T)
        m = S @ g
        for k, v in (("G", G), ("g", g), ("S", S), ("m", m), ("mu", mu), ("var", var), ("beta", beta), ("gamma", gamma)):
            out[k].append(v)
    return out
