"""Float64 reference of the binomial likelihood (AGPL_LIK_BINOMIAL, include/agpl.h): Binomial(n, sigma(f)), y successes out of n
trials.  The kind has no file in the reference package and the oracle does not know it, so its rules are restated here in numpy
plus math.lgamma, the predictive integrals by the adaptive integration of tests/predictive_reference.py (scipy's quad, split at
mu and at the mode), and the header's rule for draws of y (include/agpl_sample_y.h) on the oracle's uniforms the way
tests/sample_y_reference.py restates the other kinds.  No GPU, no library code: nothing here imports the package.

The identity everything rests on (any exponent pair; b = n):
    C(n,y) s(f)^y s(-f)^(n-y) = C(n,y) 2^-n exp((y - n/2) f) E_{w ~ PG(n,0)} exp(-w f^2 / 2),    s = logistic."""
import math

import numpy as np
from scipy import optimize, special

import predictive_reference as PR
from sample_y_reference import Stream

KIND = 8
BINOMIAL_DIRECT = 64   # include/agpl_sample_y.h: up to here y is the sum of n comparisons
BINOMIAL_WALK = 10.0   # beyond: the inverse-cdf walk while n q < 10, BTRS from there
NEG_INF = -math.inf


def logC(n, y):
    """log C(n, y) from lgamma; -inf for a count outside 0..n (the pole of lgamma the device meets)."""
    if y < 0 or y > n:
        return NEG_INF
    return math.lgamma(n + 1.0) - math.lgamma(y + 1.0) - math.lgamma(n - y + 1.0)


def logC_vec(n, y):
    return np.array([logC(n, float(v)) for v in np.asarray(y).ravel()]).reshape(np.shape(y))


def sigma(x):
    return 1.0 / (1.0 + np.exp(-x))


def logcosh(x):
    ax = np.abs(x)
    return ax + np.log1p(np.exp(-2.0 * ax)) - math.log(2.0)


def pg_mean(b, c):
    """E PG(b, c) = b tanh(c / 2) / (2 c), b / 4 at c = 0."""
    c = np.asarray(c, dtype=np.float64)
    safe = np.where(c == 0.0, 1.0, c)
    return np.where(c == 0.0, b / 4.0, b * np.tanh(safe / 2.0) / (2.0 * safe))


# ---- the per-point rules -------------------------------------------------------------------------------------------------------
def aux_posterior(mu, var):
    """c of q(omega) = PG(n, c); does not read y."""
    return np.sqrt(mu * mu + var)


def expected_potential_precision(n, y, c):
    return y - n / 2.0, pg_mean(float(n), c)


def sampled_potential_precision(n, y, omega):
    return y - n / 2.0, omega


def logtilt(n, y, omega, f):
    """sum_i logC(n, y_i) - n log 2 + (y_i - n/2) f_i - omega_i f_i^2 / 2."""
    return float(np.sum(logC_vec(n, y) - n * math.log(2.0) + (y - n / 2.0) * f - omega * f * f / 2.0))


def expected_logtilt(n, y, c, mu, var):
    th = pg_mean(float(n), c)
    return float(np.sum(logC_vec(n, y) - n * math.log(2.0) + (y - n / 2.0) * mu - (mu * mu + var) * th / 2.0))


def aux_kl(n, c):
    """KL(PG(n, c) || PG(n, 0)) = n logcosh(c / 2) - c^2 E[omega] / 2, summed."""
    return float(np.sum(n * logcosh(c / 2.0) - c * c * pg_mean(float(n), c) / 2.0))


def elbo_terms(n, y, mu, var):
    """sum_i expected_logtilt_i - aux_kldivergence_i at the optimal q(omega): the per-point part of the ELBO."""
    c = aux_posterior(mu, var)
    return expected_logtilt(n, y, c, mu, var) - aux_kl(n, c)


# ---- p(y | f) and its Polya-Gamma form ----------------------------------------------------------------------------------------
def loglik(n, y, f):
    """log Binomial(y; n, sigma(f))."""
    lc = logC(n, float(y))
    if lc == NEG_INF:
        return NEG_INF if np.ndim(f) == 0 else np.full(np.shape(f), NEG_INF)
    return lc + y * PR.logsig(f) + (n - y) * PR.logsig(-f)


def pg_laplace(b, t):
    """E_{w ~ PG(b, 0)} exp(-w t) = cosh(sqrt(t / 2))^-b: the Laplace transform that defines the Polya-Gamma family, evaluated here
    from its product form prod_k (1 + t / (2 pi^2 (k - 1/2)^2))^-b (the law of sum_k g_k / (2 pi^2 (k - 1/2)^2), g_k ~ Gamma(b, 1))
    so that the check of the identity does not assume the closed form it would otherwise be comparing with itself."""
    k = np.arange(1, 2_000_001, dtype=np.float64)
    d = 2.0 * math.pi ** 2 * (k - 0.5) ** 2
    tail = t / (2.0 * math.pi ** 2 * (k[-1]))  # sum_{k > K} t / d_k ~ t / (2 pi^2 K): first order of the remainder
    return math.exp(-b * (float(np.sum(np.log1p(t / d))) + tail))


def pg_identity_sides(n, y, f):
    """(C(n,y) s(f)^y s(-f)^(n-y),  C(n,y) 2^-n exp((y - n/2) f) E exp(-w f^2 / 2))."""
    lhs = math.exp(loglik(n, y, float(f)))
    rhs = math.exp(logC(n, y) - n * math.log(2.0) + (y - n / 2.0) * f) * pg_laplace(float(n), f * f / 2.0)
    return lhs, rhs


# ---- the predictive distribution under q(f) = N(mu, var) ---------------------------------------------------------------------
def ref_logp(n, y, mu, var):
    """(log int Binomial(y; n, sigma(f)) N(f; mu, var) df, relative error estimate)."""
    if logC(n, float(y)) == NEG_INF:
        return NEG_INF, 0.0
    if var == 0.0:
        return float(loglik(n, y, mu)), 0.0
    return _gauss_quad_concave(n, y, mu, math.sqrt(var))


def _gauss_quad_concave(n, y, mu, s):
    """PR._gauss_quad for this likelihood, with the mode found where that function's search grid (mu +- 40 s) does not reach: the
    integrand's logarithm h(f) = loglik(f) - (f - mu)^2 / (2 s^2) is concave and h'(f) = y - n sigma(f) - (f - mu) / s^2 has
    |y - n sigma| <= n, so its root lies within n s^2 of mu (n = 1000, s = 0.1, mu = 40, y = 0: 100 s away).  Then the same
    adaptive integration of exp(h - h(mode)), split at mu, the mode and a few widths (-h'')^-1/2 around it, over both +- 16 s."""
    h = lambda f: loglik(n, y, f) - 0.5 * ((f - mu) / s) ** 2
    d1 = lambda f: y - n * float(special.expit(f)) - (f - mu) / (s * s)
    r = n * s * s + 1.0
    mode = optimize.brentq(d1, mu - r, mu + r, xtol=1e-14, rtol=8.9e-16)
    sg = float(special.expit(mode))
    w = 1.0 / math.sqrt(n * sg * (1.0 - sg) + 1.0 / (s * s))
    hm = float(h(mode))
    a, b = min(mu, mode) - 16.0 * s, max(mu, mode) + 16.0 * s
    pts = sorted({a, b, mu, mode, *[mode + k * w for k in (-12.0, -4.0, 4.0, 12.0) if a < mode + k * w < b]})
    tot, err = PR._quad_pieces(lambda f: np.exp(h(f) - hm), pts)
    return hm + math.log(tot) - math.log(s) - PR.LOG_SQRT_2PI, err / tot


def ref_moments(n, mu, var):
    """(E y, Var y) = (n e1, n (e1 - e2) + n^2 (e2 - e1^2)), e_k = E sigma(f)^k."""
    if var == 0.0:
        e1 = float(special.expit(mu))
        e2 = e1 * e1
    else:
        s = math.sqrt(var)
        e1 = PR._gauss_mean(special.expit, mu, s)[0]
        e2 = PR._gauss_mean(lambda f: special.expit(f) ** 2, mu, s)[0]
    return n * e1, n * (e1 - e2) + n * n * (e2 - e1 * e1)


def ref_moments_direct(n, mu, var):
    """The same two moments with the variance from terms that do not cancel where sigma is within rounding of 0 or 1 or q(f) is
    narrow: E[sigma (1 - sigma)] as the integral of sigma(f) sigma(-f), and Var sigma = E d^2 - (E d)^2 with d = sigma(f) - sigma(mu)
    (an integration error of 1e-7 relative in E sigma itself, which quad leaves at s = 1e-8, would otherwise enter n^2 Var sigma
    as 1e-14 n^2)."""
    if var == 0.0:
        p = float(special.expit(mu))
        return n * p, n * float(special.expit(mu) * special.expit(-mu))
    s = math.sqrt(var)
    s0 = float(special.expit(mu))
    e1 = PR._gauss_mean(special.expit, mu, s)[0]
    a = PR._gauss_mean(lambda f: special.expit(f) * special.expit(-f), mu, s)[0]
    d1 = PR._gauss_mean(lambda f: special.expit(f) - s0, mu, s)[0]
    d2 = PR._gauss_mean(lambda f: (special.expit(f) - s0) ** 2, mu, s)[0]
    return n * e1, n * a + n * n * (d2 - d1 * d1)


def pmf_all(n, mu, s):
    """p(y), y = 0 .. n, by the trapezoid rule on a grid fine enough for the narrowest factor: the likelihood's peak in f is at
    least 2 / sqrt(n) wide and q(f) is s wide, the spacing a sixth of the smaller, the range mu +- 12 s.  For an integrand that is
    analytic and Gaussian-like of width w the rule's error at spacing h is exp(-2 pi^2 w^2 / h^2): nothing at w / h = 6."""
    h = min(s, 2.0 / math.sqrt(n)) / 6.0
    m = int(math.ceil(12.0 * s / h))
    f = mu + h * np.arange(-m, m + 1, dtype=np.float64)
    w = np.exp(-0.5 * ((f - mu) / s) ** 2) * (h / (s * math.sqrt(2.0 * math.pi)))
    ys = np.arange(n + 1, dtype=np.float64)
    lc = logC_vec(n, ys)
    lsp, lsn = PR.logsig(f), PR.logsig(-f)
    out = np.empty(n + 1)
    for j0 in range(0, n + 1, 128):  # (blocks of y: [128, nodes] at a time)
        yy = ys[j0:j0 + 128, None]
        out[j0:j0 + 128] = np.exp(lc[j0:j0 + 128, None] + yy * lsp[None, :] + (n - yy) * lsn[None, :]) @ w
    return out


def cdf_all(n, mu, s):
    """(P(Y <= y), P(Y > y)) for y = 0 .. n: cumulative sums of the mass function from each end, so that neither tail is
    1 - (a number near 1)."""
    p = pmf_all(n, mu, s)
    cdf = np.cumsum(p)
    sf = np.concatenate([np.cumsum(p[::-1])[::-1][1:], [0.0]])
    return cdf, sf


def quantile(cdf, p):
    """The smallest y with cdf(y) >= p."""
    return int(np.searchsorted(cdf, p, side="left"))


# ---- the expected log-likelihood ---------------------------------------------------------------------------------------------
def expected_loglik(n, y, mu, var):
    """logC(n, y) + y E log sigma(f) + (n - y) E log sigma(-f) per point, by adaptive quadrature."""
    out = np.empty(len(y))
    for i in range(len(y)):
        lc = logC(n, float(y[i]))
        if lc == NEG_INF:
            out[i] = NEG_INF
            continue
        if var[i] == 0.0:
            a, b = float(PR.logsig(mu[i])), float(PR.logsig(-mu[i]))
        else:
            s = math.sqrt(var[i])
            g = lambda f, sign: PR.logsig(sign * f) * np.exp(-0.5 * ((f - mu[i]) / s) ** 2)
            c = s * math.sqrt(2.0 * math.pi)
            pts = sorted({mu[i] - 16.0 * s, mu[i], mu[i] + 16.0 * s} | ({0.0} if abs(mu[i]) < 16.0 * s else set()))
            a = PR._quad_pieces(lambda f: g(f, 1.0), pts)[0] / c
            b = PR._quad_pieces(lambda f: g(f, -1.0), pts)[0] / c
        out[i] = lc + y[i] * a + (n - y[i]) * b
    return out


# ---- draws of y: the rule of include/agpl_sample_y.h ---------------------------------------------------------------------------
def draw_y(O, n, f, seed, p, sweep, d):
    """(y, margin) of draw d of global point p: the header's rule on the draw's Philox sub-stream (margin: the smallest relative
    distance of a comparison the rule made, tests/sample_y_reference.py)."""
    g = Stream(O, seed, p, sweep, d)
    if not math.isfinite(f):
        return -1, math.inf
    pr = 1.0 / (1.0 + math.exp(-f))
    if n <= BINOMIAL_DIRECT:
        y = 0
        for _ in range(int(n)):
            y += 1 if g.less(g.u01(), pr) else 0
        return y, g.margin
    flip = pr > 0.5
    g.note(pr, 0.5)
    q = 1.0 - pr if flip else pr
    nf = float(n)
    g.note(nf * q, BINOMIAL_WALK)
    if nf * q < BINOMIAL_WALK:
        s = q / (1.0 - q)
        a = (nf + 1.0) * s
        r = math.exp(nf * math.log1p(-q))
        u = g.u01()
        k = 0.0
        while k < nf:
            g.note(u, r)
            if not u > r:
                break
            u -= r
            k += 1.0
            r *= a / k - s
    else:
        spq = math.sqrt(nf * q * (1.0 - q))
        b = 1.15 + 2.53 * spq
        a = -0.0873 + 0.0248 * b + 0.01 * q
        c = nf * q + 0.5
        vr = 0.92 - 4.2 / b
        alpha = (2.83 + 5.1 / b) * spq
        lpq = math.log(q / (1.0 - q))
        m = math.floor((nf + 1.0) * q)
        h = math.lgamma(m + 1.0) + math.lgamma(nf - m + 1.0)
        while True:
            U = g.u01() - 0.5
            V = g.u01()
            us = 0.5 - abs(U)
            arg = (2.0 * a / us + b) * U + c
            k = math.floor(arg)
            g.margin = min(g.margin, min(arg - k, k + 1.0 - arg) / max(abs(arg), 1.0))
            if k < 0.0 or k > nf:
                continue
            g.note(us, 0.07)
            if us >= 0.07:
                g.note(V, vr)
                if V <= vr:
                    break
            lhs = math.log(V * alpha / (a / (us * us) + b))
            rhs = h - math.lgamma(k + 1.0) - math.lgamma(nf - k + 1.0) + (k - m) * lpq
            g.note(lhs, rhs)
            if lhs <= rhs:
                break
    return int(nf - k if flip else k), g.margin


def sample_y(O, n, F, seed, point0, draw0, sweep):
    """The reference of one agpl_sample_y call on F [T, 1, Ns]: (y int32 [T, Ns], margin [T, Ns])."""
    T, _, Ns = F.shape
    y = np.zeros((T, Ns), dtype=np.int32)
    margin = np.full((T, Ns), math.inf)
    for t in range(T):
        for i in range(Ns):
            y[t, i], margin[t, i] = draw_y(O, n, float(F[t, 0, i]), seed, point0 + i, sweep, draw0 + t)
    return y, margin


# ---- sweeps, float64 --------------------------------------------------------------------------------------------------------
def cavi_sweeps(n, Phi, kdiag, y, nsweeps, bernoulli=False):
    """``nsweeps`` CAVI sweeps on float64 features Phi [N, M] with the Nystrom residual kdiag [N] (k_ii - |phi_i|^2), from
    q(v) = N(0, I): per sweep the marginals of q(v) (mu = Phi m, var = kdiag + phi' S phi), aux_posterior!, the expected potential / precision, G = Phi' Diag(gamma) Phi, g = Phi' beta, then
    S = (I + G)^-1, m = S g.  Returns the lists of G, g, S, m and of the ELBO of the q(v) each sweep used
    (its per-point terms minus KL(q(v) || N(0, I))).  ``bernoulli``: the Bernoulli rules (beta = +-1/2, b = 1), y in {0, 1}."""
    N, M = Phi.shape
    S, m = np.eye(M), np.zeros(M)
    y = y.astype(np.float64)
    out = dict(G=[], g=[], S=[], m=[], elbo=[])
    nt = 1.0 if bernoulli else float(n)
    for _ in range(nsweeps):
        mu = Phi @ m
        var = kdiag + np.einsum("ia,ab,ib->i", Phi, S, Phi)
        c = aux_posterior(mu, var)
        beta, gamma = y - nt / 2.0, pg_mean(nt, c)
        klv = 0.5 * (np.trace(S) + m @ m - M - np.linalg.slogdet(S)[1])
        out["elbo"].append(elbo_terms(nt, y, mu, var) - klv)
        G = (Phi * gamma[:, None]).T @ Phi
        g = Phi.T @ beta
        S = np.linalg.inv(np.eye(M) + G)
        S = 0.5 * (S + S.T)
        m = S @ g
        for k, v in (("G", G), ("g", g), ("S", S), ("m", m)):
            out[k].append(v)
    return out
