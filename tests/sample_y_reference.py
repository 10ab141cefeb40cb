"""Float64 reference of agpl_sample_y (include/agpl_sample_y.h): the seven rules of the header restated on the uniforms of the
built oracle (``agplo_uniforms`` at the stream index of draw (point p, draw d)), with ``normal``, Marsaglia-Tsang ``rand_gamma`` and
``rand_poisson`` restated from oracle/agpl_oracle.c:261-283, 345-385.  Plain Python / numpy float64, one draw at a time: no
fused multiply-add, the order of operations of the device code.

Every draw comes back with its MARGIN: the smallest relative distance |a - b| / max(|a|, |b|) of any comparison a < b the rule
made on the way (u < p, the gamma accept, the PTRS accepts and its floor -- the distance of the argument from the integers on
both sides --, the arrival count and the inverse-cdf walk).  A device libm that differs from the host's in the last place can
only change a draw whose margin is of that order (1e-16); tests/test_sample_y_reference_cpu.py counts the margins below 1e-9 on
the inputs of the GPU tests (none).

``variant`` swaps in one of five deliberately WRONG samplers, for the test that shows the equality test would see them.
No GPU, no library code."""
import math
from collections import namedtuple

import numpy as np

BERNOULLI, NEGBINOMIAL, STUDENTT, CATEGORICAL, CATEGORICAL_BIJ, POISSON, LAPLACE, HETEROGAUSS = range(8)
VARIANTS = ("neg_f", "no_draw", "no_point", "swap_normal", "nb_sigma")
INF = float("inf")

# a likelihood: kind, (p0, p1), logtheta
Case = namedtuple("Case", "id kind p logtheta")
CASES = [
    Case("bernoulli", BERNOULLI, (), None),
    Case("negbinomial-r0.7", NEGBINOMIAL, (0.7,), None),
    Case("negbinomial-r15", NEGBINOMIAL, (15.0,), None),
    Case("poisson-3", POISSON, (3.0,), None),
    Case("poisson-40", POISSON, (40.0,), None),
    Case("studentt-nu1.5", STUDENTT, (1.5, 0.8), None),
    Case("studentt-nu10", STUDENTT, (10.0, 0.8), None),
    Case("laplace", LAPLACE, (0.7,), None),
    Case("heterogauss", HETEROGAUSS, (2.5,), None),
    Case("categorical", CATEGORICAL, (), (0.3, -0.2, 0.5)),
    Case("categorical-bij", CATEGORICAL_BIJ, (), (0.3, -0.2, 0.5, 0.1)),
]
# the shape of the equality test: the high word of the stream changes inside the call, the draw index passes 65535
T, NS, LDF, POINT0, DRAW0, SEED, SWEEP = 3, 257, 300, 2 ** 32 - 100, 65534, 20250607, 11


def nlatent(c):
    if c.kind == CATEGORICAL:
        return len(c.logtheta)
    if c.kind == CATEGORICAL_BIJ:
        return len(c.logtheta) - 1
    return 2 if c.kind == HETEROGAUSS else 1


def case_F(c, seed=5):
    """F [T, L, LDF] float32 in [-4, 4] (the columns beyond NS are never read: they hold NaN)."""
    rng = np.random.default_rng([seed, CASES.index(c) if c in CASES else 99])
    F = rng.uniform(-4, 4, size=(T, nlatent(c), LDF)).astype(np.float32)
    F[:, :, NS:] = np.nan
    return F


def stream_index(p, d):
    return (p & 0xFFFFFFFF) | (((((p >> 32) & 0xFF) + ((1 + d) << 8)) & 0xFFFFFFFF) << 32)


class Stream:
    """The uniforms of draw (point p, draw d), taken in order; ``margin`` collects the comparisons."""

    def __init__(self, O, seed, p, sweep, d):
        self.O, self.key, self.buf, self.pos, self.margin = O, (seed, stream_index(p, d), sweep), None, 0, INF
        self._fill(16)

    def _fill(self, n):
        self.buf = self.O.uniforms(self.key[0], self.key[1], self.key[2], n)

    def u01(self):
        if self.pos == len(self.buf):
            self._fill(4 * len(self.buf))
        self.pos += 1
        return float(self.buf[self.pos - 1])

    def exp1(self):
        return -math.log(self.u01())

    def normal(self, swapped=False):
        u1 = self.u01()
        u2 = self.u01()
        if swapped:
            u1, u2 = u2, u1
        return math.sqrt(-2.0 * math.log(u1)) * math.cos(2.0 * math.pi * u2)

    def less(self, a, b):
        """a < b, recorded."""
        self.note(a, b)
        return a < b

    def note(self, a, b):
        s = max(abs(a), abs(b))
        self.margin = min(self.margin, abs(a - b) / s if s > 0 else 0.0)


def sigma(x):
    return 1.0 / (1.0 + math.exp(-x))


def rand_gamma_mt(g, shape):
    d = shape - 1.0 / 3.0
    c = 1.0 / math.sqrt(9.0 * d)
    while True:
        x = g.normal()
        v = 1.0 + c * x
        g.margin = min(g.margin, abs(v))  # v <= 0 against 1 + c x, terms of order one
        while v <= 0.0:
            x = g.normal()
            v = 1.0 + c * x
            g.margin = min(g.margin, abs(v))
        v = v * v * v
        u = g.u01()
        x2 = x * x
        if g.less(u, 1.0 - 0.0331 * x2 * x2) or g.less(math.log(u), 0.5 * x2 + d * (1.0 - v + math.log(v))):
            return d * v


def rand_gamma(g, shape):
    if shape >= 1.0:
        return rand_gamma_mt(g, shape)
    x = rand_gamma_mt(g, shape + 1.0)
    e = g.exp1()
    return x * math.exp(-e / shape)


def rand_poisson(g, mu):
    if not mu > 0.0:
        return 0
    if mu < 6.0:
        n = 0
        c = g.exp1()
        while g.less(c, mu):
            n += 1
            c += g.exp1()
        return n
    slam, loglam = math.sqrt(mu), math.log(mu)
    b = 0.931 + 2.53 * slam
    a = -0.059 + 0.02483 * b
    invalpha = 1.1239 + 1.1328 / (b - 3.4)
    vr = 0.9277 - 3.6224 / (b - 2.0)
    while True:
        U = g.u01() - 0.5
        V = g.u01()
        us = 0.5 - abs(U)
        arg = (2.0 * a / us + b) * U + mu + 0.43
        kf = math.floor(arg)
        g.margin = min(g.margin, min(arg - kf, kf + 1.0 - arg) / max(abs(arg), 1.0))
        g.note(us, 0.07)
        if us >= 0.07:
            g.note(V, vr)
            if V <= vr:
                return int(kf)
        if kf < 0.0:
            continue
        g.note(us, 0.013)
        if us < 0.013:
            g.note(V, us)
            if V > us:
                continue
        lhs = math.log(V) + math.log(invalpha) - math.log(a / (us * us) + b)
        rhs = -mu + kf * loglam - math.lgamma(kf + 1.0)
        g.note(lhs, rhs)
        if lhs <= rhs:
            return int(kf)


def count(k):
    return min(k, 2 ** 31 - 1)


def draw(O, c, f, seed, p, sweep, d, variant=None):
    """One draw of y for the latents ``f`` (length L, float64 values of the float32 F): (value, margin); a categorical value is
    the class index (L = the implicit class of the bijective link)."""
    g = Stream(O, seed, p, sweep, d)
    k, f0 = c.kind, float(f[0])
    if variant == "neg_f":
        f0 = -f0
    if not all(math.isfinite(float(v)) for v in f):
        return (-1 if k in (NEGBINOMIAL, POISSON) else 255 if k in (BERNOULLI, CATEGORICAL, CATEGORICAL_BIJ) else math.nan), INF
    if k == BERNOULLI:
        y = 1 if g.less(g.u01(), sigma(f0)) else 0
    elif k in (CATEGORICAL, CATEGORICAL_BIJ):
        L = len(f)
        theta = [math.exp(t) for t in c.logtheta]
        tot = theta[L] * 0.5 if k == CATEGORICAL_BIJ else 0.0
        w = [theta[j] * sigma(float(f[j])) for j in range(L)]
        for j in range(L):
            tot += w[j]
        u = g.u01() * tot
        cum, y = 0.0, L
        for j in range(L):
            cum += w[j]
            if g.less(u, cum):
                y = j
                break
        if k == CATEGORICAL and y == L:
            y = L - 1
    elif k == POISSON:
        y = count(rand_poisson(g, c.p[0] * sigma(f0)))
    elif k == NEGBINOMIAL:
        a = rand_gamma(g, c.p[0])
        lam = a * (sigma(f0) if variant == "nb_sigma" else math.exp(f0))
        y = 2 ** 31 - 1 if lam >= 2 ** 31 - 1 else count(rand_poisson(g, lam))
    elif k == STUDENTT:
        z = g.normal(swapped=variant == "swap_normal")
        ch = 2.0 * rand_gamma(g, c.p[0] / 2.0)
        y = f0 + c.p[1] * z / math.sqrt(ch / c.p[0])
    elif k == LAPLACE:
        dd = g.u01() - 0.5
        y = f0 - c.p[0] * float(np.sign(dd)) * math.log1p(-2.0 * abs(dd))
    else:
        z = g.normal()
        y = f0 + z / math.sqrt(c.p[0] * sigma(float(f[1])))
    return y, g.margin


def sample(O, c, F, seed, point0, draw0, sweep, ns=None, variant=None):
    """The reference of one agpl_sample_y call on F [T, L, ldf] (its first ``ns`` columns; all by default): (y, margin), y in
    the layout of the entry point ([T, ns], one-hot [T, ns, L] for the categorical kinds), margin float64 [T, ns]."""
    Tn, L, ldf = F.shape
    ns = ldf if ns is None else ns
    cat = c.kind in (CATEGORICAL, CATEGORICAL_BIJ)
    dtype = np.uint8 if cat or c.kind == BERNOULLI else np.int32 if c.kind in (NEGBINOMIAL, POISSON) else np.float64
    y = np.zeros((Tn, ns, L) if cat else (Tn, ns), dtype=dtype)
    margin = np.full((Tn, ns), INF)
    for t in range(Tn):
        for i in range(ns):
            p = i if variant == "no_point" else point0 + i
            d = 0 if variant == "no_draw" else draw0 + t
            v, margin[t, i] = draw(O, c, F[t, :, i].astype(np.float64), seed, p, sweep, d, variant)
            if not cat:
                y[t, i] = v
            elif v == 255:
                y[t, i, :] = 255
            elif v < L:
                y[t, i, v] = 1
    return y, margin


_cache = {}


def case_reference(O, c):
    """(F, y, margin) of an equality case, computed once."""
    if c.id not in _cache:
        F = case_F(c)
        _cache[c.id] = (F,) + sample(O, c, F, SEED, POINT0, DRAW0, SWEEP, ns=NS)
    return _cache[c.id]


# ---- closed forms of p(y | f), for the statistics ------------------------------------------------------------------------------
def count_moments(c, f):
    """Mean, variance and fourth central moment of the count y | f by direct sums over its probabilities."""
    if c.kind == POISSON:
        mu = c.p[0] * sigma(f)
        return mu, mu, mu + 3.0 * mu * mu
    r, m = c.p[0], c.p[0] * math.exp(f)
    q = 1.0 / (1.0 + math.exp(-f))  # sigma(f): P(y) = Gamma(y + r) / (y! Gamma(r)) sigma(f)^y sigma(-f)^r
    v = m * (1.0 + math.exp(f))
    K = int(m + 60.0 * math.sqrt(v) + 60)
    ks = np.arange(K + 1, dtype=np.float64)
    lg = np.array([math.lgamma(x + r) - math.lgamma(x + 1.0) for x in ks]) - math.lgamma(r)
    pm = np.exp(lg + ks * math.log(q) + r * math.log1p(-q))
    assert abs(pm.sum() - 1.0) < 1e-9, pm.sum()
    return m, v, float(((ks - m) ** 4 * pm).sum())


def studentt_central_mass(nu, half_width=1.0, n=200001):
    """P(|t_nu| <= half_width): the trapezoid rule on the density."""
    x = np.linspace(-half_width, half_width, n)
    dens = np.exp(math.lgamma(0.5 * (nu + 1)) - math.lgamma(0.5 * nu) - 0.5 * math.log(nu * math.pi) - 0.5 * (nu + 1) * np.log1p(x * x / nu))
    return float((dens.sum() - 0.5 * (dens[0] + dens[-1])) * (x[1] - x[0]))


# ---- moments of the marginal p(y) = int p(y | f) N(f; mu, s^2) df, for the Monte Carlo bars -----------------------------------------
def marginal_moments(c, mu, s, mu_g=0.0, s_g=0.0, nodes=200):
    """(mean, variance, fourth central moment) of y under q(f) = N(mu, s^2) (and q(g) for the heteroscedastic link) by Gauss-Hermite
    quadrature of the conditional cumulants of y | f.  Not for the categorical kinds or a Student-t with nu <= 4."""
    x, w = np.polynomial.hermite_e.hermegauss(nodes)
    w = w / w.sum()
    f = mu + s * x
    sg = 1.0 / (1.0 + np.exp(-f))
    zero = np.zeros_like(f)
    if c.kind == BERNOULLI:
        m, v, c3, c4 = sg, sg * (1 - sg), sg * (1 - sg) * (1 - 2 * sg), sg * (1 - sg) * (1 - 3 * sg * (1 - sg))
    elif c.kind == POISSON:
        lam = c.p[0] * sg
        m, v, c3, c4 = lam, lam, lam, lam + 3 * lam * lam
    elif c.kind == NEGBINOMIAL:
        r, b = c.p[0], np.exp(f)  # cumulants of -r log(1 - b (e^t - 1))
        m, v = r * b, r * b * (1 + b)
        c3, c4 = v * (1 + 2 * b), v * (1 + 6 * b + 6 * b * b) + 3 * v * v
    elif c.kind == STUDENTT:
        nu, sc = c.p
        m, v, c3, c4 = f, zero + sc * sc * nu / (nu - 2), zero, zero + 3 * sc ** 4 * nu * nu / ((nu - 2) * (nu - 4))
    elif c.kind == LAPLACE:
        m, v, c3, c4 = f, zero + 2 * c.p[0] ** 2, zero, zero + 24 * c.p[0] ** 4
    elif c.kind == HETEROGAUSS:
        vg = (1.0 + np.exp(-(mu_g + s_g * x))) / c.p[0]  # the noise variance under q(g), independent of f
        ev, ev2 = float((w * vg).sum()), float((w * vg * vg).sum())
        return mu, s * s + ev, 3 * s ** 4 + 6 * s * s * ev + 3 * ev2
    else:
        raise ValueError(c.kind)
    M = float((w * m).sum())
    d = m - M
    return M, float((w * (v + d * d)).sum()), float((w * (c4 + 4 * c3 * d + 6 * v * d * d + d ** 4)).sum())
