"""The per-point rules of the eight likelihoods (csrc/agpl_lik_rules.h, the float64 ELBO terms of csrc/agpl_operators.hip) stated three
times, without torch and without a GPU:

  * ``Ref``     -- mpmath at 50 digits, the reference *as coded* (the logistic cut-offs of the element type), on the
                   rounded inputs the device sees, per point, never a sum;
  * a bar per output, derived from the arithmetic while the reference runs;
  * ``Model``   -- numpy scalars of the element type in the device's order of operations, with named wrong variants.

The bar.  Every value the reference forms carries E, the first-order bound of its absolute error in units of the unit round-off u
(2^-24, 2^-53), and K, the number of roundings behind it.  Inputs have E = 0 (they are the rounded numbers the device reads); a
correctly rounded operation (+ - * / sqrt) adds max(|z|, tiny) to the propagated E, a transcendental 2 of them (one ulp: exp, log,
log1p, cosh, tanh, the accuracy device math libraries state for these) and lgamma 8 (4 ulp, of max(|z|, 1): it has
zeros at 1 and 2).  tiny = the smallest normal number, so u tiny is half a denormal spacing: the absolute floor of an operation that
underflows.  Propagation is the derivative with magnitudes: |y| Ex + |x| Ey for a product, Ex / |y| + |x| Ey / y^2 for a quotient, Ex +
Ey for a sum AND for a difference.  That is "the expression with every subtraction replaced by the sum of magnitudes": the E of
p0 = 1 - sum q2 is of size 1 + sum q2 whatever p0 is, 1 / p0 then carries (1 + sum q2) / p0 of itself, pg_kl carries b logcosh +
c^2 theta / 2, and so on, with nobody writing these down per rule.  bar = u E.  In the issue's form bar = K u A with A = E / K; K
counts ALL roundings behind an output, not the longest chain ((a b)(c d) has three roundings and a chain of two, and 3 u is its bound).
K of each rule at a typical point is the comment beside the rule in ``Ref`` (counted from the source; the tracker's own count, returned
with every value, counts a value used twice -- mu - y in its square -- twice, which moves no bar: the bar is u E).  sqrt near zero uses
sqrt(x + d) - sqrt(x) <= sqrt(d) where the derivative bound is larger.

Unresolved outputs.  Where an intermediate leaves the range of the type (overflow), or a divisor / the argument of a logarithm is not
larger than its own error bound, exact arithmetic cannot say what the type gives: the output is *unresolved*, its class (finite, +inf,
-inf, nan, negative) is the model's -- the same expression rounded in the type, which is the reference's own behaviour there (float32
p0 -> 0, 0 log 0, (1e19 + 1e19)^2) -- and the CPU module pins the set of such (point, output) pairs by name.  Everywhere else the class
is the mpmath value's and the value is held to the bar.

No bar here was tuned to a device result."""
import os
import re
from collections import namedtuple

import numpy as np
import pytest

mp = pytest.importorskip("mpmath")
mp.mp.dps = 50
mpf = mp.mpf

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "augmentedgplikelihoods.jl_amd", "csrc")

KINDS = ("bernoulli", "negbin", "studentt", "cat", "catbij", "poisson", "laplace", "hetero")
HAS_Q2 = ("cat", "catbij", "poisson", "hetero")
REAL_Y = ("studentt", "laplace", "hetero")
LOGTWO = mp.log(2)
LOG2PI = mp.log(2 * mp.pi)

Fmt = namedtuple("Fmt", "name T u maxv tiny lo hi")
F32 = Fmt("f32", np.float32, mpf(2) ** -24, mpf(float(np.finfo(np.float32).max)), mpf(2) ** -126, np.float32(-103.27893), np.float32(16.635532))
F64 = Fmt("f64", np.float64, mpf(2) ** -53, mpf(float(np.finfo(np.float64).max)), mpf(2) ** -1022, np.float64(-744.4400719213812),
          np.float64(36.7368005696771))
FMT = {"f32": F32, "f64": F64}
DENORM32 = float(np.float32(2.0) ** -149)

Point = namedtuple("Point", "name y mu var params")


def header_constants():
    """The logistic cut-offs of both element types and the c == T(0) branch of pg_mean, read from agpl_random.h."""
    src = open(os.path.join(CSRC, "agpl_random.h")).read()
    d = re.search(r"double approx_expected_logistic\(double mu, double c\) \{\s*if \(mu < (-[\d.]+)\) return 0\.0;\s*"
                  r"if \(mu > ([\d.]+)\) return 1\.0;\s*return exp\(mu / 2\.0\) \* \(1\.0 / cosh\(c / 2\.0\)\) / 2\.0;", src)
    f = re.search(r"float approx_expected_logistic\(float mu, float c\) \{\s*if \(mu < (-[\d.]+)f\) return 0\.0f;\s*"
                  r"if \(mu > ([\d.]+)f\) return 1\.0f;\s*return expf\(mu / 2\.0f\) \* \(1\.0f / coshf\(c / 2\.0f\)\) / 2\.0f;", src)
    p = re.search(r"T pg_mean\(T b, T c\) \{\s*if \(c == T\(0\)\) return b / T\(4\);\s*return b / \(T\(2\) \* c\) \* tanh\(c / T\(2\)\);", src)
    if not (d and f and p):
        raise LookupError("approx_expected_logistic / pg_mean are not stated in agpl_random.h as this module restates them")
    return {"f64": (float(d.group(1)), float(d.group(2))), "f32": (float(np.float32(f.group(1))), float(np.float32(f.group(2)))),
            "pg_mean_zero_branch": True}


def cat_consts(logtheta, bij):
    """(den of aux_posterior!, sum_theta) in float64 as agpl_lik_to_device forms them (categorical.jl:12-20)."""
    lt = np.asarray(logtheta, np.float64)
    L = len(lt) - (1 if bij else 0)
    s = np.float64(0.0)
    for k in range(L):
        s = s + np.exp(lt[k])
    cc = np.exp(lt[L]) * 0.5 if bij else np.float64(0.0)
    if bij:
        s = s + cc
    return (np.float64(cc + float(L)) if bij else np.float64(L)), s, L


def params_T(kind, params, fmt):
    """The parameters as the rule of element type T reads them: (T)lik.p[j], den = (T)(cat_const + L)."""
    T = fmt.T
    if kind in ("cat", "catbij"):
        den, st, L = cat_consts(params["logtheta"], kind == "catbij")
        return {"den": T(den), "sum_theta": st, "L": L}
    return {k: T(v) for k, v in params.items()}


# ======================================================================================================================= tracked arithmetic
class X:
    __slots__ = ("v", "e", "k", "bad")

    def __init__(self, v, e=0, k=0, bad=False):
        self.v, self.e, self.k, self.bad = v, mpf(e), k, bad


class Ar:
    """Exact arithmetic of one element type's rule: value, E (units of u), K, unresolved flag."""

    def __init__(self, fmt):
        self.f = fmt

    def inp(self, x):
        if isinstance(x, X):  # (a value the rule formed itself, with its error so far)
            return x
        x = float(x)
        if x != x or abs(x) == float("inf"):
            return X(mpf(x), 0, 0, True)
        return X(mpf(x))

    def _r(self, v, e, k, bad, w=1, floor=None):
        if not mp.isfinite(v):
            return X(v, 0, k + w, True)
        e = e + w * max(abs(v), self.f.tiny if floor is None else floor)
        return X(v, e, k + w, bad or abs(v) > self.f.maxv)

    def _c(self, a):
        """A constant of the source: exact if the type holds it, else one rounding of its own."""
        if isinstance(a, X):
            return a
        v = mpf(a)
        return X(v, 0 if mpf(float(self.f.T(float(v)))) == v else abs(v), 0)

    def add(self, a, b):
        a, b = self._c(a), self._c(b)
        return self._r(a.v + b.v, a.e + b.e, a.k + b.k, a.bad or b.bad)

    def sub(self, a, b):
        a, b = self._c(a), self._c(b)
        return self._r(a.v - b.v, a.e + b.e, a.k + b.k, a.bad or b.bad)

    def mul(self, a, b):
        a, b = self._c(a), self._c(b)
        return self._r(a.v * b.v, abs(b.v) * a.e + abs(a.v) * b.e, a.k + b.k, a.bad or b.bad)

    def scale(self, a, s):
        """Times a power of two: exact (no rounding) unless it underflows; overflow is flagged."""
        a = self._c(a)
        v = a.v * s
        e = a.e * abs(s) + (self.f.tiny if 0 < abs(v) < self.f.tiny else 0)
        return X(v, e, a.k, a.bad or abs(v) > self.f.maxv)

    def neg(self, a):
        return X(-a.v, a.e, a.k, a.bad)

    def div(self, a, b):
        a, b = self._c(a), self._c(b)
        if b.v == 0 or abs(b.v) <= b.e * self.f.u:
            return X(mp.inf if b.v == 0 else a.v / b.v, 0, a.k + b.k + 1, True)
        return self._r(a.v / b.v, a.e / abs(b.v) + abs(a.v) * b.e / (b.v * b.v), a.k + b.k, a.bad or b.bad)

    def sqrt(self, a):
        if a.v < 0:
            return X(mp.nan, 0, a.k + 1, True)
        z = mp.sqrt(a.v)
        e = mp.sqrt(a.e * self.f.u) / self.f.u
        if a.v > 0:
            e = min(e, a.e / (2 * z))
        return self._r(z, e, a.k, a.bad)

    def exp(self, a):
        z = mp.exp(a.v)
        return self._r(z, z * a.e, a.k, a.bad, w=2)

    def log(self, a):
        if a.v <= 0 or a.v <= a.e * self.f.u:
            return X(mp.log(a.v) if a.v > 0 else -mp.inf, 0, a.k + 2, True)
        return self._r(mp.log(a.v), a.e / a.v, a.k, a.bad, w=2)

    def log1p(self, a):
        return self._r(mp.log1p(a.v), a.e / (1 + a.v), a.k, a.bad, w=2)

    def tanh(self, a):
        z = mp.tanh(a.v)
        return self._r(z, a.e / mp.cosh(a.v) ** 2, a.k, a.bad, w=2)

    def sech(self, a):
        """1 / cosh(x) as the rules write it: a transcendental and a division; a cosh beyond the range gives 0 for a value
        below tiny, which the floor of the division covers only if the floor is the value itself."""
        ch = mp.cosh(a.v)
        z = 1 / ch
        e = z * abs(mp.tanh(a.v)) * a.e + 2 * z
        if ch > self.f.maxv:
            return X(z, e + z / self.f.u, a.k + 3, a.bad)
        return self._r(z, e, a.k + 2, a.bad)

    def lgamma(self, a):
        if a.v <= 0:
            return X(mp.inf, 0, a.k + 8, True)
        z = mp.loggamma(a.v)
        return self._r(z, abs(mp.digamma(a.v)) * a.e, a.k, a.bad, w=8, floor=mpf(1))

    def fabs(self, a):
        return X(abs(a.v), a.e, a.k, a.bad)


def classify(x):
    """'nan' | '+inf' | '-inf' | 'neg' | 'fin' of a float."""
    x = float(x)
    if x != x:
        return "nan"
    if x in (float("inf"), float("-inf")):
        return "+inf" if x > 0 else "-inf"
    return "neg" if x < 0 else "fin"


Out = namedtuple("Out", "v bar K unresolved")


def _out(fmt, x):
    return Out(x.v, x.e * fmt.u, x.k, bool(x.bad))


# ======================================================================================================================= the mpmath reference
class Ref:
    """The rules in exact arithmetic.  K at a typical point is noted beside each rule (``k`` of the returned value says it exactly)."""

    def __init__(self, kind, fmt, params):
        self.kind, self.fmt, self.a = kind, fmt, Ar(fmt)
        self.p = params_T(kind, params, fmt)

    # ---- helpers
    def sm(self, mu, var):  # K = 2
        a = self.a
        return a.add(a.mul(mu, mu), var)

    def sm_y(self, mu, var, y):  # K = 3
        a = self.a
        d = a.sub(mu, y)
        return a.add(a.mul(d, d), var)

    def ael(self, m, c):  # approx_expected_logistic, K = 6 (exp 2, cosh 2, 1/., *)  -- the halvings are exact
        a, f = self.a, self.fmt
        if float(m.v) < float(f.lo):
            return X(mpf(0))
        if float(m.v) > float(f.hi):
            return X(mpf(1))
        return a.scale(a.mul(a.exp(a.scale(m, mpf(1) / 2)), a.sech(a.scale(c, mpf(1) / 2))), mpf(1) / 2)

    def pg_mean(self, b, c):  # K = 4 (b / (2c), tanh 2, *)
        a = self.a
        if c.v == 0:
            return a.scale(b, mpf(1) / 4)
        return a.mul(a.div(b, a.scale(c, 2)), a.tanh(a.scale(c, mpf(1) / 2)))

    def logcosh(self, x):  # K = 6 (exp 2, log1p 2, +, -)
        a = self.a
        ax = a.fabs(x)
        return a.sub(a.add(ax, a.log1p(a.exp(a.scale(ax, -2)))), LOGTWO)

    def pg_kl(self, b, c):  # K = 4 (pg_mean) + 6 (logcosh) + 5
        a = self.a
        om = self.pg_mean(b, c)
        return a.sub(a.mul(b, self.logcosh(a.scale(c, mpf(1) / 2))), a.scale(a.mul(a.mul(c, c), om), mpf(1) / 2))

    def digamma(self, x):
        a = self.a
        r = X(mpf(0))
        while x.v < 6:
            r = a.sub(r, a.div(1, x))
            x = a.add(x, 1)
        f = a.div(1, a.mul(x, x))
        # r + log(x) - 0.5 / x - f * (1/12 - f * (1/120 - f * (1/252 - f * (1/240 - f / 132))))
        t = a.sub(mpf(1) / 240, a.div(f, 132))
        t = a.sub(mpf(1) / 252, a.mul(f, t))
        t = a.sub(mpf(1) / 120, a.mul(f, t))
        t = a.sub(mpf(1) / 12, a.mul(f, t))
        return a.sub(a.sub(a.add(r, a.log(x)), a.div(mpf(1) / 2, x)), a.mul(f, t))

    # ---- aux_posterior!: (o1[k], o2[k], o3) of one point; y, mu, var tuples of floats of the element type
    def aux_posterior(self, y, mu, var):
        a, p, kind = self.a, self.p, self.kind
        I = a.inp
        o1, o2, o3 = [], [], None
        if kind in ("bernoulli", "negbin"):  # K = 3
            o1.append(a.sqrt(self.sm(I(mu[0]), I(var[0]))))
        elif kind == "studentt":  # K = 6: nu / (sg sg) 2, second_moment_y 3, + 1; the halving is exact
            q = a.div(I(p["nu"]), a.mul(I(p["sigma"]), I(p["sigma"])))
            o1.append(a.scale(a.add(q, self.sm_y(I(mu[0]), I(var[0]), I(y[0]))), mpf(1) / 2))
        elif kind in ("cat", "catbij"):  # o1 K = 3, o2 K = 3 + 6 + 1
            for k in range(p["L"]):
                m = I(mu[k])
                c = a.sqrt(self.sm(m, I(var[k])))
                o1.append(c)
                o2.append(a.div(self.ael(a.neg(m), c), I(p["den"])))
        elif kind == "poisson":  # o2 K = 3 + 6 + 1
            m = I(mu[0])
            c = a.sqrt(self.sm(m, I(var[0])))
            o1.append(c)
            o2.append(a.mul(I(p["lam"]), self.ael(a.neg(m), c)))
        elif kind == "laplace":  # K = 3 + sqrt + 2 * beta (1, the doubling is exact) + 1 / .
            s = a.sqrt(self.sm_y(I(mu[0]), I(var[0]), I(y[0])))
            o1.append(a.div(1, a.mul(a.scale(I(p["beta"]), 2), s)))
        elif kind == "hetero":  # o3 K = 3, o2 K = 3 + 6 + 2 + 3
            o3 = a.scale(self.sm_y(I(mu[0]), I(var[0]), I(y[0])), mpf(1) / 2)
            m = I(mu[1])
            c = a.sqrt(self.sm(m, I(var[1])))
            o1.append(c)
            o2.append(a.mul(a.mul(I(p["lam"]), self.ael(a.neg(m), c)), o3))
        return o1, o2, o3

    # ---- expected potential / precision from q1, q2 (floats of the element type): (gamma[k], beta[k])
    def expected_pp(self, y, q1, q2, mu_g=None):
        a, p, kind = self.a, self.p, self.kind
        I = a.inp
        if kind == "bernoulli":  # gamma K = 4, beta exact
            return [self.pg_mean(X(mpf(1)), I(q1[0]))], [X(mpf(0.5 if y[0] != 0 else -0.5))]
        if kind == "negbin":  # gamma K = 1 + 4, beta K = 1
            r = I(p["r"])
            return [self.pg_mean(a.add(I(y[0]), r), I(q1[0]))], [a.scale(a.sub(I(y[0]), r), mpf(1) / 2)]
        if kind == "studentt":  # w K = 1 (nu + 1) + 1 (1 / b) + 1; beta + 1
            w = a.mul(a.scale(a.add(I(p["nu"]), 1), mpf(1) / 2), a.div(1, I(q1[0])))
            return [w], [a.mul(w, I(y[0]))]
        if kind in ("cat", "catbij"):  # p0 K = L + 1; nbar + 2; gamma + 1 + 4
            sp = X(mpf(0))
            for k in range(p["L"]):
                sp = a.add(sp, I(q2[k]))
            p0 = a.sub(1, sp)
            ip0 = a.div(1, p0)
            g, b = [], []
            for k in range(p["L"]):
                nbar = a.mul(ip0, I(q2[k]))
                g.append(self.pg_mean(a.add(I(y[k]), nbar), I(q1[k])))
                b.append(a.scale(a.sub(I(y[k]), nbar), mpf(1) / 2))
            return g, b
        if kind == "poisson":  # gamma K = 1 + 4
            return [self.pg_mean(a.add(I(y[0]), I(q2[0])), I(q1[0]))], [a.scale(a.sub(I(y[0]), I(q2[0])), mpf(1) / 2)]
        if kind == "laplace":  # gamma exact (a doubling), beta K = 1
            m2 = a.scale(I(q1[0]), 2)
            return [m2], [a.mul(m2, I(y[0]))]
        if kind == "hetero":  # lsg K = 6 + 2; beta0 + 1; gamma1 K = 1 + 4
            lsg = a.mul(I(p["lam"]), a.sub(1, self.ael(a.neg(I(mu_g)), I(q1[0]))))
            g1 = self.pg_mean(a.add(mpf(1) / 2, I(q2[0])), I(q1[0]))
            return [lsg, g1], [a.scale(a.mul(I(y[0]), lsg), mpf(1) / 2), a.scale(a.sub(mpf(1) / 2, I(q2[0])), mpf(1) / 2)]
        raise ValueError(kind)

    # ---- float64 ELBO terms of one point (self.fmt must be F64): inputs are float64 numbers
    def negbin_logconst(self, y, r):  # K = 1 + 8 + 1 + 8 + 8 + 2
        a = self.a
        return a.sub(a.sub(a.lgamma(a.add(y, r)), a.lgamma(a.add(y, 1))), a.lgamma(r))

    def expected_logtilt(self, y, q1, q2, mu, var):
        a, p, kind = self.a, self.p, self.kind
        I = a.inp
        half = mpf(1) / 2
        if kind == "bernoulli":  # K = 4 + 2 + 1 + 1 + 1 + 1
            th = self.pg_mean(X(mpf(1)), I(q1[0]))
            m = I(mu[0])
            s = m if y[0] != 0 else a.neg(m)
            return a.add(-LOGTWO, a.scale(a.sub(s, a.mul(self.sm(m, I(var[0])), th)), half))
        if kind == "negbin":
            r, yy, m = I(p["r"]), I(y[0]), I(mu[0])
            th = self.pg_mean(a.add(yy, r), I(q1[0]))
            t = a.sub(self.negbin_logconst(yy, r), a.mul(a.add(yy, r), LOGTWO))
            return a.add(t, a.scale(a.sub(a.mul(m, a.sub(yy, r)), a.mul(self.sm(m, I(var[0])), th)), half))
        if kind == "studentt":
            th = a.div(a.scale(a.add(I(p["nu"]), 1), half), I(q1[0]))
            d = a.sub(I(mu[0]), I(y[0]))
            t = a.add(-half * LOG2PI, a.scale(a.log(th), half))
            t = a.sub(t, a.mul(a.mul(a.scale(d, half), d), th))  # 0.5 * d * d * th
            return a.sub(t, a.scale(a.mul(I(var[0]), th), half))
        if kind in ("cat", "catbij"):
            L = p["L"]
            sp = X(mpf(0))
            for k in range(L):
                sp = a.add(sp, I(q2[k]))
            p0 = a.sub(1, sp)
            s1, s2 = X(mpf(0)), X(mpf(0))
            for k in range(L):
                yk, nbar = I(y[k]), a.div(I(q2[k]), p0)
                w = self.pg_mean(a.add(yk, nbar), I(q1[k]))
                m = I(mu[k])
                s1 = a.add(s1, a.add(yk, nbar))
                s2 = a.add(s2, a.scale(a.sub(a.mul(a.sub(yk, nbar), m), a.mul(self.sm(m, I(var[k])), w)), half))
            return a.add(a.mul(a.neg(s1), LOGTWO), s2)
        if kind == "poisson":
            yy, nbar, m = I(y[0]), I(q2[0]), I(mu[0])
            w = self.pg_mean(a.add(yy, nbar), I(q1[0]))
            t = a.mul(a.neg(a.add(yy, nbar)), LOGTWO)
            t = a.add(t, a.scale(a.sub(a.mul(a.sub(yy, nbar), m), a.mul(self.sm(m, I(var[0])), w)), half))
            t = a.add(t, a.mul(yy, a.log(I(p["lam"]))))
            return a.sub(t, a.lgamma(a.add(yy, 1)))
        if kind == "laplace":
            t = a.sub(a.sub(a.lgamma(X(half)), a.scale(a.log(X(mp.pi)), half)), a.log(a.scale(I(p["beta"]), 2)))
            return a.sub(t, a.mul(self.sm_y(I(mu[0]), I(var[0]), I(y[0])), I(q1[0])))
        raise ValueError(kind)

    def pois_kl(self, lq, lp):
        a = self.a
        if lq.v > 0:
            return a.add(a.sub(a.mul(lq, a.sub(a.log(lq), a.log(lp))), lq), lp)
        return lp

    def aux_kl(self, y, q1, q2):
        a, p, kind = self.a, self.p, self.kind
        I = a.inp
        half = mpf(1) / 2
        if kind == "bernoulli":
            return self.pg_kl(X(mpf(1)), I(q1[0]))
        if kind == "negbin":
            return self.pg_kl(a.add(I(y[0]), I(p["r"])), I(q1[0]))
        if kind == "studentt":
            nu, sg = I(p["nu"]), I(p["sigma"])
            ap, thp = a.scale(a.add(nu, 1), half), a.div(1, I(q1[0]))
            aq = a.scale(nu, half)
            thq = a.div(a.mul(sg, sg), aq)
            t = a.sub(a.mul(a.sub(ap, aq), self.digamma(ap)), a.lgamma(ap))
            t = a.add(t, a.lgamma(aq))
            t = a.add(t, a.mul(aq, a.sub(a.log(thq), a.log(thp))))
            return a.add(t, a.div(a.mul(ap, a.sub(thp, thq)), thq))
        if kind == "poisson":
            lq = I(q2[0])
            return a.add(self.pg_kl(a.add(I(y[0]), lq), I(q1[0])), self.pois_kl(lq, I(p["lam"])))
        if kind == "laplace":
            b2 = a.scale(I(p["beta"]), 2)
            lam = a.div(1, a.mul(b2, b2))
            t = a.sub(a.scale(a.log(a.scale(lam, 2)), half), a.scale(a.log(X(2 * mp.pi)), half))
            t = a.sub(t, a.scale(a.log(lam), half))
            t = a.add(t, a.lgamma(X(half)))
            return a.add(t, a.div(lam, I(q1[0])))
        if kind == "catbij":
            L = p["L"]
            sp = X(mpf(0))
            for k in range(L):
                sp = a.add(sp, I(q2[k]))
            p0 = a.sub(1, sp)
            pp = a.div(1, I(p["sum_theta"]))
            p0p = a.sub(1, a.mul(L, pp))
            s, acc = X(mpf(0)), X(mpf(0))
            for k in range(L):
                qk = I(q2[k])
                acc = a.add(acc, self.pg_kl(a.add(I(y[k]), a.div(qk, p0)), I(q1[k])))
                s = a.add(s, a.mul(qk, a.sub(a.log(qk), a.log(pp))))
            return a.add(a.sub(a.add(acc, a.log(p0)), a.log(p0p)), a.div(s, p0))
        raise ValueError(kind)

    def expected_aug_loglik(self, y, q1, q2, mu, var):
        a, p, kind = self.a, self.p, self.kind
        I = a.inp
        half = mpf(1) / 2
        if kind != "hetero":  # generic.jl:52-54: a PLUS
            return a.add(self.expected_logtilt(y, q1, q2, mu, var), self.aux_kl(y, q1, q2))
        lam, yy = I(p["lam"]), I(y[0])
        mf, vf, g, vg = I(mu[0]), I(var[0]), I(mu[1]), I(var[1])
        tn = I(q2[0])
        tw = self.pg_mean(a.add(half, tn), I(q1[0]))
        d = a.sub(yy, mf)
        lp = a.mul(a.scale(lam, half), a.add(a.mul(d, d), vf))
        klp = self.pois_kl(tn, lp)
        t = a.scale(a.add(a.log(lam), a.log(X(2 / mp.pi))), half)
        t = a.sub(t, a.mul(a.add(half, tn), LOGTWO))
        t = a.add(t, a.scale(a.sub(a.mul(a.sub(half, tn), g), a.mul(a.add(a.mul(g, g), vg), tw)), half))
        t = a.add(t, self.pg_kl(a.add(half, tn), I(q1[0])))
        return a.add(t, klp)


# ======================================================================================================================= the numpy model
VARIANTS = ("tanh_from_exp", "no_c0_branch", "cutoffs_of_other_type", "sech_from_exp", "p0_reversed", "studentt_quirk_fixed",
            "pg_kl_terms_swapped", "elbo_shortcut_c_for_half_c", "zero_log_zero_is_zero")


class Model:
    """The rules in numpy scalars of the element type, in the device's order of operations (no fused multiply-add: numpy has none)."""

    def __init__(self, kind, fmt, params, variant=None):
        assert variant is None or variant in VARIANTS
        self.kind, self.fmt, self.T, self.V = kind, fmt, fmt.T, variant
        self.p = params_T(kind, params, fmt)
        self._raw = params

    def tanh(self, x):
        T = self.T
        if self.V == "tanh_from_exp":  # of c = 2 x
            e = np.exp(-(x + x))
            return (T(1) - e) / (T(1) + e)
        return np.tanh(x)

    def pg_mean(self, b, c, T=None):
        T = T or self.T
        b, c = T(b), T(c)
        if c == T(0) and self.V != "no_c0_branch":
            return b / T(4)
        return b / (T(2) * c) * self.tanh(c / T(2))

    def ael(self, m, c):
        T, f = self.T, self.fmt
        if self.V == "cutoffs_of_other_type":
            f = F64 if f is F32 else F32
        if m < T(f.lo):
            return T(0)
        if m > T(f.hi):
            return T(1)
        x = c / T(2)
        sech = T(2) / (np.exp(x) + np.exp(-x)) if self.V == "sech_from_exp" else T(1) / np.cosh(x)
        return np.exp(m / T(2)) * sech / T(2)

    def aux_posterior(self, y, mu, var):
        T, p, kind = self.T, self.p, self.kind
        mu, var = [T(v) for v in mu], [T(v) for v in var]
        y = [T(v) for v in y]
        with np.errstate(all="ignore"):
            if kind in ("bernoulli", "negbin"):
                return [np.sqrt(mu[0] * mu[0] + var[0])], [], None
            if kind == "studentt":
                nu, sg = p["nu"], p["sigma"]
                q = nu * (sg * sg) if self.V == "studentt_quirk_fixed" else nu / (sg * sg)
                return [(q + ((mu[0] - y[0]) * (mu[0] - y[0]) + var[0])) / T(2)], [], None
            if kind in ("cat", "catbij"):
                o1, o2 = [], []
                for k in range(p["L"]):
                    c = np.sqrt(mu[k] * mu[k] + var[k])
                    o1.append(c)
                    o2.append(self.ael(-mu[k], c) / p["den"])
                return o1, o2, None
            if kind == "poisson":
                c = np.sqrt(mu[0] * mu[0] + var[0])
                return [c], [p["lam"] * self.ael(-mu[0], c)], None
            if kind == "laplace":
                return [T(1) / (T(2) * p["beta"] * np.sqrt((mu[0] - y[0]) * (mu[0] - y[0]) + var[0]))], [], None
            o3 = ((mu[0] - y[0]) * (mu[0] - y[0]) + var[0]) / T(2)
            c = np.sqrt(mu[1] * mu[1] + var[1])
            return [c], [p["lam"] * self.ael(-mu[1], c) * o3], o3

    def expected_pp(self, y, q1, q2, mu_g=None):
        T, p, kind = self.T, self.p, self.kind
        y, q1, q2 = [T(v) for v in y], [T(v) for v in q1], [T(v) for v in q2]
        with np.errstate(all="ignore"):
            if kind == "bernoulli":
                return [self.pg_mean(T(1), q1[0])], [T(0.5) if y[0] != T(0) else T(-0.5)]
            if kind == "negbin":
                return [self.pg_mean(y[0] + p["r"], q1[0])], [(y[0] - p["r"]) / T(2)]
            if kind == "studentt":
                w = ((p["nu"] + T(1)) / T(2)) * (T(1) / q1[0])
                return [w], [w * y[0]]
            if kind in ("cat", "catbij"):
                sp = T(0)
                for k in (reversed(range(p["L"])) if self.V == "p0_reversed" else range(p["L"])):
                    sp = sp + q2[k]
                p0 = T(1) - sp
                g, b = [], []
                for k in range(p["L"]):
                    nbar = T(1) / p0 * q2[k]
                    g.append(self.pg_mean(y[k] + nbar, q1[k]))
                    b.append((y[k] - nbar) / T(2))
                return g, b
            if kind == "poisson":
                return [self.pg_mean(y[0] + q2[0], q1[0])], [(y[0] - q2[0]) / T(2)]
            if kind == "laplace":
                return [T(2) * q1[0]], [T(2) * q1[0] * y[0]]
            lsg = p["lam"] * (T(1) - self.ael(-T(mu_g), q1[0]))
            return [lsg, self.pg_mean(T(0.5) + q2[0], q1[0])], [y[0] * lsg / T(2), (T(0.5) - q2[0]) / T(2)]

    # ---- float64 ELBO terms (the model must be built with F64)
    @staticmethod
    def logcosh(x):
        ax = np.abs(x)
        return ax + np.log1p(np.exp(-2.0 * ax)) - np.float64(0.69314718055994530942)

    def pg_kl(self, b, c):
        om = self.pg_mean(b, c)
        if self.V == "pg_kl_terms_swapped":
            return c * c * om / 2.0 - b * self.logcosh(c / 2.0)
        return b * self.logcosh(c / 2.0) - c * c * om / 2.0

    @staticmethod
    def lgamma(x):
        import math

        x = float(x)
        return np.float64(math.lgamma(x)) if x > 0 and x == x and x != float("inf") else np.float64(np.inf if x == x else np.nan)

    def negbin_logconst(self, y, r):
        return self.lgamma(y + r) - self.lgamma(y + 1.0) - self.lgamma(r)

    @staticmethod
    def digamma(x):
        r = np.float64(0.0)
        while x < 6.0:
            r = r - 1.0 / x
            x = x + 1.0
        f = 1.0 / (x * x)
        return r + np.log(x) - 0.5 / x - f * (1.0 / 12.0 - f * (1.0 / 120.0 - f * (1.0 / 252.0 - f * (1.0 / 240.0 - f / 132.0))))

    def expected_logtilt(self, y, q1, q2, mu, var):
        D = np.float64
        p, kind = self.p, self.kind
        y, q1, q2, mu, var = ([D(v) for v in s] for s in (y, q1, q2, mu, var))
        L2, L2PI = D(0.69314718055994530942), D(1.83787706640934548356)
        with np.errstate(all="ignore"):
            if kind == "bernoulli":
                s = D(1.0) if y[0] != 0.0 else D(-1.0)
                th = self.pg_mean(1.0, q1[0])
                return -L2 + (s * mu[0] - (mu[0] * mu[0] + var[0]) * th) / 2.0
            if kind == "negbin":
                r, yy = p["r"], y[0]
                th = self.pg_mean(yy + r, q1[0])
                return self.negbin_logconst(yy, r) - (yy + r) * L2 + (mu[0] * (yy - r) - (mu[0] * mu[0] + var[0]) * th) / 2.0
            if kind == "studentt":
                th = ((p["nu"] + 1.0) / 2.0) / q1[0]
                d = mu[0] - y[0]
                return -0.5 * L2PI + 0.5 * np.log(th) - 0.5 * d * d * th - var[0] * th / 2.0
            if kind in ("cat", "catbij"):
                sp = D(0.0)
                for k in range(p["L"]):
                    sp = sp + q2[k]
                p0, s1, s2 = 1.0 - sp, D(0.0), D(0.0)
                for k in range(p["L"]):
                    nbar = q2[k] / p0
                    w = self.pg_mean(y[k] + nbar, q1[k])
                    s1 = s1 + (y[k] + nbar)
                    s2 = s2 + ((y[k] - nbar) * mu[k] - (mu[k] * mu[k] + var[k]) * w) / 2.0
                return -s1 * L2 + s2
            if kind == "poisson":
                yy, nbar = y[0], q2[0]
                w = self.pg_mean(yy + nbar, q1[0])
                return (-(yy + nbar) * L2 + ((yy - nbar) * mu[0] - (mu[0] * mu[0] + var[0]) * w) / 2.0 + yy * np.log(p["lam"])
                        - self.lgamma(yy + 1.0))
            if kind == "laplace":
                return (self.lgamma(0.5) - 0.5 * np.log(D(np.pi)) - np.log(2.0 * p["beta"])
                        - ((mu[0] - y[0]) * (mu[0] - y[0]) + var[0]) * q1[0])
        raise ValueError(kind)

    @staticmethod
    def pois_kl(lq, lp):
        return lq * (np.log(lq) - np.log(lp)) - lq + lp if lq > 0 else lp

    def aux_kl(self, y, q1, q2):
        D = np.float64
        p, kind = self.p, self.kind
        y, q1, q2 = ([D(v) for v in s] for s in (y, q1, q2))
        with np.errstate(all="ignore"):
            if kind == "bernoulli":
                return self.pg_kl(D(1.0), q1[0])
            if kind == "negbin":
                return self.pg_kl(y[0] + p["r"], q1[0])
            if kind == "studentt":
                nu, sg = p["nu"], p["sigma"]
                ap, thp = (nu + 1.0) / 2.0, 1.0 / q1[0]
                aq, thq = nu / 2.0, sg * sg / (nu / 2.0)
                return ((ap - aq) * self.digamma(ap) - self.lgamma(ap) + self.lgamma(aq) + aq * (np.log(thq) - np.log(thp))
                        + ap * (thp - thq) / thq)
            if kind == "poisson":
                return self.pg_kl(y[0] + q2[0], q1[0]) + self.pois_kl(q2[0], p["lam"])
            if kind == "laplace":
                lam = 1.0 / ((2.0 * p["beta"]) * (2.0 * p["beta"]))
                return np.log(2.0 * lam) / 2.0 - np.log(2.0 * D(np.pi)) / 2.0 - np.log(lam) / 2.0 + self.lgamma(0.5) + lam / q1[0]
            if kind == "catbij":
                L = p["L"]
                sp = D(0.0)
                for k in range(L):
                    sp = sp + q2[k]
                p0 = 1.0 - sp
                pp = 1.0 / p["sum_theta"]
                p0p = 1.0 - L * pp
                s, acc = D(0.0), D(0.0)
                for k in range(L):
                    acc = acc + self.pg_kl(y[k] + q2[k] / p0, q1[k])
                    if self.V == "zero_log_zero_is_zero" and q2[k] == 0.0:
                        continue
                    s = s + q2[k] * (np.log(q2[k]) - np.log(pp))
                return acc + np.log(p0) - np.log(p0p) + s / p0
        raise ValueError(kind)

    def expected_aug_loglik(self, y, q1, q2, mu, var):
        D = np.float64
        if self.kind != "hetero":
            return self.expected_logtilt(y, q1, q2, mu, var) + self.aux_kl(y, q1, q2)
        lam, yy = self.p["lam"], D(y[0])
        mf, vf, g, vg = D(mu[0]), D(var[0]), D(mu[1]), D(var[1])
        tn, c = D(q2[0]), D(q1[0])
        with np.errstate(all="ignore"):
            tw = self.pg_mean(0.5 + tn, c)
            lp = lam / 2.0 * ((yy - mf) * (yy - mf) + vf)
            klp = self.pois_kl(tn, lp)
            return (0.5 * (np.log(lam) + np.log(2.0 / D(np.pi))) - (0.5 + tn) * D(0.69314718055994530942)
                    + ((0.5 - tn) * g - (g * g + vg) * tw) / 2.0 + self.pg_kl(0.5 + tn, c) + klp)

    def elbo_point(self, y, mu32, var32):
        """elbo_point of the sweep's kernel: expected_logtilt - aux_kl in float64 from float32 marginals; Bernoulli and negative
        binomial by the one-logcosh shortcut."""
        D = np.float64
        mu, var = [D(np.float32(v)) for v in mu32], [D(np.float32(v)) for v in var32]
        y = [D(np.float32(v)) for v in y] if self.kind in REAL_Y else [D(v) for v in y]
        q1, q2, _ = Model(self.kind, F64, self._raw).aux_posterior(y, mu, var)
        with np.errstate(all="ignore"):
            if self.kind in ("bernoulli", "negbin"):
                c = q1[0] if self.V == "elbo_shortcut_c_for_half_c" else q1[0] / 2.0
                if self.kind == "bernoulli":
                    return -D(0.69314718055994530942) + (mu[0] if y[0] != 0.0 else -mu[0]) / 2.0 - self.logcosh(c)
                r, yy = self.p["r"], y[0]
                return self.negbin_logconst(yy, r) - (yy + r) * D(0.69314718055994530942) + mu[0] * (yy - r) / 2.0 - (yy + r) * self.logcosh(c)
            return self.expected_logtilt(y, q1, q2, mu, var) - self.aux_kl(y, q1, q2)


def model(kind, fmt, params, variant=None):
    return Model(kind, fmt, params, variant)


# ======================================================================================================================= the edge grid
LOGTHETA = {"cat": [0.1, -0.2, 0.3, 0.0], "catbij": [0.1, -0.2, 0.3, 0.0, -0.1], "catbij1": [0.2, -0.3]}


def _c_pairs():
    """(name, mu, var) whose c = sqrt(mu^2 + var) walks 0, tiny, typical, either side of the float32 cosh overflow, huge."""
    return [("c=0", 0.0, 0.0), ("mu=denormal", DENORM32, 0.0), ("c=1e-20", 1e-20, 0.0), ("c=1e-4", 6e-5, 6.4e-9), ("c=1", -0.6, 0.64),
            ("c=20", 12.0, 256.0), ("c=176", 0.0, 176.0 ** 2), ("c=178", 0.0, 178.0 ** 2), ("c=180", 0.0, 180.0 ** 2),
            ("c=1500", 0.0, 1500.0 ** 2), ("c=3e4", 0.0, 9e8)]


def _cut_pairs(fmt):
    """-mu at each logistic cut-off of the type and one ulp either side."""
    T = fmt.T
    out = []
    for nm, cut in (("lo", fmt.lo), ("hi", fmt.hi)):
        for tag, v in (("-1ulp", np.nextafter(cut, T(-np.inf))), ("", cut), ("+1ulp", np.nextafter(cut, T(np.inf)))):
            out.append((f"-mu={nm}cut{tag}", float(-v), 1.0))
    return out


def grid(kind, fmt):
    """The named points (name, y, mu, var, params) of one likelihood for one element type; y, mu, var are tuples."""
    P = []
    add = lambda name, y, mu, var, **pr: P.append(Point(name, tuple(y), tuple(float(fmt.T(m)) for m in mu), tuple(float(fmt.T(v)) for v in var), pr))
    cp = _c_pairs()
    if kind == "bernoulli":
        for i, (nm, m, v) in enumerate(cp):
            add(nm, [i & 1], [m], [v])
        add("typical", [1], [0.3], [0.9])
    elif kind == "negbin":
        for nm, m, v in cp:
            add(nm, [3], [m], [v], r=15.0)
        for r in (15.0, 5.5, 1e-3):
            for yy in (0, 1, 2 ** 24 + 1, 2 ** 31 - 1):
                add(f"y={yy},r={r}", [yy], [0.7], [0.5], r=r)
            add(f"y=0,c=0,r={r}", [0], [0.0], [0.0], r=r)
    elif kind == "poisson":
        for nm, m, v in cp + _cut_pairs(fmt):
            add(nm, [3], [m], [v], lam=10.0)
        for lam in (10.0, 1e-6, 1e6):
            for yy in (0, 1, 2 ** 24 + 1, 2 ** 31 - 1):
                add(f"y={yy},lam={lam}", [yy], [0.7], [0.5], lam=lam)
            add(f"y=0,mu=-30,lam={lam}", [0], [-30.0], [1.0], lam=lam)
    elif kind == "studentt":
        for nu, sg in ((3.5, 2.0), (1e-3, 2.0), (1e6, 2.0), (3.5, 1e-8), (1e6, 1e-8)):
            for res in (0.0, 1e-20, 1e3, 1e18, 1e19, 2e19):
                if (nu, sg) != (3.5, 2.0) and res in (1e-20, 1e18):
                    continue
                add(f"res={res:g},nu={nu:g},sg={sg:g}", [0.0], [res], [0.0], nu=nu, sigma=sg)
        for v in (1.0, 1e-30):
            add(f"var={v:g}", [0.7], [-0.4], [v], nu=3.5, sigma=2.0)
        add("y=-1e19,mu=1e19", [-1e19], [1e19], [1.0], nu=3.5, sigma=2.0)
    elif kind == "laplace":
        for beta in (1.3, 1e-8, 1e6):
            for v in (0.0, DENORM32, 1e-30, 1.0):
                add(f"mu=y,var={v:g},beta={beta:g}", [0.7], [0.7], [v], beta=beta)
            for res in (1e-20, 1.0, 1e19, 2e19):
                add(f"res={res:g},beta={beta:g}", [0.0], [res], [0.0], beta=beta)
        add("mu=y=0,var=0", [0.0], [0.0], [0.0], beta=1.3)
    elif kind == "hetero":
        for nm, m, v in cp + _cut_pairs(fmt):
            add("g:" + nm, [0.3], [-0.2, m], [0.5, v], lam=5.0)
        for res, vf in ((0.0, 0.0), (0.0, 1.0), (1e19, 0.0), (2e19, 0.0), (1e-20, 0.0)):
            for nm, m, v in (("c=0", 0.0, 0.0), ("c=1", -0.6, 0.64), ("c=20", -12.0, 256.0)):
                add(f"y-mu={res:g},varf={vf:g},g:{nm}", [res], [0.0, m], [vf, v], lam=5.0)
        for lam in (1e-6, 1e6):
            add(f"lam={lam:g}", [0.3], [-0.2, 0.4], [0.5, 0.3], lam=lam)
    elif kind in ("cat", "catbij"):
        lt = LOGTHETA[kind]
        L = 4
        onehot = lambda c: [1 if k == c else 0 for k in range(L)]
        typ_m, typ_v = [0.4, -1.1, 0.2, 2.0], [0.3, 1.2, 0.05, 0.7]
        for i, (nm, m, v) in enumerate(cp + _cut_pairs(fmt)):
            add("k0:" + nm, onehot(i % (L + 1)), [m] + typ_m[1:], [v] + typ_v[1:], logtheta=lt)
        for m in (-4.0, -10.0, -17.0, -40.0):
            add(f"all={m:g}", onehot(1), [m] * L, [0.0] * L, logtheta=lt)
            add(f"all={m:g},var=1", onehot(4), [m] * L, [1.0] * L, logtheta=lt)
        add("one=+800,var=2e6", onehot(2), [800.0] + typ_m[1:], [2e6] + typ_v[1:], logtheta=lt)
        add("all=+800,var=2e6", onehot(0), [800.0] * L, [2e6] * L, logtheta=lt)
        add("mixed", onehot(3), [-17.0, 17.0, -3.0, 3.0], [0.0, 1.0, 4.0, 0.25], logtheta=lt)
        add("mixed-big", onehot(0), [-40.0, 40.0, -110.0, 110.0], [1.0] * L, logtheta=lt)
        add("typical", onehot(1), typ_m, typ_v, logtheta=lt)
        if kind == "catbij":
            l1 = LOGTHETA["catbij1"]
            for i, (nm, m, v) in enumerate(cp + _cut_pairs(fmt)):
                add("L1:" + nm, [i & 1], [m], [v], logtheta=l1)
            for m in (-4.0, -40.0, 800.0):
                add(f"L1:mu={m:g}", [1], [m], [2e6 if m > 0 else 0.0], logtheta=l1)
    else:
        raise ValueError(kind)
    return P


def direct_q1_points(kind, fmt):
    """q1 values that aux_posterior! cannot produce in the type (c = sqrt(.) is 0 or >= 3.7e-23 in float32) but the operator
    agpl_expected_potential_precision accepts: the smallest denormal, the smallest normal, and 1e-30."""
    T = fmt.T
    tiny = float(np.finfo(T).tiny)
    den = float(np.nextafter(T(0), T(1)))
    return [("q1=denormal", den), ("q1=tiny", tiny), ("q1=1e-30", float(T(1e-30))), ("q1=0", 0.0)]


def direct_q_points(kind, fmt):
    """[(name, y, q1, q2, mu_g)] fed to expected potential / precision as they stand, beside the q1, q2 that aux_posterior! gives on
    the grid: the tiny c of ``direct_q1_points`` for the kinds whose precision is a PG mean, and for the categorical kinds a q2 whose
    sum rounds to 1 in the rule's order of summation and to 1 - 2u in the reverse order."""
    T = fmt.T
    out = []
    if kind in ("bernoulli", "negbin", "poisson", "hetero"):
        for nm, c in direct_q1_points(kind, fmt):
            out.append((nm, [1], [c], [0.75] if kind in HAS_Q2 else [], 0.3 if kind == "hetero" else None))
    if kind in ("cat", "catbij"):
        e = float(np.finfo(T).eps) / 8  # u / 4
        big = float(np.nextafter(T(1), T(0)))  # 1 - u
        for nm, c in direct_q1_points(kind, fmt):
            out.append((nm, [0, 1, 0, 0], [c, 1.0, 2.0, 3.0], [0.1, 0.2, 0.3, 0.15], None))
        out.append(("sum q2 rounds to 1 forwards only", [0, 0, 1, 0], [1.0, 2.0, 0.5, 3.0], [e, e, e, big], None))
        out.append(("p0 = u", [1, 0, 0, 0], [1.0, 2.0, 0.5, 3.0], [0.25, 0.25, 0.25, float(np.nextafter(T(0.25), T(0)))], None))
    return out


def groups(points):
    """The points grouped by their parameters (one launch each): [(params, [points])]."""
    out = []
    for p in points:
        key = repr(sorted(p.params.items()))
        for k, pr, lst in out:
            if k == key:
                lst.append(p)
                break
        else:
            out.append((key, p.params, [p]))
    return [(pr, lst) for _, pr, lst in out]


def cast_y(kind, y, fmt):
    """y of one point as the rule of element type T reads it: (T)y."""
    return [float(fmt.T(v)) for v in y]


# ======================================================================================================================= comparison
def verdict(got, ref, model_value):
    """(ok, ratio, why) of one output: ``got`` a float of the device (or a variant), ``ref`` an Out, ``model_value`` the model's float.
    Resolved: the class must be the mpmath value's and |got - v| <= bar.  Unresolved: the class must be the model's, the sign of a
    finite value included; a finite unresolved value is held to no bar (exact arithmetic does not know it: its amplification is
    unbounded there, which is what unresolved means)."""
    cg = classify(got)
    if ref.unresolved:
        cm = classify(model_value)
        # (a value finite in the type although exact arithmetic could not promise it is held to the model's sign, no bar)
        return cg == cm, 0.0 if cg == cm else float("inf"), f"unresolved, model {cm}, got {cg}"
    want = "neg" if ref.v < 0 else "fin"
    if cg not in ("fin", "neg"):
        return False, float("inf"), f"resolved {want}, got {cg}"
    err = abs(mpf(float(got)) - ref.v)
    if ref.bar == 0:
        return err == 0, 0.0 if err == 0 else float("inf"), "exact"
    ratio = float(err / ref.bar)
    return ratio <= 1.0, ratio, f"|got - ref| / bar = {ratio:.3g}"


# ======================================================================================================================= evaluation
Rec = namedtuple("Rec", "point out got ref model")


class ModelImpl:
    """The numpy model (or one of its wrong variants) behind the interface the device is driven through in the GPU module."""

    def __init__(self, variant=None):
        self.variant = variant

    def aux_posterior(self, kind, fmt, params, ys, mus, vars_):
        m = model(kind, fmt, params, self.variant)
        return [m.aux_posterior(y, mu, var) for y, mu, var in zip(ys, mus, vars_)]

    def expected_pp(self, kind, fmt, params, ys, q1s, q2s, mugs):
        m = model(kind, fmt, params, self.variant)
        return [m.expected_pp(y, q1, q2, g) for y, q1, q2, g in zip(ys, q1s, q2s, mugs)]

    def elbo_term(self, kind, which, params, y, q1, q2, mu, var):
        m = model(kind, F64, params, self.variant)
        fn = {"elt": m.expected_logtilt, "kl": lambda y, q1, q2, mu, var: m.aux_kl(y, q1, q2), "eal": m.expected_aug_loglik}[which]
        return float(fn(y, q1, q2, mu, var))


def _fl(seq):
    return [float(v) for v in seq]


def evaluate_operators(kind, fmt, impl):
    """aux_posterior! on the grid and expected potential / precision on the q1, q2 that ``impl`` itself returned (they are exact
    numbers of the type: each operator is held to the bar of its own arithmetic), then on the direct q points.  -> [Rec]."""
    base = ModelImpl()
    recs = []
    for params, pts in groups(grid(kind, fmt)):
        ref = Ref(kind, fmt, params)
        ys = [list(p.y) for p in pts]  # (as observed: the implementation casts them, the reference takes the cast value)
        mus, vs = [p.mu for p in pts], [p.var for p in pts]
        got = impl.aux_posterior(kind, fmt, params, ys, mus, vs)
        mod = base.aux_posterior(kind, fmt, params, ys, mus, vs)
        for p, y, g, m in zip(pts, ys, got, mod):
            r1, r2, r3 = ref.aux_posterior(cast_y(kind, y, fmt), p.mu, p.var)
            for k in range(len(r1)):
                recs.append(Rec(p.name, f"out1[{k}]", float(g[0][k]), _out(fmt, r1[k]), float(m[0][k])))
            for k in range(len(r2)):
                recs.append(Rec(p.name, f"out2[{k}]", float(g[1][k]), _out(fmt, r2[k]), float(m[1][k])))
            if r3 is not None:
                recs.append(Rec(p.name, "out3", float(g[2]), _out(fmt, r3), float(m[2])))
        q1s, q2s = [_fl(g[0]) for g in got], [_fl(g[1]) for g in got]
        mugs = [p.mu[1] if kind == "hetero" else None for p in pts]
        names = [p.name for p in pts]
        if params == grid(kind, fmt)[0].params:
            for nm, y, q1, q2, mg in direct_q_points(kind, fmt):
                names.append(nm), ys.append(list(y)), q1s.append(q1), q2s.append(q2), mugs.append(mg)
        got = impl.expected_pp(kind, fmt, params, ys, q1s, q2s, mugs)
        mod = base.expected_pp(kind, fmt, params, ys, q1s, q2s, mugs)
        for nm, y, q1, q2, mg, g, m in zip(names, ys, q1s, q2s, mugs, got, mod):
            rg, rb = ref.expected_pp(cast_y(kind, y, fmt), q1, q2, mg)
            for k in range(len(rg)):
                recs.append(Rec(nm, f"gamma[{k}]", float(g[0][k]), _out(fmt, rg[k]), float(m[0][k])))
                recs.append(Rec(nm, f"beta[{k}]", float(g[1][k]), _out(fmt, rb[k]), float(m[1][k])))
    return recs


ELBO_TERMS = {"bernoulli": ("elt", "kl", "eal"), "negbin": ("elt", "kl", "eal"), "studentt": ("elt", "kl", "eal"), "cat": ("elt",),
              "catbij": ("elt", "kl", "eal"), "poisson": ("elt", "kl", "eal"), "laplace": ("elt", "kl", "eal"), "hetero": ("eal",)}


def elbo_inputs(kind):
    """[(point name, params, y, q1, q2, mu, var)] of the float64 ELBO terms: the float64 grid with q1, q2 of the float64 MODEL's
    aux_posterior! (inputs of the terms, exact float64 numbers); points whose q1 / q2 are not finite are left to the operators."""
    out = []
    for params, pts in groups(grid(kind, F64)):
        m = model(kind, F64, params)
        for p in pts:
            y = cast_y(kind, p.y, F64)
            q1, q2, _ = m.aux_posterior(y, p.mu, p.var)
            q1, q2 = _fl(q1), _fl(q2)
            if np.all(np.isfinite(q1)) and np.all(np.isfinite(q2)):
                out.append((p.name, params, y, q1, q2, list(p.mu), list(p.var)))
    return out


def elbo_reference(kind, which, params, y, q1, q2, mu, var):
    ref = Ref(kind, F64, params)
    x = {"elt": ref.expected_logtilt, "kl": lambda y, q1, q2, mu, var: ref.aux_kl(y, q1, q2), "eal": ref.expected_aug_loglik}[which](y, q1, q2, mu, var)
    return _out(F64, x)


def evaluate_elbo(kind, impl):
    base = ModelImpl()
    recs = []
    for nm, params, y, q1, q2, mu, var in elbo_inputs(kind):
        for which in ELBO_TERMS[kind]:
            recs.append(Rec(nm, which, impl.elbo_term(kind, which, params, y, q1, q2, mu, var),
                            elbo_reference(kind, which, params, y, q1, q2, mu, var), base.elbo_term(kind, which, params, y, q1, q2, mu, var)))
    return recs


def evaluate_elbo_point(kind, variant=None):
    """elbo_point of the sweep's kernel (float64 from float32 marginals; the one-logcosh shortcut for Bernoulli and the negative
    binomial) against expected_logtilt - aux_kl of the exact rules from the same float32 marginals."""
    recs = []
    for params, pts in groups(grid(kind, F32)):
        ref, a = Ref(kind, F64, params), Ar(F64)
        for p in pts:
            y = cast_y(kind, p.y, F32)
            r1, r2, _ = ref.aux_posterior(y, p.mu, p.var)
            x = a.sub(ref.expected_logtilt(y, r1, r2, p.mu, p.var), ref.aux_kl(y, r1, r2))
            recs.append(Rec(p.name, "elbo_point", float(model(kind, F64, params, variant).elbo_point(y, p.mu, p.var)), _out(F64, x),
                            float(model(kind, F64, params).elbo_point(y, p.mu, p.var))))
    return recs


def summarize(recs):
    """(worst ratio over the resolved outputs, [failures as text], number of unresolved outputs)."""
    worst, fails, unres = 0.0, [], 0
    for r in recs:
        ok, ratio, why = verdict(r.got, r.ref, r.model)
        unres += r.ref.unresolved
        if ok:
            worst = max(worst, ratio)
        else:
            fails.append(f"{r.point} / {r.out}: {why} (got {r.got!r}, reference {mp.nstr(r.ref.v, 12)}, bar {mp.nstr(r.ref.bar, 3)}, K {r.ref.K})")
    return worst, fails, unres


def plan_points(kind, params, pts):
    """The float32 grid points of one parameter set as a plan can hold them: every latent of a point shares the features and the
    residual, so the point gets ONE var over its latents -- that of the latent the point is about (latent 0 of a categorical point,
    the second latent of a heteroscedastic one) -- plus the 2^-20 of the one feature column.  -> ([Point] whose gamma and beta the
    model expects finite and gamma >= 0, [Point] of the other classes); the Points carry the common var BEFORE the 2^-20."""
    m = model(kind, F32, params)
    ok, other = [], []
    for p in pts:
        cv = p.var[1] if kind == "hetero" else p.var[0]
        q = Point(p.name, p.y, p.mu, (cv,) * len(p.var), p.params)
        var = [float(np.float32(np.float32(cv) + np.float32(2.0 ** -20)))] * len(p.var)
        q1, q2, _ = m.aux_posterior(p.y, p.mu, var)
        g, b = m.expected_pp(p.y, q1, q2, p.mu[1] if kind == "hetero" else None)
        fine = all(np.isfinite(float(v)) and float(v) >= 0 for v in g) and all(np.isfinite(float(v)) for v in b)
        (ok if fine else other).append(q)
    return ok, other
