"""numpy twin of the per-point rules of csrc/agpl_likgrad.hip: E_q log p(y | f) and its derivatives for the
logarithms of the likelihood's parameters, the same rules in float64 without contraction (numpy adds the nodes in another order).
CPU only, nothing imports the package.

    python tools/likgrad_twin.py        prints, per likelihood, the twin's worst figure over tests/likgrad_domain.py in units of the bar

The constants below are plain numbers; tests/test_likgrad_domain_cpu.py holds them against the .hip source.  twin() returns
(ell, dell [P], tq [1 + P]): tq[k] is the sum of |coefficient x expectation| over the terms of output k that went through a
quadrature rule.  EVALS is the number of integrand evaluations (nodes) of the last twin() call; VARIANT names one deliberately wrong
rule (tests only, None = the kernel's): "parent_wide" is the rule of the commit before the sinh branch."""
import math

import numpy as np
from scipy import special

MAXHALF, SPAN = 2048, 8.0
SINH_STEP = 0.19634954084936207  # pi / 16: the largest spacing in x of the sinh rule
SINH_DENSITY, SINH_PAD = 0.5, 4.0  # spacing SINH_DENSITY / (|d| / s + SINH_PAD) where that is smaller
SINH_MAX = 1024  # intervals of the sinh rule, at most
LN2 = 0.69314718055994530942
LOG_SQRT_2PI = 0.91893853320467274178
SQRT_2_OVER_PI = 0.79788456080286535588

VARIANTS = ("parent_wide", "centre_half", "nb_swap", "no_half_over_nu", "nu_for_nu_plus_1", "spacing_half", "no_lambda")
VARIANT = None
EVALS = 0


def make_rule(s, a):
    """(spacing, nodes on each side of mu, whether the node limit widened the spacing)."""
    h = (0.5 if VARIANT == "spacing_half" else 0.25) * min(s, a)
    want = math.ceil(SPAN * s / h)
    if want > MAXHALF:
        return SPAN * s / MAXHALF, MAXHALF, True
    return h, int(want), False


def _centre(w, j):
    if VARIANT == "centre_half":
        w = np.where(j == 0, 0.5 * w, w)
    return w


def logistic_at(f):
    f = np.asarray(f, dtype=np.float64)
    e = np.exp(-np.abs(f))
    sp, l1p = 1.0 / (1.0 + e), np.log1p(e)
    pos = f >= 0.0
    return np.where(pos, -l1p, f - l1p), np.where(pos, -f - l1p, -l1p), np.where(pos, sp, e * sp)


def logistic_expectations(mu, var):
    """(E log sigma(f), E log sigma(-f), E sigma(f))."""
    global EVALS
    if var == 0.0:
        EVALS += 1
        return tuple(float(v) for v in logistic_at(mu))
    s = math.sqrt(var)
    h, nh, _ = make_rule(s, math.pi)
    hs = h / s
    j = np.arange(-nh, nh + 1)
    EVALS += len(j)
    x = j.astype(np.float64) * hs
    w = _centre(np.exp(-0.5 * x * x), j)
    lsp, lsn, sig = logistic_at(mu + j.astype(np.float64) * h)
    a0 = w.sum()
    return float((w * lsp).sum() / a0), float((w * lsn).sum() / a0), float((w * sig).sum() / a0)


def studentt_expectations(nu, sg, y, mu, var):
    """(E log1p(u), E u / (1 + u)), u = (y - f)^2 / (nu sg^2)."""
    global EVALS
    a2, d = nu * sg * sg, y - mu
    if var == 0.0:
        EVALS += 1
        u = d * d / a2
        return math.log1p(u), u / (1.0 + u)
    s = math.sqrt(var)
    a = math.sqrt(a2)
    h, nh, capped = make_rule(s, a)
    if capped and abs(d) < SPAN * s and VARIANT != "parent_wide":
        # y - f = a sinh x: log1p(u) = 2 log cosh x, u / (1 + u) = tanh^2 x, weight N(a sinh x; d, s^2) cosh x
        ia, isd = 1.0 / a, 1.0 / s
        hx = min(SINH_STEP, SINH_DENSITY / (abs(d) * isd + SINH_PAD))
        xlo, xhi = math.asinh((d - SPAN * s) * ia), math.asinh((d + SPAN * s) * ia)
        if xhi - xlo > hx * SINH_MAX:
            hx = (xhi - xlo) / SINH_MAX
        if not math.isfinite(hx):  # 16 s / a overflows: no rule
            return float("nan"), float("nan")
        j = np.arange(math.ceil(xlo / hx), math.floor(xhi / hx) + 1)
        EVALS += len(j)
        x = j.astype(np.float64) * hx
        ax = np.abs(x)
        e = np.exp(ax)
        ie = 1.0 / e
        sh, ch = np.copysign(0.5 * (e - ie), x), 0.5 * (e + ie)
        q = (d - a * sh) * isd
        w = _centre(np.exp(-0.5 * q * q) * ch, j)
        th = sh / ch
        a0 = w.sum()
        return float((w * (2.0 * (ax + np.log1p(ie * ie) - LN2))).sum() / a0), float((w * (th * th)).sum() / a0)
    hs, ia2 = h / s, 1.0 / a2
    j = np.arange(-nh, nh + 1)
    EVALS += len(j)
    jf = j.astype(np.float64)
    x = jf * hs
    w = _centre(np.exp(-0.5 * x * x), j)
    t = d - jf * h
    u = t * t * ia2
    a0 = w.sum()
    return float((w * np.log1p(u)).sum() / a0), float((w * (u / (1.0 + u))).sum() / a0)


def expected_abs(d, var):
    if var == 0.0:
        return abs(d)
    s = math.sqrt(var)
    return s * SQRT_2_OVER_PI * math.exp(-0.5 * d * d / var) + d * math.erf(d / s * math.sqrt(0.5))


def _bad(mu, var):
    return not (math.isfinite(mu) and math.isfinite(var) and var >= 0.0)


def twin(kind, p, y, mu, var):
    """(ell, dell [P], tq [1 + P]) of one point; the heteroscedastic kind takes mu = (mu_f, mu_g), var = (var_f, var_g)."""
    global EVALS
    EVALS = 0
    nan = float("nan")
    P = {"bernoulli": 0, "studentt": 2}.get(kind, 1)
    none = (nan, [nan] * P, [0.0] * (1 + P))
    p0 = p[0]
    with np.errstate(all="ignore"):
        if kind == "heterogauss":
            if _bad(mu[0], var[0]) or _bad(mu[1], var[1]):
                return none
        elif _bad(mu, var):
            return none
        if kind in ("studentt", "laplace", "heterogauss") and not math.isfinite(y):
            return (nan if math.isnan(y) else -math.inf, [nan] * P, [0.0] * (1 + P))
        if kind == "bernoulli":
            lsp, lsn, _ = logistic_expectations(mu, var)
            ell = lsp if y else lsn
            return ell, [], [abs(ell)]
        if kind == "negbinomial":
            y = float(y)
            if y < 0.0:
                return (-math.inf, [nan], [0.0, 0.0])
            lsp, lsn, _ = logistic_expectations(mu, var)
            if VARIANT == "nb_swap":
                lsp, lsn = lsn, lsp
            ell = special.gammaln(y + p0) - special.gammaln(y + 1.0) - special.gammaln(p0) + y * lsp + p0 * lsn
            d0 = p0 * (special.digamma(y + p0) - special.digamma(p0) + lsn)
            return float(ell), [float(d0)], [abs(y * lsp) + abs(p0 * lsn), abs(p0 * lsn)]
        if kind == "poisson":
            y = float(y)
            if y < 0.0:
                return (-math.inf, [nan], [0.0, 0.0])
            lsp, _, sig = logistic_expectations(mu, var)
            ell = y * (math.log(p0) + lsp) - p0 * sig - special.gammaln(y + 1.0)
            d0 = y - (sig if VARIANT == "no_lambda" else p0 * sig)
            return float(ell), [float(d0)], [abs(y * lsp) + abs(p0 * sig), abs(p0 * sig)]
        if kind == "studentt":
            nu, sg = p
            elog, efrac = studentt_expectations(nu, sg, y, mu, var)
            c0 = special.gammaln(0.5 * (nu + 1.0)) - special.gammaln(0.5 * nu) - 0.5 * math.log(nu * math.pi) - math.log(sg)
            c1 = 0.5 * special.digamma(0.5 * (nu + 1.0)) - 0.5 * special.digamma(0.5 * nu) - (0.0 if VARIANT == "no_half_over_nu" else 0.5 / nu)
            ell = c0 - 0.5 * (nu + 1.0) * elog
            d0 = nu * (c1 - 0.5 * elog + 0.5 * (nu + 1.0) * efrac / nu)
            d1 = -1.0 + ((nu if VARIANT == "nu_for_nu_plus_1" else nu + 1.0)) * efrac
            tq = [0.5 * (nu + 1.0) * elog, 0.5 * nu * elog + 0.5 * (nu + 1.0) * efrac, (nu + 1.0) * efrac]
            return float(ell), [float(d0), float(d1)], tq
        if kind == "laplace":
            ea = expected_abs(y - mu, var) / p0
            return -ea - math.log(2.0 * p0), [-1.0 + ea], [0.0, 0.0]
        (mf, mg), (vf, vg) = mu, var
        d = y - mf
        lsp, _, sig = logistic_expectations(mg, vg)
        q = 0.5 * p0 * sig * (d * d + vf)
        return 0.5 * math.log(p0) - LOG_SQRT_2PI + 0.5 * lsp - q, [0.5 - q], [abs(0.5 * lsp) + abs(q), abs(q)]


if __name__ == "__main__":
    import os
    import sys

    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
    import likgrad_domain as D
    import likgrad_domain_reference as Q

    for kind in D.KINDS:
        worst, most = (0.0, ""), 0
        for name, p, y, mu, var in D.points(kind):
            ref = Q.reference(kind, p, y, mu, var)
            ell, dell, _ = twin(kind, p, y, mu, var)
            most = max(most, EVALS)
            for got, want, bar in zip([ell] + list(dell), ref.values, Q.bars(ref)):
                if math.isfinite(want):
                    worst = max(worst, (abs(got - want) / bar, name))
        print(f"{kind}: {len(D.points(kind))} points, worst {worst[0]:.3e} of the bar at {worst[1]}, at most {most} nodes")
