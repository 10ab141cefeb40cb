"""numpy twin of the quadrature rules of csrc/agpl_predictive.hip, measured against the scipy.integrate.quad
references of tests/predictive_reference.py over the parameter box of tests/test_gpu_predictive.py.  CPU only.

    python tools/predictive_twin.py [points per kind] [seed]

prints, per likelihood, the worst |log density - reference| and the worst relative error of the predictive mean / variance.

The constants below are plain numbers; tests/test_predictive_domain_cpu.py holds them against the .hip source.  EVALS counts the
integrand evaluations of the last twin() call; VARIANT names one deliberately wrong rule (tests only, None = the kernel's)."""
import os
import sys

import numpy as np
from scipy import special

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
import predictive_reference as R  # noqa: E402

NEWTON, GRID, SPAN, MAXHALF, RECENTRE = 48, 65, 8.0, 1024, 32
NEWTON_TOL = 1e-3
BRACKET = 64  # doublings of the bracket beside the Poisson candidate, at most
POLE_CAP = 0.5  # largest spacing of a rule whose integrand has poles at distance pi: exp(-2 pi pi / 0.5) = 7e-18
ST_NEWTON, ST_STEP, ST_DROP, ST_MAXHALF = 6, 2.0, 30.0, 1024
ST_POINTS_PARENT = 96  # the fixed rule this one replaced (variant "parent_studentt"; the evaluation budget inside the old box)

VARIANTS = ("parent_studentt", "spacing_s4", "sigma_neg", "no_c0", "centre_half", "no_log_s", "erfc_only")
VARIANT = None
EVALS = 0
MAG = 0.0  # sum of the magnitudes of the terms that the last log density was added up from (without the count's constant)
PARENT_EVALS = 0  # what the rules before the spacing cap and the stopped Newton iteration spent on the same point AT LEAST: 12 Newton
# steps, spacing min(w / 2, s / 4), and as many grids as this rule needs (a grid that does not double moves at least as often)


def count_terms(f, A, B, Lam):
    """lp = A log sigma(f) + B log sigma(-f) - Lam sigma(f) and its first two derivatives (the three logistic likelihoods)."""
    global EVALS
    EVALS += 1
    e = np.exp(-abs(f))
    sp = 1.0 / (1.0 + e)
    sig, sgc = (sp, e * sp) if f >= 0 else (e * sp, sp)
    l1p = np.log1p(e)
    lsp, lsn = (-l1p, -f - l1p) if f >= 0 else (f - l1p, -l1p)
    ssc = sig * sgc
    return A * lsp + B * lsn - Lam * sig, A * sgc - B * sig - Lam * ssc, -(A + B) * ssc - Lam * ssc * (1.0 - 2.0 * sig)


def hetero_terms(g, vf, lam, d2):
    """lg = -log(v) / 2 - d2 / (2 v), v = vf + (1 + exp(-g)) / lam, and its first two derivatives in g."""
    global EVALS
    EVALS += 1
    ilam = 1.0 / lam
    e = np.exp(-g) * ilam
    v = vf + ilam + e
    q, r = -0.5 * e / v, d2 / v - 1.0  # v' = -e, v'' = e
    return -0.5 * np.log(v) - 0.5 * d2 / v, q * r, (0.5 * e / v - 0.5 * e * e / (v * v)) * r + q * d2 * e / (v * v)


def agh_logp(A, B, Lam, c0, mu, var, count_terms=count_terms, cand=None):
    if VARIANT == "no_c0":
        c0 = 0.0
    if var == 0.0:
        return c0 + count_terms(mu, A, B, Lam)[0]
    s = np.sqrt(var)
    iv = 1.0 / var
    d = 2.0 * SPAN * s / (GRID - 1)
    best, m, c = -np.inf, mu, mu
    reps = 0
    for _ in range(RECENTRE):  # a maximum on the grid's edge moves the grid there
        reps += 1
        kb = (GRID - 1) // 2
        for k in range(GRID):
            f = c + (k - (GRID - 1) // 2) * d
            h = count_terms(f, A, B, Lam)[0] - 0.5 * (f - mu) * (f - mu) * iv
            if h > best:
                best, m, kb = h, f, k
        if kb not in (0, GRID - 1):
            break
        c = m
        d *= 2.0  # (the next grid is twice as wide: a mode 500 s from mu is reached in six moves, not in sixty)
    if cand is not None:  # the likelihood's own maximum: where h has a second maximum far from mu, it is there
        hc = count_terms(cand, A, B, Lam)[0] - 0.5 * (cand - mu) * (cand - mu) * iv
        if hc > best:
            best, m = hc, cand
        else:
            cand = None
    lo, hi = m - d, m + d  # the maximum lies between the neighbours of the grid's best point: Newton, or bisection where it leaves them
    if cand is not None:
        # at the candidate lp' = 0, so h' = (mu - cand) / var points to mu: the maximum lies between the candidate and the first point
        # towards mu where h' has changed sign (steps of d, doubled; h' has changed at mu at the latest for this likelihood)
        sgn, step = (1.0 if mu > cand else -1.0), d
        for _ in range(BRACKET):
            t = cand + sgn * step
            _, d1, _ = count_terms(t, A, B, Lam)
            if sgn * (d1 - (t - mu) * iv) <= 0.0:
                break
            step *= 2.0
        lo, hi = min(cand, t), max(cand, t)
    for _ in range(NEWTON):
        _, d1, d2 = count_terms(m, A, B, Lam)
        h1, h2 = d1 - (m - mu) * iv, d2 - iv
        if h1 == 0.0:
            break
        if h1 > 0.0:
            lo = m
        else:
            hi = m
        t = m - h1 / h2 if h2 < 0.0 else lo
        t = t if lo < t < hi else 0.5 * (lo + hi)
        done = h2 < 0.0 and abs(t - m) * np.sqrt(-h2) <= NEWTON_TOL  # the step is a small part of the peak's width
        m = t
        if done:
            break
    lp, _, d2 = count_terms(m, A, B, Lam)
    h2 = d2 - iv
    w = s if h2 >= 0.0 else min(s, 1.0 / np.sqrt(-h2))
    hm = lp - 0.5 * (m - mu) * (m - mu) * iv
    # trapezoid rule centred on the mode: spacing fine enough for the peak (w / 2) and for the poles at distance pi (s / 4 and
    # POLE_CAP, whichever is smaller), +- 8 s; the terms are scaled by the largest so far, so a centre beside the maximum cannot overflow
    dl = min(0.5 * w, 0.25 * s)
    if VARIANT != "spacing_s4":
        dl = min(dl, POLE_CAP)
    nh = int(min(np.ceil(SPAN * s / dl), MAXHALF))
    global PARENT_EVALS
    PARENT_EVALS += GRID * reps + 13 + 2 * int(min(np.ceil(SPAN * s / min(0.5 * w, 0.25 * s)), MAXHALF)) + 1
    mx, acc = hm, 0.0
    for j in range(-nh, nh + 1):
        f = m + j * dl
        e = count_terms(f, A, B, Lam)[0] - 0.5 * (f - mu) * (f - mu) * iv
        if e > mx:
            acc = acc * np.exp(mx - e) + 1.0
            mx = e
        else:
            acc += np.exp(e - mx)
    hm = mx
    global MAG
    MAG = abs(hm) + abs(np.log(acc)) + abs(np.log(dl)) + abs(np.log(s)) + R.LOG_SQRT_2PI
    return c0 + hm + np.log(acc) + np.log(dl) - (0.0 if VARIANT == "no_log_s" else np.log(s)) - R.LOG_SQRT_2PI


def st_terms(t, a, c, var, dd):
    """g(t) = a t - e^t - log(v) / 2 - dd / (2 v), v = var + c e^-t: the log of the Student-t mixture's integrand in t = log x, and
    its first two derivatives."""
    global EVALS
    EVALS += 1
    x = np.exp(t)
    u = c / x
    v = var + u
    return (a * t - x - 0.5 * np.log(v) - 0.5 * dd / v, a - x + 0.5 * u / v - 0.5 * dd * u / (v * v),
            -x - 0.5 * u * var / (v * v) + 0.5 * dd * u * (var - u) / (v * v * v))


def studentt_logp_parent(nu, sg, y, mu, var, end_weight=0.5):
    a, c = 0.5 * nu, 0.5 * nu * sg * sg
    lo, hi = np.log(a) - 12.0 / np.sqrt(a) - 6.0, np.log(a) + np.log1p(40.0 / a)
    h = (hi - lo) / (ST_POINTS_PARENT - 1)
    dd = (y - mu) * (y - mu)
    li = np.array([st_terms(lo + k * h, a, c, var, dd)[0] for k in range(ST_POINTS_PARENT)])
    li[0] += np.log(end_weight)
    li[-1] += np.log(end_weight)
    m = li.max()
    return m + np.log(np.exp(li - m).sum()) + np.log(h) - special.gammaln(a) - R.LOG_SQRT_2PI


def st_newton(t, a, c, var, dd):
    for _ in range(ST_NEWTON):
        _, g1, g2 = st_terms(t, a, c, var, dd)
        if g2 >= 0.0:
            break
        t += min(max(-g1 / g2, -ST_STEP), ST_STEP)
    return t


def studentt_logp(nu, sg, y, mu, var):
    if var == 0.0:
        return float(R.loglik("studentt", (nu, sg), y, mu))
    if VARIANT == "parent_studentt":
        return studentt_logp_parent(nu, sg, y, mu, var)
    a, c = 0.5 * nu, 0.5 * nu * sg * sg
    dd = (y - mu) * (y - mu)
    # two starts: the Gamma density's own mode (the Gaussian factor flat) and the mode where c / x dominates var (the factor is then
    # x^1/2 exp(-dd x / 2 c)); Newton from each, the higher one is the centre
    ta = st_newton(np.log(a), a, c, var, dd)
    tb = st_newton(np.log((a + 0.5) / (1.0 + 0.5 * dd / c)), a, c, var, dd)
    ga, _, ga2 = st_terms(ta, a, c, var, dd)
    gb, _, gb2 = st_terms(tb, a, c, var, dd)
    if gb > ga:
        ta, tb, ga, gb, ga2 = tb, ta, gb, ga, gb2
    w = 1.0 / np.sqrt(-ga2) if ga2 < 0.0 else 1.0
    h = min(0.5 * w, POLE_CAP)
    other = gb > ga - ST_DROP  # the second maximum counts: the march does not stop before it
    mx, tot = ga, (0.5 if VARIANT == "centre_half" else 1.0)
    for side in (1.0, -1.0):
        for j in range(1, ST_MAXHALF + 1):
            t = ta + side * j * h
            li = st_terms(t, a, c, var, dd)[0]
            if li > mx:
                tot = tot * np.exp(mx - li) + 1.0
                mx = li
            else:
                tot += np.exp(li - mx)
            if li < mx - ST_DROP and not (other and side * (tb - t) > 0.0):
                break
    global MAG
    MAG = abs(mx) + abs(np.log(tot)) + abs(np.log(h)) + abs(special.gammaln(a)) + R.LOG_SQRT_2PI
    return mx + np.log(tot) + np.log(h) - special.gammaln(a) - R.LOG_SQRT_2PI


def laplace_logp(beta, y, mu, var):
    d = y - mu
    if var == 0.0:
        return -abs(d) / beta - np.log(2.0 * beta)
    s = np.sqrt(var)
    q = 0.5 * d * d / var

    def term(z, e):  # log(exp(e) erfc(z)), e = z^2 - q
        with np.errstate(all="ignore"):
            return -q + np.log(special.erfcx(z)) if z > 0 and VARIANT != "erfc_only" else e + np.log(special.erfc(z))

    z1, z2 = (s / beta - d / s) * np.sqrt(0.5), (s / beta + d / s) * np.sqrt(0.5)
    e0 = 0.5 * var / (beta * beta)
    t1, t2 = term(z1, e0 - d / beta), term(z2, e0 + d / beta)
    hi, lo = max(t1, t2), min(t1, t2)
    global MAG
    MAG = q + e0 + abs(d) / beta + abs(hi) + abs(np.log(4.0 * beta)) + 1.0
    with np.errstate(all="ignore"):
        return hi + np.log1p(np.exp(lo - hi)) - np.log(4.0 * beta)


def hetero_logp(lam, y, mu, var):
    (mf, mg), (vf, vg) = mu, var
    return agh_logp(vf, lam, (y - mf) * (y - mf), 0.0, mg, vg, count_terms=hetero_terms) - R.LOG_SQRT_2PI


def sigma_moments(mu, var):
    """E sigma(f), E sigma(f)^2: the trapezoid rule over mu +- 8 s, spacing s / 4 and at most POLE_CAP, normalised by its weights."""
    global EVALS
    s = np.sqrt(var)
    nh = (GRID - 1) // 2
    if VARIANT != "spacing_s4":
        nh = int(min(max(float(nh), np.ceil(SPAN * s / POLE_CAP)), float(MAXHALF)))
    global PARENT_EVALS
    EVALS += 2 * nh + 1
    PARENT_EVALS += GRID
    x = np.arange(-nh, nh + 1) * (SPAN / nh)
    wt = np.exp(-0.5 * x * x)
    f = mu + s * x
    sg = special.expit(-f if VARIANT == "sigma_neg" else f)
    return (wt * sg).sum() / wt.sum(), (wt * sg * sg).sum() / wt.sum()


def negbinomial_moments(r, mu, var):
    with np.errstate(over="ignore", invalid="ignore"):
        m1, m2 = np.exp(mu + 0.5 * var), np.exp(2.0 * mu + 2.0 * var)
        return r * m1, (r * (m1 + m2) + r * r * (m2 - m1 * m1) if np.isfinite(m2) else np.inf)


def twin(kind, p, y, mu, var):
    global EVALS, PARENT_EVALS, MAG
    EVALS = PARENT_EVALS = 0
    MAG = 0.0
    if kind == "bernoulli":
        e1 = special.expit(mu) if var == 0.0 else sigma_moments(mu, var)[0]
        lp = agh_logp(float(y), 1.0 - float(y), 0.0, 0.0, mu, var)
        return e1, e1 * (1.0 - e1), lp
    if kind == "negbinomial":
        r = p[0]
        c0 = special.gammaln(y + r) - special.gammaln(y + 1.0) - special.gammaln(r)
        return (*negbinomial_moments(r, mu, var), agh_logp(float(y), r, 0.0, c0, mu, var))
    if kind == "poisson":
        lam = p[0]
        c0 = y * np.log(lam) - special.gammaln(y + 1.0)
        e1, e2 = (special.expit(mu), special.expit(mu) ** 2) if var == 0.0 else sigma_moments(mu, var)
        cand = np.log(y / (lam - y)) if 0.0 < y < lam else None  # sigma(f) = y / lambda
        return lam * e1, lam * e1 + lam * lam * (e2 - e1 * e1), agh_logp(float(y), 0.0, lam, c0, mu, var, cand=cand)
    if kind == "studentt":
        nu, sg = p
        return (mu if nu > 1.0 else np.nan), (var + sg * sg * nu / (nu - 2.0) if nu > 2.0 else np.inf), studentt_logp(nu, sg, y, mu, var)
    if kind == "laplace":
        return mu, var + 2.0 * p[0] * p[0], laplace_logp(p[0], y, mu, var)
    (mf, mg), (vf, vg) = mu, var
    with np.errstate(over="ignore"):
        return mf, vf + (1.0 + np.exp(-mg + 0.5 * vg)) / p[0], hetero_logp(p[0], y, mu, var)


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 600
    seed = int(sys.argv[2]) if len(sys.argv) > 2 else 7
    for kind in R.KINDS:
        worst, wm, wv, skipped, arg, ev = 0.0, 0.0, 0.0, 0, None, 0
        for p, y, mu, var in R.box_cases(kind, n, seed):
            mean, v, lp, er = R.reference(kind, p, y, mu, var)
            for i in range(len(y)):
                if er[i] > 1e-9:
                    skipped += 1
                    continue
                tm, tv, tl = twin(kind, p, y[i], mu[i], var[i])
                ev = max(ev, EVALS)
                if abs(tl - lp[i]) > worst:
                    worst, arg = abs(tl - lp[i]), (p, y[i], mu[i], np.sqrt(var[i]))
                if np.isfinite(mean[i]):
                    wm = max(wm, abs(tm - mean[i]) / (abs(mean[i]) + 1e-4))
                if np.isfinite(v[i]):
                    wv = max(wv, abs(tv - v[i]) / abs(v[i]))
        print(f"{kind:12s} logp {worst:.2e}  mean {wm:.2e}  var {wv:.2e}  evaluations <= {ev}  skipped {skipped}  worst at {arg}")


if __name__ == "__main__":
    main()
