"""numpy twin of the quadrature rules of csrc/agpl_predictive.hip, measured against the scipy.integrate.quad
references of tests/predictive_reference.py over the parameter box of tests/test_gpu_predictive.py.  CPU only.

    python tools/predictive_twin.py [points per kind] [seed]

prints, per likelihood, the worst |log density - reference| and the worst relative error of the predictive mean / variance."""
import os
import sys

import numpy as np
from scipy import special

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
import predictive_reference as R  # noqa: E402

NEWTON, GRID, SPAN, ST_POINTS, MAXHALF, RECENTRE = 12, 65, 8.0, 96, 1024, 32


def count_terms(f, A, B, Lam):
    """lp = A log sigma(f) + B log sigma(-f) - Lam sigma(f) and its first two derivatives (the three logistic likelihoods)."""
    e = np.exp(-abs(f))
    sp = 1.0 / (1.0 + e)
    sig, sgc = (sp, e * sp) if f >= 0 else (e * sp, sp)
    l1p = np.log1p(e)
    lsp, lsn = (-l1p, -f - l1p) if f >= 0 else (f - l1p, -l1p)
    ssc = sig * sgc
    return A * lsp + B * lsn - Lam * sig, A * sgc - B * sig - Lam * ssc, -(A + B) * ssc - Lam * ssc * (1.0 - 2.0 * sig)


def hetero_terms(g, vf, lam, d2):
    """lg = -log(v) / 2 - d2 / (2 v), v = vf + (1 + exp(-g)) / lam, and its first two derivatives in g."""
    e = np.exp(-g) / lam
    v = vf + 1.0 / lam + e
    q, r = -0.5 * e / v, d2 / v - 1.0  # v' = -e, v'' = e
    return -0.5 * np.log(v) - 0.5 * d2 / v, q * r, (0.5 * e / v - 0.5 * e * e / (v * v)) * r + q * d2 * e / (v * v)


def agh_logp(A, B, Lam, c0, mu, var, count_terms=count_terms):
    if var == 0.0:
        return c0 + count_terms(mu, A, B, Lam)[0]
    s = np.sqrt(var)
    iv = 1.0 / var
    d = 2.0 * SPAN * s / (GRID - 1)
    best, m, c = -np.inf, mu, mu
    for _ in range(RECENTRE):  # a maximum on the grid's edge moves the grid there
        kb = (GRID - 1) // 2
        for k in range(GRID):
            f = c + (k - (GRID - 1) // 2) * d
            h = count_terms(f, A, B, Lam)[0] - 0.5 * (f - mu) ** 2 * iv
            if h > best:
                best, m, kb = h, f, k
        if kb not in (0, GRID - 1):
            break
        c = m
    for _ in range(NEWTON):
        _, d1, d2 = count_terms(m, A, B, Lam)
        h1, h2 = d1 - (m - mu) * iv, d2 - iv
        if h2 >= 0.0:
            break
        m += min(max(-h1 / h2, -d), d)
    lp, _, d2 = count_terms(m, A, B, Lam)
    h2 = d2 - iv
    w = s if h2 >= 0.0 else min(s, 1.0 / np.sqrt(-h2))
    hm = lp - 0.5 * (m - mu) ** 2 * iv
    # trapezoid rule centred on the mode: spacing fine enough for the peak (w / 2) and for the logistic's poles (s / 4), +- 8 s
    dl = min(0.5 * w, 0.25 * s)
    nh = min(int(np.ceil(SPAN * s / dl)), MAXHALF)
    acc = 0.0
    for j in range(-nh, nh + 1):
        f = m + j * dl
        acc += np.exp(count_terms(f, A, B, Lam)[0] - 0.5 * (f - mu) ** 2 * iv - hm)
    return c0 + hm + np.log(acc) + np.log(dl) - np.log(s) - R.LOG_SQRT_2PI


def studentt_logp(nu, sg, y, mu, var):
    if var == 0.0:
        return float(R.loglik("studentt", (nu, sg), y, mu))
    a, c = 0.5 * nu, 0.5 * nu * sg * sg
    lo, hi = np.log(a) - 12.0 / np.sqrt(a) - 6.0, np.log(a) + np.log1p(40.0 / a)
    h = (hi - lo) / (ST_POINTS - 1)
    d2 = (y - mu) ** 2
    li = np.empty(ST_POINTS)
    for k in range(ST_POINTS):
        t = lo + k * h
        x = np.exp(t)
        v = var + c / x
        li[k] = a * t - x - 0.5 * np.log(v) - 0.5 * d2 / v
    li[0] -= np.log(2.0)
    li[-1] -= np.log(2.0)
    m = li.max()
    return m + np.log(np.exp(li - m).sum()) + np.log(h) - special.gammaln(a) - R.LOG_SQRT_2PI


def laplace_logp(beta, y, mu, var):
    d = y - mu
    if var == 0.0:
        return -abs(d) / beta - np.log(2.0 * beta)
    s = np.sqrt(var)
    q = 0.5 * d * d / var

    def term(z, e):  # log(exp(e) erfc(z)), e = z^2 - q
        return -q + np.log(special.erfcx(z)) if z > 0 else e + np.log(special.erfc(z))

    z1, z2 = (s / beta - d / s) * np.sqrt(0.5), (s / beta + d / s) * np.sqrt(0.5)
    e0 = 0.5 * var / (beta * beta)
    return np.logaddexp(term(z1, e0 - d / beta), term(z2, e0 + d / beta)) - np.log(4.0 * beta)


def hetero_logp(lam, y, mu, var):
    (mf, mg), (vf, vg) = mu, var
    return agh_logp(vf, lam, (y - mf) ** 2, -R.LOG_SQRT_2PI, mg, vg, count_terms=hetero_terms)


def gh_sigma_moments(mu, var):
    """E sigma(f), E sigma(f)^2: the trapezoid rule on the seed grid (mu +- 8 s, spacing s / 4)."""
    x = (np.arange(GRID) - (GRID - 1) // 2) * (2.0 * SPAN / (GRID - 1))
    wt = np.exp(-0.5 * x * x)
    sg = special.expit(mu + np.sqrt(var) * x)
    return (wt * sg).sum() / wt.sum(), (wt * sg * sg).sum() / wt.sum()


def twin(kind, p, y, mu, var):
    if kind == "bernoulli":
        lp = agh_logp(float(y), 1.0 - float(y), 0.0, 0.0, mu, var)
        e1, _ = gh_sigma_moments(mu, var)
        return e1, e1 * (1.0 - e1), lp
    if kind == "negbinomial":
        r = p[0]
        c0 = special.gammaln(y + r) - special.gammaln(y + 1.0) - special.gammaln(r)
        return (*R.ref_moments(kind, p, mu, var), agh_logp(float(y), r, 0.0, c0, mu, var))
    if kind == "poisson":
        lam = p[0]
        c0 = y * np.log(lam) - special.gammaln(y + 1.0)
        e1, e2 = gh_sigma_moments(mu, var)
        return lam * e1, lam * e1 + lam * lam * (e2 - e1 * e1), agh_logp(float(y), 0.0, lam, c0, mu, var)
    if kind == "studentt":
        return (*R.ref_moments(kind, p, mu, var), studentt_logp(p[0], p[1], y, mu, var))
    if kind == "laplace":
        return (*R.ref_moments(kind, p, mu, var), laplace_logp(p[0], y, mu, var))
    return (*R.ref_moments(kind, p, mu, var), hetero_logp(p[0], y, mu, var))


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 600
    seed = int(sys.argv[2]) if len(sys.argv) > 2 else 7
    for kind in R.KINDS:
        worst, wm, wv, skipped, arg = 0.0, 0.0, 0.0, 0, None
        for p, y, mu, var in R.box_cases(kind, n, seed):
            mean, v, lp, er = R.reference(kind, p, y, mu, var)
            for i in range(len(y)):
                if er[i] > 1e-9:
                    skipped += 1
                    continue
                tm, tv, tl = twin(kind, p, y[i], mu[i], var[i])
                if abs(tl - lp[i]) > worst:
                    worst, arg = abs(tl - lp[i]), (p, y[i], mu[i], np.sqrt(var[i]))
                if np.isfinite(mean[i]):
                    wm = max(wm, abs(tm - mean[i]) / (abs(mean[i]) + 1e-4))
                if np.isfinite(v[i]):
                    wv = max(wv, abs(tv - v[i]) / abs(v[i]))
        print(f"{kind:12s} logp {worst:.2e}  mean {wm:.2e}  var {wv:.2e}  skipped {skipped}  worst at {arg}")


if __name__ == "__main__":
    main()
