"""The supported domain of agpl_predictive_cdf / agpl_predictive_quantile (include/agpl_quantile.h) as named points
per likelihood: plain numbers, no GPU, no package import.  tests/test_quantile_reference_cpu.py proves the float64 reference on every
point (two independent routes), tests/test_gpu_quantile.py runs the device on every point.  Accuracy outside these ranges is not
promised.

GRID[kind] = list of (name, p, mu, var); heteroscedastic: mu = (mu_f, mu_g), var = (var_f, var_g).  Every point is evaluated at the
thresholds mu + k scale(point), k in K (out to 30 predictive scales), and at the probabilities PROBS.  A count point is evaluated at
the integer thresholds of count_thresholds (0, around the likelihood's mean at mu, ten times it, the cap COUNT_CAP = 1e5) and at COUNT_PROBS
wherever the reference's quantile does not exceed the cap (a quantile beyond the cap is not promised)."""
import math

S = (0.0, 1e-6, 0.05, 1.0, 5.0, 20.0)  # sqrt(var): var = 0, and 1e-6 to 20
MU = (0.0, 20.0, -20.0, 3.0)
K = (-30.0, -8.0, -3.0, -1.0, 0.0, 0.5, 2.0, 6.0, 30.0)
PROBS = (1e-4, 0.025, 0.5, 0.9, 1.0 - 1e-4)
KINDS = ("bernoulli", "studentt", "laplace", "heterogauss", "poisson", "negbinomial")
COUNTS = ("poisson", "negbinomial")
COUNT_CAP = 100000
COUNT_PROBS = (1e-4, 0.025, 0.37, 0.9, 1.0 - 1e-4)  # (0.5 sits exactly on a jump's edge where mu = 0 makes the predictive symmetric)


def _n(x):
    return f"{x:g}"


def _bernoulli():
    return [(f"mu{_n(mu)}_s{_n(s)}", (0.0,), mu, s * s) for mu in (0.0, 3.0, -3.0, 10.0, 20.0, -20.0) for s in S]


def _studentt():
    out = []
    params = ((0.5, 1.0), (1.0, 0.01), (1.5, 0.5), (2.0, 100.0), (3.0, 1.0), (10.0, 0.5), (100.0, 2.0), (1e4, 1.0), (0.5, 100.0),
              (1e4, 0.01))
    for i, (nu, sg) in enumerate(params):
        for mu, s in ((MU[i % 4], S[i % 6]), (MU[(i + 1) % 4], S[(i + 3) % 6]), (MU[(i + 2) % 4], S[(i + 4) % 6])):
            out.append((f"nu{_n(nu)}_sg{_n(sg)}_mu{_n(mu)}_s{_n(s)}", (nu, sg), mu, s * s))
    return out


def _laplace():
    out = []
    for i, beta in enumerate((1e-2, 0.1, 1.0, 10.0)):
        for j, s in enumerate(S):
            out.append((f"b{_n(beta)}_mu{_n(MU[(i + j) % 4])}_s{_n(s)}", (beta,), MU[(i + j) % 4], s * s))
    return out


def _heterogauss():
    out = []
    vgs = (0.0, 0.01, 4.0, 25.0)
    for i, lam in enumerate((1e-3, 2.0, 1e3)):
        for j, mg in enumerate((-10.0, -1.0, 5.0, 10.0)):
            for t in (0, 2):
                vg, s, mf = vgs[(i + j + t) % 4], S[(2 * i + j + 3 * t) % 6], MU[(i + j + t) % 4]
                out.append((f"lam{_n(lam)}_mf{_n(mf)}_mg{_n(mg)}_sf{_n(s)}_vg{_n(vg)}", (lam,), (mf, mg), (s * s, vg)))
    return out


def _poisson():
    out = []
    for i, lam in enumerate((1e-3, 3.0, 1e3, 1e5)):
        for j, s in enumerate(S):
            mu = (0.0, 3.0, -3.0, 20.0, -20.0, 1.0)[(i + j) % 6]
            out.append((f"lam{_n(lam)}_mu{_n(mu)}_s{_n(s)}", (lam,), mu, s * s))
    return out


def _negbinomial():
    out = []
    for i, r in enumerate((1e-2, 1.0, 15.0, 1e3)):
        for j, s in enumerate(S):
            mu = (0.0, 3.0, -3.0, 20.0, -20.0, 1.0)[(i + j) % 6]
            out.append((f"r{_n(r)}_mu{_n(mu)}_s{_n(s)}", (r,), mu, s * s))
    return out


def count_mean(kind, p, mu):
    """The likelihood's own mean at f = mu, at most the cap."""
    m = p[0] / (1.0 + math.exp(-mu)) if kind == "poisson" else p[0] * math.exp(min(mu, 50.0))
    return min(m, float(COUNT_CAP))


GRID = {"poisson": _poisson(), "negbinomial": _negbinomial(), "bernoulli": _bernoulli(), "studentt": _studentt(), "laplace": _laplace(), "heterogauss": _heterogauss()}


def scale(kind, p, mu, var):
    """The scale that the thresholds are spaced by: sqrt(var + the likelihood's own scale^2); heteroscedastic: the noise variance at the
    mean of g (the quantile solve brackets from the predictive's variance, exp(-mu_g + var_g / 2), instead)."""
    if kind == "studentt":
        return math.sqrt(var + p[1] * p[1])
    if kind == "laplace":
        return math.sqrt(var + 2.0 * p[0] * p[0])
    if kind == "heterogauss":
        return math.sqrt(var[0] + (1.0 + math.exp(-mu[1])) / p[0])
    raise KeyError(kind)


def thresholds(kind, p, mu, var):
    """The thresholds of one point: y = 0 and 1 for Bernoulli, the location + k scales otherwise."""
    if kind == "bernoulli":
        return [0, 1]
    if kind in COUNTS:
        m = count_mean(kind, p, mu)
        ys = {0, 1, int(m / 2), int(m), int(m) + 1, int(2 * m) + 3, int(10 * m) + 10, COUNT_CAP}
        return sorted(y for y in ys if y <= COUNT_CAP)
    loc = mu[0] if kind == "heterogauss" else mu
    return [loc + k * scale(kind, p, mu, var) for k in K]


def groups(kind):
    """The kind's points by parameter set: [(p, [points])], one device launch each."""
    out = {}
    for pt in GRID[kind]:
        out.setdefault(pt[1], []).append(pt)
    return list(out.items())
