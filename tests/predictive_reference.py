"""Float64 references of the predictive distribution p(y* | q(f)) for tests/test_gpu_predictive.py (and tools/predictive_twin.py):
the likelihoods p(y | f) of oracle/agpl_oracle.c written out in numpy / scipy, integrated against q(f) = N(mu, s^2) with
scipy.integrate.quad (epsrel 1e-13, split at mu and at y or the mode of the integrand), and the random cases of the test box.
No GPU, no library code: nothing here imports the package."""
import numpy as np
from scipy import integrate, optimize, special

KINDS = ("bernoulli", "negbinomial", "studentt", "poisson", "laplace", "heterogauss")
LOG_SQRT_2PI = 0.5 * np.log(2.0 * np.pi)


def logsig(x):
    return -np.logaddexp(0.0, -x)


def loglik(kind, p, y, f, g=None):
    """log p(y | f) (heteroscedastic: log p(y | f, g)); p = the likelihood's parameters as the descriptor carries them."""
    if kind == "bernoulli":
        return logsig((2.0 * y - 1.0) * f)
    if kind == "negbinomial":
        r = p[0]
        return special.gammaln(y + r) - special.gammaln(y + 1.0) - special.gammaln(r) + y * logsig(f) + r * logsig(-f)
    if kind == "poisson":
        lam = p[0]
        return y * (np.log(lam) + logsig(f)) - lam * special.expit(f) - special.gammaln(y + 1.0)
    if kind == "studentt":
        nu, sg = p[0], p[1]
        z = (y - f) / sg
        return (special.gammaln(0.5 * (nu + 1.0)) - special.gammaln(0.5 * nu) - 0.5 * np.log(nu * np.pi) - np.log(sg)
                - 0.5 * (nu + 1.0) * np.log1p(z * z / nu))
    if kind == "laplace":
        return -np.abs(y - f) / p[0] - np.log(2.0 * p[0])
    if kind == "heterogauss":
        v = (1.0 + np.exp(-g)) / p[0]  # 1 / (lambda sigma(g))
        return -0.5 * np.log(2.0 * np.pi * v) - 0.5 * (y - f) ** 2 / v
    raise ValueError(kind)


def _quad_pieces(fun, edges):
    tot, err = 0.0, 0.0
    for lo, hi in zip(edges[:-1], edges[1:]):
        if hi > lo:
            v, e = integrate.quad(fun, lo, hi, epsabs=0.0, epsrel=1e-13, limit=400)
            tot += v
            err += e
    return tot, err


def _gauss_quad(logfun, mu, s, extra=(), width=16.0):
    """integral of exp(logfun(f)) N(f; mu, s^2) df over mu +- width s (widened to the mode of the integrand +- width s), split at mu
    and at `extra`; the integrand is scaled by its maximum so that tiny densities keep their relative accuracy.
    Returns (log of the integral, quad's error estimate relative to the integral)."""
    h = lambda f: logfun(f) - 0.5 * ((f - mu) / s) ** 2
    a, b = mu - width * s, mu + width * s
    grid = np.linspace(mu - 40.0 * s, mu + 40.0 * s, 801)
    g0 = grid[np.argmax(h(grid))]
    r = optimize.minimize_scalar(lambda f: -h(f), bounds=(g0 - 0.1 * s, g0 + 0.1 * s), method="bounded", options={"xatol": 1e-12})
    mode = float(r.x)
    a, b = min(a, mode - width * s), max(b, mode + width * s)
    hm = float(h(mode))
    pts = sorted({mu, mode, *[e for e in extra if a < e < b]})
    tot, err = _quad_pieces(lambda f: np.exp(h(f) - hm), [a] + pts + [b])
    return hm + np.log(tot) - np.log(s) - LOG_SQRT_2PI, err / tot


def ref_logp(kind, p, y, mu, var):
    """(log int p(y | f) q(f) df, relative error estimate) of one point; mu, var scalars (heteroscedastic: pairs (f, g))."""
    if kind == "heterogauss":
        (mf, mg), (vf, vg) = mu, var
        lam = p[0]

        def lg(g):  # f integrated analytically: y | g ~ N(mu_f, s_f^2 + 1 / (lambda sigma(g)))
            v = vf + (1.0 + np.exp(-g)) / lam
            return -0.5 * np.log(2.0 * np.pi * v) - 0.5 * (y - mf) ** 2 / v

        if vg == 0.0:
            return float(lg(mg)), 0.0
        return _gauss_quad(lg, mg, np.sqrt(vg))
    if var == 0.0:
        return float(loglik(kind, p, y, mu)), 0.0
    extra = (y,) if kind in ("studentt", "laplace") else ()
    return _gauss_quad(lambda f: loglik(kind, p, y, f), mu, np.sqrt(var), extra)


def _gauss_mean(fun, mu, s):
    pts = [mu] + ([0.0] if abs(mu) < 16.0 * s else [])
    g = lambda f: fun(f) * np.exp(-0.5 * ((f - mu) / s) ** 2)
    tot, err = _quad_pieces(g, sorted({mu - 16.0 * s, *pts, mu + 16.0 * s}))
    c = s * np.sqrt(2.0 * np.pi)
    return tot / c, err / c


def ref_moments(kind, p, mu, var):
    """(E y, Var y) of the predictive distribution of one point."""
    if kind == "heterogauss":
        (mf, mg), (vf, vg) = mu, var
        return mf, vf + (1.0 + np.exp(-mg + 0.5 * vg)) / p[0]
    s = np.sqrt(var)
    if kind in ("bernoulli", "poisson"):
        if var == 0.0:
            e1, e2 = special.expit(mu), special.expit(mu) ** 2
        else:
            e1 = _gauss_mean(special.expit, mu, s)[0]
            e2 = _gauss_mean(lambda f: special.expit(f) ** 2, mu, s)[0]
        if kind == "bernoulli":
            return e1, e1 * (1.0 - e1)
        lam = p[0]
        return lam * e1, lam * e1 + lam * lam * (e2 - e1 * e1)
    if kind == "negbinomial":
        r = p[0]
        m1, m2 = np.exp(mu + 0.5 * var), np.exp(2.0 * mu + 2.0 * var)
        return r * m1, r * (m1 + m2) + r * r * (m2 - m1 * m1)
    if kind == "studentt":
        nu, sg = p[0], p[1]
        return (mu if nu > 1.0 else np.nan), (var + sg * sg * nu / (nu - 2.0) if nu > 2.0 else np.inf)
    if kind == "laplace":
        return mu, var + 2.0 * p[0] ** 2
    raise ValueError(kind)


def box_cases(kind, n, seed):
    """The parameter box of the accuracy test: a list of (p, y [n], mu, var) groups, one per parameter setting, that together hold
    n points.  mu uniform in [-4, 4], s log-uniform in [0.05, 2]."""
    rng = np.random.default_rng(seed)
    settings = {
        "bernoulli": [(0.0,)], "negbinomial": [(1.0,), (15.0,)], "poisson": [(3.0,)],
        "studentt": [(nu, sg) for nu in (1.5, 3.0, 10.0) for sg in (0.1, 0.5, 2.0)],
        "laplace": [(0.1,), (1.0,)], "heterogauss": [(2.0,)],
    }[kind]
    sizes = [n // len(settings) + (1 if i < n % len(settings) else 0) for i in range(len(settings))]
    out = []
    for p, m in zip(settings, sizes):
        L = 2 if kind == "heterogauss" else 1
        mu = rng.uniform(-4.0, 4.0, size=(m, L))
        s = np.exp(rng.uniform(np.log(0.05), np.log(2.0), size=(m, L)))
        var = s * s
        if kind == "bernoulli":
            y = rng.integers(0, 2, size=m).astype(np.uint8)
        elif kind == "negbinomial":
            y = rng.integers(0, 61, size=m).astype(np.int32)
        elif kind == "poisson":
            y = rng.integers(0, 13, size=m).astype(np.int32)
        elif kind == "studentt":
            y = mu[:, 0] + 3.0 * rng.standard_normal(m) * np.sqrt(var[:, 0] + p[1] ** 2)
        elif kind == "laplace":  # the same spread with the Laplace variance 2 beta^2
            y = mu[:, 0] + 3.0 * rng.standard_normal(m) * np.sqrt(var[:, 0] + 2.0 * p[0] ** 2)
        else:  # up to ~3 sigma N(0, 1) of the predictive standard deviation at the mean of g
            y = mu[:, 0] + 3.0 * rng.standard_normal(m) * np.sqrt(var[:, 0] + (1.0 + np.exp(-mu[:, 1])) / p[0])
        if L == 1:
            mu, var = mu[:, 0], var[:, 0]
        out.append((p, y, mu, var))
    return out


def reference(kind, p, y, mu, var):
    """(mean, var, logp, rel_err) arrays for one group."""
    n = len(y)
    mean, v, lp, er = (np.empty(n) for _ in range(4))
    for i in range(n):
        mean[i], v[i] = ref_moments(kind, p, mu[i], var[i])
        lp[i], er[i] = ref_logp(kind, p, float(y[i]), mu[i], var[i])
    return mean, v, lp, er


def categorical_reference(logtheta, bijective, mu, var, nodes=48):
    """Class probabilities E[theta_k sigma(f_k) / sum_j theta_j sigma(f_j)] under independent q(f_k) = N(mu_k, var_k): a tensor
    Gauss-Hermite rule with `nodes` per latent.  mu, var: [n, L]; returns [n, K]."""
    t, w = np.polynomial.hermite.hermgauss(nodes)
    w = w / np.sqrt(np.pi)
    n, L = mu.shape
    theta = np.exp(np.asarray(logtheta, dtype=np.float64))
    K = L + 1 if bijective else L
    out = np.zeros((n, K))
    idx = np.stack(np.meshgrid(*[np.arange(nodes)] * L, indexing="ij"), axis=-1).reshape(-1, L)
    wt = np.prod(w[idx], axis=1)
    for i in range(n):
        f = mu[i] + np.sqrt(2.0 * var[i]) * t[idx]  # [nodes^L, L]
        u = theta[:L] * special.expit(f)
        if bijective:
            u = np.concatenate([u, np.full((u.shape[0], 1), 0.5 * theta[L])], axis=1)
        out[i] = wt @ (u / u.sum(axis=1, keepdims=True))
    return out
