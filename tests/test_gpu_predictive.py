"""agpl_predictive on the device (include/agpl_predictive.h): predictive moments and held-out log densities against float64
integration (tests/predictive_reference.py: scipy.integrate.quad), the edge cases, the deterministic sum, the categorical Monte
Carlo rule against a tensor Gauss-Hermite rule, and the plan / sweep drivers."""
import numpy as np
import pytest

import predictive_reference as R

pytestmark = pytest.mark.gpu

N = 257  # crosses one 256-lane workgroup


@pytest.fixture(scope="module")
def A():
    import agpl_amd

    return agpl_amd


@pytest.fixture(scope="module")
def ctx(A):
    return A.Context(seed=1234)


def _lik(A, kind, p):
    return {"bernoulli": lambda: A.BernoulliLikelihood(), "negbinomial": lambda: A.NegativeBinomialLikelihood(p[0]),
            "studentt": lambda: A.StudentTLikelihood(p[0], p[1]), "poisson": lambda: A.PoissonLikelihood(p[0]),
            "laplace": lambda: A.LaplaceLikelihood(p[0]), "heterogauss": lambda: A.HeteroscedasticGaussianLikelihood(p[0])}[kind]()


def _dev(a):
    import torch

    return torch.as_tensor(np.ascontiguousarray(a)).cuda()


def _run(A, ctx, lik, mu, var, y=None, **kw):
    m, v, lp = A.predictive(lik, (_dev(mu), _dev(var)), None if y is None else _dev(y), ctx=ctx, **kw)
    return m.cpu().numpy(), None if v is None else v.cpu().numpy(), None if lp is None else lp.cpu().numpy()


# every non-categorical likelihood of agpl.h (six kinds; the box holds the negative binomial at r = 1 and r = 15, Student-t at nine
# (nu, sigma), Laplace at two beta).  The bar on log p is per kind: 10 x the worst |twin - reference| of tools/predictive_twin.py over
# 800 points of the box (seed 7): Bernoulli 3.55e-15, NegBinomial 2.13e-11, Student-t 1.03e-7, Poisson 8.96e-12, Laplace 1.07e-14,
# heteroscedastic 1.54e-7.  No point is excluded: the reference's error estimate is asserted for every one.
LOGP_BAR = {"bernoulli": 3.55e-14, "negbinomial": 2.13e-10, "studentt": 1.03e-6, "poisson": 8.96e-11, "laplace": 1.07e-13, "heterogauss": 1.54e-6}


@pytest.mark.parametrize("kind", R.KINDS)
def test_against_float64_integration(A, ctx, kind):
    worst = dict(logp=0.0, mean=0.0, var=0.0, err=0.0)
    total = 0
    for p, y, mu, var in R.box_cases(kind, N, seed=2024):
        mean_r, var_r, lp_r, err = R.reference(kind, p, y, mu, var)
        mean, v, lp = _run(A, ctx, _lik(A, kind, p), mu, var, y)
        total += len(y)
        worst["err"] = max(worst["err"], err.max())
        worst["logp"] = max(worst["logp"], np.abs(lp - lp_r).max())
        fin = np.isfinite(mean_r)
        worst["mean"] = max(worst["mean"], (np.abs(mean - mean_r)[fin] / (1e-5 * np.abs(mean_r[fin]) + 1e-9)).max() if fin.any() else 0)
        finv = np.isfinite(var_r)
        worst["var"] = max(worst["var"], (np.abs(v - var_r)[finv] / (1e-5 * np.abs(var_r[finv]) + 1e-9)).max() if finv.any() else 0)
        assert np.array_equal(np.isnan(mean), np.isnan(mean_r)) and np.array_equal(np.isinf(v), np.isinf(var_r))
    print(f"{kind}: worst |dlogp| {worst['logp']:.3e} (bar {LOGP_BAR[kind]:.3e}), mean / var in units of the bar {worst['mean']:.3e} "
          f"{worst['var']:.3e}, worst error estimate of the reference {worst['err']:.3e}, {total} points")
    assert total == N and worst["err"] <= 1e-9
    assert worst["logp"] <= LOGP_BAR[kind]
    assert worst["mean"] <= 1.0 and worst["var"] <= 1.0  # 1e-5 relative + 1e-9 absolute


def test_zero_variance_is_the_pointwise_likelihood(A, ctx):
    for kind, p in (("bernoulli", (0.0,)), ("negbinomial", (15.0,)), ("studentt", (3.0, 0.5)), ("poisson", (3.0,)),
                    ("laplace", (0.1,)), ("heterogauss", (2.0,))):
        (_, y, mu, var), = [c for c in R.box_cases(kind, N, seed=3) if c[0] == p][:1]
        var = np.zeros_like(var)
        _, _, lp = _run(A, ctx, _lik(A, kind, p), mu, var, y)
        ref = R.loglik(kind, p, y.astype(np.float64), mu[:, 0], mu[:, 1]) if kind == "heterogauss" else R.loglik(kind, p, y.astype(np.float64), mu)
        print(f"{kind}: var = 0, worst |logp - log p(y | mu)| {np.abs(lp - ref).max():.3e}")
        assert np.abs(lp - ref).max() <= 1e-12, kind


def test_far_means_give_finite_log_densities(A, ctx):
    mu = np.array([-40.0, 40.0, -40.0, 40.0])
    var = np.array([1.0, 1.0, 4.0, 0.0025])
    for kind, p, y in (("bernoulli", (0.0,), np.array([1, 0, 0, 1], dtype=np.uint8)),
                       ("negbinomial", (15.0,), np.array([60, 0, 3, 7], dtype=np.int32)),
                       ("poisson", (3.0,), np.array([12, 0, 1, 5], dtype=np.int32))):
        mean, v, lp = _run(A, ctx, _lik(A, kind, p), mu, var, y)
        assert np.isfinite(lp).all() and np.isfinite(mean).all() and np.isfinite(v).all(), (kind, lp)
        # (y + r = 75 at mu = -40, s = 1 puts the integrand's mode 39 s from mu)
        ref = np.array([R.ref_logp(kind, p, float(y[i]), mu[i], var[i])[0] for i in range(4)])
        assert np.abs(lp - ref).max() <= 1e-4, (kind, lp, ref)
    # a negative count has probability zero
    _, _, lp = _run(A, ctx, A.PoissonLikelihood(3.0), mu[:2], var[:2], np.array([-1, 2], dtype=np.int32))
    assert lp[0] == -np.inf and np.isfinite(lp[1])


def test_bad_marginals_give_nan_at_that_point_only(A, ctx):
    (p, y, mu, var), = R.box_cases("bernoulli", N, seed=11)
    lik = A.BernoulliLikelihood()
    good = _run(A, ctx, lik, mu, var, y)
    mu2, var2 = mu.copy(), var.copy()
    var2[3], var2[100], mu2[256], var2[255] = np.nan, -1e-3, np.inf, np.inf
    bad = _run(A, ctx, lik, mu2, var2, y)
    idx = np.array([3, 100, 255, 256])
    rest = np.setdiff1d(np.arange(N), idx)
    for g, b in zip(good, bad):
        assert np.isnan(b[idx]).all()
        assert np.array_equal(g[rest], b[rest])


def test_without_observations_only_the_moments(A, ctx):
    (p, y, mu, var), = R.box_cases("poisson", N, seed=12)
    lik = A.PoissonLikelihood(3.0)
    m0, v0, lp0 = _run(A, ctx, lik, mu, var)
    m1, v1, lp1 = _run(A, ctx, lik, mu, var, y)
    assert lp0 is None and lp1 is not None
    assert np.array_equal(m0, m1) and np.array_equal(v0, v1)
    with pytest.raises(A.ArgumentError):
        A.log_predictive_density(lik, (_dev(mu), _dev(var)), None, ctx=ctx)


def test_bad_nsamples_is_an_argument_error_and_the_context_lives(A, ctx):
    lik = A.CategoricalLikelihood(3)
    mu, var = np.zeros((4, 3)), np.ones((4, 3))
    for ns in (5, (1 << 20) + 1):
        with pytest.raises(A.ArgumentError):
            _run(A, ctx, lik, mu, var, nsamples=ns)
    probs, v, lp = _run(A, ctx, lik, mu, var, nsamples=16)
    assert v is None and lp is None and probs.shape == (4, 3) and np.abs(probs.sum(1) - 1.0).max() <= 1e-12


def test_sum_is_deterministic_and_propagates_nan(A, ctx):
    import torch

    n = 70_001
    rng = np.random.default_rng(21)
    mu, var = _dev(rng.uniform(-4, 4, n)), _dev(np.exp(rng.uniform(np.log(0.05), np.log(2.0), n)) ** 2)
    y = _dev(rng.integers(0, 2, n).astype(np.uint8))
    lik = A.BernoulliLikelihood()
    s1 = A.log_predictive_density(lik, (mu, var), y, ctx=ctx)
    s2 = A.log_predictive_density(lik, (mu, var), y, ctx=ctx)
    assert np.float64(s1).tobytes() == np.float64(s2).tobytes()
    lp = A.predictive(lik, (mu, var), y, ctx=ctx)[2].cpu().numpy()
    ref = float(np.sum(lp, dtype=np.float64))
    assert abs(s1 - ref) <= 1e-12 * abs(ref), (s1, ref)
    var[n - 2] = float("nan")
    assert np.isnan(A.log_predictive_density(lik, (mu, var), y, ctx=ctx))
    torch.cuda.synchronize()


@pytest.mark.parametrize("bijective", [False, True])
def test_categorical_monte_carlo(A, bijective):
    import torch

    n, ns = 64, 16_384
    L, K = (2, 3) if bijective else (3, 3)
    rng = np.random.default_rng(31 + bijective)
    logtheta = rng.normal(size=K) * 0.5
    lik = A.CategoricalLikelihood(logtheta, bijective=bijective)
    mu, var = rng.uniform(-3, 3, (n, L)), np.exp(rng.uniform(np.log(0.05), np.log(2.0), (n, L))) ** 2
    cls = rng.integers(0, K, n)
    y = np.zeros((n, L), dtype=np.uint8)
    for i, c in enumerate(cls):
        if c < L:
            y[i, c] = 1  # class L of the bijective link: the all-zero row
    ref = R.categorical_reference(logtheta, bijective, mu, var)
    ctx = A.Context(seed=99)
    probs, v, lp = _run(A, ctx, lik, mu, var, y, nsamples=ns, sweep=7)
    assert v is None and probs.shape == (n, K)
    print("categorical: worst |dp|", np.abs(probs - ref).max())
    assert np.abs(probs - ref).max() <= 6 * 0.5 / np.sqrt(ns)  # each draw lies in [0, 1]: sd <= 0.5
    assert np.abs(probs.sum(1) - 1.0).max() <= 1e-12
    # the device's log against numpy's of the same float64 probability: each is within one unit in the last place of the result
    want = np.log(probs[np.arange(n), cls])
    assert np.abs(lp - want).max() <= 4 * np.finfo(np.float64).eps * np.maximum(1.0, np.abs(want)).max()
    again = _run(A, ctx, lik, mu, var, y, nsamples=ns, sweep=7)
    assert np.array_equal(probs, again[0]) and np.array_equal(lp, again[2])
    assert not np.array_equal(probs, _run(A, ctx, lik, mu, var, y, nsamples=ns, sweep=8)[0])
    # a shard evaluated alone with its point offset draws what the full call drew for those rows
    ctx.set_point_offset(17)
    part = _run(A, ctx, lik, mu[17:49], var[17:49], y[17:49], nsamples=ns, sweep=7)
    ctx.set_point_offset(0)
    assert np.array_equal(part[0], probs[17:49]) and np.array_equal(part[2], lp[17:49])
    # the device sum of the same call
    tot = A.log_predictive_density(lik, (_dev(mu), _dev(var)), _dev(y), nsamples=ns, sweep=7, ctx=ctx)
    assert abs(tot - lp.sum()) <= 1e-12 * abs(lp.sum())
    torch.cuda.synchronize()


def test_categorical_sixty_four_latents(A, ctx):
    rng = np.random.default_rng(41)
    n, L = 9, 64
    for bij in (False, True):
        lik = A.CategoricalLikelihood(rng.normal(size=L + bij) * 0.3, bijective=bij)
        probs, _, _ = _run(A, ctx, lik, rng.uniform(-2, 2, (n, L)), rng.uniform(0.1, 2.0, (n, L)), nsamples=256)
        assert probs.shape == (n, L + bij) and np.isfinite(probs).all() and (probs > 0).all()
        assert np.abs(probs.sum(1) - 1.0).max() <= 1e-12


def test_on_the_plan(A):
    import torch

    ctx = A.Context(seed=5)
    lik = A.BernoulliLikelihood()
    Nn, M = 10_000, 64
    x, y = A.synth_xy(lik, seed=3, i0=0, n=Nn, ctx=ctx)
    z = torch.linspace(-10, 10, M, dtype=torch.float64, device=x.device)
    cavi = A.SparseCAVI.from_inputs(lik, x, y, z, lengthscale=1.5 * 20.0 / (M - 1), ctx=ctx)  # 1.5 inducing spacings
    cavi.run(10)
    x_s = torch.linspace(-10, 10, 2001, dtype=torch.float64, device=x.device)
    _, y_s = A.synth_xy(lik, seed=4, i0=0, n=2001, ctx=ctx, want_x=False)  # held-out labels
    mu, var = cavi.predict(x_s)
    qf = (mu[0].to(torch.float64), var[0].to(torch.float64))
    want = A.predictive(lik, qf, y_s, ctx=ctx)
    got = cavi.predict_y(x_s, y_s)
    for w, g in zip(want, got):
        assert torch.equal(w, g)
    assert torch.isfinite(got[2]).all() and ((got[0] > 0) & (got[0] < 1)).all()
    total = cavi.heldout_logp(x_s, y_s)
    ref = float(got[2].cpu().numpy().sum(dtype=np.float64))
    assert abs(total - ref) <= 1e-12 * abs(ref)
    m_only = cavi.predict_y(x_s)
    assert m_only[2] is None and torch.equal(m_only[0], got[0])
    # an object that was not made from raw inputs cannot predict
    Phi = torch.randn(512, 128, device=x.device) * 0.05
    plain = A.SparseCAVI(lik, Phi, torch.ones(512, device=x.device), y[:512], ctx=ctx)
    with pytest.raises(A.ArgumentError):
        plain.predict_y(x_s, y_s)
    with pytest.raises(A.ArgumentError):
        plain.heldout_logp(x_s, y_s)
