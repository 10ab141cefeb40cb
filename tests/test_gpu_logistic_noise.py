"""GPU tests of the logistic-noise likelihood (AGPL_LIK_LOGISTIC_NOISE = 10; run with -m gpu on an MI355X) through every layer that
takes a likelihood descriptor, against tests/logistic_noise_reference.py (float64 numpy, held by
tests/test_logistic_noise_reference_cpu.py to mpmath and quadrature; the oracle does not know the kind) and against
BinomialLikelihood(2) at f' = |y - f| / s, whose PG(b, c) code the oracle checks.

Bars, as tests/test_gpu_binomial.py lists where the project states them: float64 operators 1e-12 (the auxiliary posterior), 1e-11
(potentials, logtilt, expected_logtilt), 1e-10 (KL), aug_loglik 1e-9, float32 operators 3e-6 / 3e-5 (tests/test_gpu_parity.py);
natural parameters after ten sweeps 1e-5 of max|ref| and both ELBO routes 1e-5 relative (tests/test_gpu_binomial.py);
Gibbs G, g 5e-6 and the dense step 1e-6 max(1, max|f|) (tests/test_gpu_parity.py); log p 1e-4 absolute, moments 1e-5 relative +
1e-9 absolute (tests/test_gpu_predictive_domain.py); cdf and sf 1e-8 and 1e-4 relative from 1e-12 up, quantiles by the residual
|F_ref(q) - p| <= 2e-8 (tests/test_gpu_quantile.py, tests/test_gpu_asymlaplace.py); expected log-likelihood and gradient
10 x 2.526e-12 of max(1, |ref|), the first Adam step within 1e-6 of lr (tests/test_gpu_likgrad.py); leave-one-out: the cavity's bar
of tests/test_gpu_loo.py carried through the predictive's derivatives, as tests/test_gpu_asymlaplace.py does."""
import ctypes as C
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import logistic_noise_reference as R  # noqa: E402

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

SEED = 20261022
N = 777
SPLIT = 400
NPRED = (1, 2, 7, 1000)
NAT_TOL = 1e-5
ELL_TOL = 10.0 * 2.526e-12


@pytest.fixture(scope="module")
def A():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import __graft_entry__ as g

    g.build()
    import agpl_amd

    return agpl_amd


@pytest.fixture(scope="module")
def ctx(A):
    return A.Context(0, seed=SEED)


def dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    return t if dtype is None else t.to(dtype)


def host(t):
    return t.detach().cpu().numpy()


def relmax(a, b):
    return np.abs(np.asarray(a) - np.asarray(b)).max() / max(np.abs(np.asarray(b)).max(), 1e-300)


def points(rng, n=N):
    """(y, f, mu, var): real observations with a few far from the latent, in float32-exact values for y."""
    y = (rng.normal(size=n) * 1.5).astype(np.float32).astype(np.float64)
    y[:3] = (-9.0, 0.0, 11.0)
    return y, rng.normal(size=n), rng.normal(size=n) * 1.2, rng.uniform(0.05, 2.0, size=n)


def sparse_problem(M, scale=0.4, seed=3):
    """Features with |phi|^2 ~ 1 (one largest entry shared by both halves of the two-way split, as tests/test_gpu_binomial.py
    explains), a positive residual, a smooth truth, logistic noise about it and a non-zero prior mean."""
    rng = np.random.default_rng([seed, M])
    Phi = (rng.normal(size=(N, M)) / math.sqrt(M)).astype(np.float32)
    assert np.abs(Phi).max() < 0.9 or M < 16
    big = max(0.75, float(np.ceil(np.abs(Phi).max() * 4) / 4))
    Phi[0, 0] = Phi[SPLIT, 0] = big
    kd = rng.uniform(0.05, 0.3, size=N).astype(np.float32)
    mu0 = (0.3 * np.sin(np.arange(N) / 40.0)).astype(np.float32)
    f = Phi.astype(np.float64) @ rng.normal(size=M) + mu0
    y = R.inverse_cdf(scale, f, rng.uniform(size=N)).astype(np.float32)
    return Phi, kd, y, mu0


# ------------------------------------------------------------------------------------------ (a) accepted where it was refused
def test_every_entry_point_accepts_the_kind(A, ctx):
    """Each call below raised ArgumentError (AGPL_ERR_INVALID_ARGUMENT, unknown likelihood kind 10) before the kind existed."""
    rng = np.random.default_rng(1)
    lik = A.LogisticNoiseLikelihood(0.7)
    yh, fh, muh, varh = points(rng)
    y, f, mu, var = dev(yh), dev(fh), dev(muh), dev(varh)
    Om = A.aux_sample(lik, y, f, ctx=ctx, sweep=1)
    assert np.isfinite(host(Om.ω)).all() and (host(Om.ω) > 0).all()
    A.auglik_potential_and_precision(lik, Om, y, ctx=ctx)
    assert np.isfinite(A.logtilt(lik, Om, y, f, ctx=ctx)) and np.isfinite(A.aug_loglik(lik, Om, y, f, ctx=ctx))
    assert np.isfinite(A.aux_prior_logpdf(lik, Om, y, ctx=ctx))
    for dt in (torch.float64, torch.float32):
        q = A.aux_posterior(lik, y.to(dt), (mu.to(dt), var.to(dt)), ctx=ctx)
        A.expected_auglik_potential_and_precision(lik, q, y.to(dt), ctx=ctx)
    q = A.aux_posterior(lik, y, (mu, var), ctx=ctx)
    for fn in (A.expected_logtilt, A.expected_aug_loglik):
        assert np.isfinite(fn(lik, q, y, (mu, var), ctx=ctx))
    assert np.isfinite(A.aux_kldivergence(lik, q, y, ctx=ctx))
    K = np.exp(-0.5 * (np.subtract.outer(np.arange(64.0), np.arange(64.0)) / 8.0) ** 2) + 1e-6 * np.eye(64)
    A.DenseGibbs(lik, dev(K), dev(yh[3:67]), ctx=ctx).sweep()  # agpl_dense_gibbs_step
    assert all(np.isfinite(host(t)).all() for t in A.predictive(lik, (mu, var), y, ctx=ctx))
    assert all(np.isfinite(host(t)).all() for t in A.predictive_cdf(lik, (mu, var), y, ctx=ctx))
    assert np.isfinite(host(A.predictive_quantile(lik, (mu, var), (0.1, 0.5, 0.9), ctx=ctx))).all()
    tot, grad = A.expected_loglik(lik, mu, var, y, ctx=ctx)[:2]
    assert np.isfinite(tot) and grad.numel() == 1
    assert np.isfinite(host(A.sample_y(lik, f.to(torch.float32).reshape(1, 1, N), sweep=2, ctx=ctx))).all()
    ctx.synchronize()


@pytest.mark.parametrize("M", [5, 300])
def test_cavi_sweeps_against_the_reference(A, ctx, M):
    """(a), (h): ten sweeps with a prior mean, M = 5 and 300 (one and two 256-blocks of the padded plan): natural parameters, the
    fused kernel's ELBO terms and the operator kernels' elbo(), then leave-one-out at the fitted q(v)."""
    s = 0.4
    Phi, kd, y, mu0 = sparse_problem(M, s)
    lik = A.LogisticNoiseLikelihood(s)
    cavi = A.SparseCAVI(lik, dev(Phi), dev(kd), dev(y), mu0=dev(mu0[None]), ctx=ctx, keep_points=True, track_elbo=True)
    Phi_d = host(cavi.plan.features()).astype(np.float64)  # what the plan's images hold
    assert np.abs(Phi_d - Phi).max() <= 2.0 ** -21 * np.abs(Phi).max()
    ref = R.cavi_sweeps(s, Phi_d, host(cavi.plan.resid).astype(np.float64), y, 11, mu0=mu0)
    for it in range(10):
        e_ops = cavi.elbo()
        cavi.sweep()
        assert e_ops == pytest.approx(ref["elbo"][it], rel=1e-5)
        assert cavi.elbo_entering() == pytest.approx(ref["elbo"][it], rel=1e-5)  # agpl_fused_point_kernel<true, 10>
        if it in (0, 9):
            figs = relmax(host(cavi.G)[0], ref["G"][it]), relmax(host(cavi.g)[0], ref["g"][it])
            print(f"LOGISTIC NOISE CAVI M = {M} sweep {it + 1}: G {figs[0]:.3e}, g {figs[1]:.3e} of max|ref|")
            assert max(figs) < NAT_TOL, (it, figs)
    # (h) leave-one-out: the rule of include/agpl_loo.h on the reference's sites, the predictive of the reference at that cavity
    import loo_reference as LR

    gam, bet, d = ref["gamma"][9][None], ref["beta"][9][None], host(cavi.plan.resid).astype(np.float64)
    cm, cv, h = LR.closed_form(Phi_d, d, gam, bet, mu0=mu0[None].astype(np.float64))
    mu_m, var_m = ref["mu"][10][None], ref["var"][10][None]
    Tv, Tm = 2e-5 * np.abs(var_m).max(), 2e-5 * max(1.0, np.abs(mu_m).max())
    q, a = var_m - d[None], mu_m - mu0[None]
    bar_v = Tv / (1 - h) ** 2
    bar_m = (Tm + np.abs(bet) * Tv) / (1 - h) + np.abs(a - bet * q) * gam * Tv / (1 - h) ** 2
    # ... carried through the predictive: |d log p / d mu| = |E tanh| / s <= 1 / s =: r, |d log p / d var| <= r^2 / 2 (the density
    # solves the heat equation in var and |p''| / p <= r^2 for a mixture of sech^2 densities)
    r = 1.0 / s
    bar_lp = (r * bar_m + 0.5 * r * r * bar_v)[0]
    idx = np.arange(0, N, 37)  # (the reference integrates each point at 50 digits: every 37th point, 21 of them)
    lp_ref = np.array([R.logp(s, float(y[i]), cm[0, i], cv[0, i]) for i in idx])
    loo = cavi.loo()
    lp = host(loo.logp)
    print(f"LOGISTIC NOISE LOO M = {M}: worst |logp - ref| / bar {(np.abs(lp[idx] - lp_ref) / bar_lp[idx]).max():.3e}")
    assert loo.n_bad == 0 and (np.abs(lp[idx] - lp_ref) <= bar_lp[idx]).all()
    assert abs(loo.elpd - float(np.sum(lp.astype(np.longdouble)))) <= N * 2.0 ** -53 * np.abs(lp).sum()  # tests/test_gpu_loo.py


# ------------------------------------------------------------------------------------------ refused parameters
@pytest.mark.parametrize("scale", [0.0, -1.0, math.inf, math.nan])
def test_bad_scale_is_refused_with_a_message(A, ctx, scale):
    lik = A.LogisticNoiseLikelihood(scale)
    z = torch.zeros(4, dtype=torch.float64, device="cuda")
    calls = [lambda: A.aux_sample(lik, z, z, ctx=ctx, sweep=1), lambda: A.aux_posterior(lik, z, (z, z + 1), ctx=ctx),
             lambda: A.predictive(lik, (z, z + 1), z, ctx=ctx), lambda: A.predictive_cdf(lik, (z, z + 1), z, ctx=ctx),
             lambda: A.predictive_quantile(lik, (z, z + 1), (0.5,), ctx=ctx), lambda: A.expected_loglik(lik, z, z + 1, z, ctx=ctx),
             lambda: A.sample_y(lik, z.to(torch.float32).reshape(1, 1, 4), sweep=1, ctx=ctx)]
    for call in calls:
        with pytest.raises(A.ArgumentError, match="LogisticNoise needs"):
            call()


# ------------------------------------------------------------------------------------------ (b) the draws are Binomial(2)'s
@pytest.mark.parametrize("scale", [0.25, 3.0])
def test_omega_is_the_binomial_kinds_at_the_standardised_residual(A, scale):
    """The same context seed and point offset: omega, the uniforms consumed and the series indices are those of
    BinomialLikelihood(2) at f' = |y - f| / s (formed on the host with the device's float64 expression), byte for byte; so is the
    prior density PG(2, 0) of those draws."""
    rng = np.random.default_rng([3, int(100 * scale)])
    ln, bi = A.LogisticNoiseLikelihood(scale), A.BinomialLikelihood(2)
    yh, fh, _, _ = points(rng)
    fp = np.abs(yh - fh) / scale
    c1, c2 = A.Context(0, seed=SEED), A.Context(0, seed=SEED)
    c1.set_point_offset(12345)
    c2.set_point_offset(12345)
    yb = dev(np.ones(N, dtype=np.int32))
    o1, u1, t1 = A.aux_sample_(A.init_aux_variables(ln, N, ctx=c1), ln, dev(yh), dev(fh), ctx=c1, sweep=5, stats=True)
    o2, u2, t2 = A.aux_sample_(A.init_aux_variables(bi, N, ctx=c2), bi, yb, dev(fp), ctx=c2, sweep=5, stats=True)
    assert torch.equal(o1.ω, o2.ω) and torch.equal(u1, u2) and torch.equal(t1, t2)
    assert A.aux_prior_logpdf(ln, o1, dev(yh), ctx=c1) == A.aux_prior_logpdf(bi, o2, yb, ctx=c2)


# ------------------------------------------------------------------------------------------ (c) operators
def test_operators_against_the_reference(A, ctx):
    s = 0.7
    rng = np.random.default_rng(5)
    lik = A.LogisticNoiseLikelihood(s)
    y, f, mu, var = points(rng)
    Om = A.aux_sample(lik, dev(y), dev(f), ctx=ctx, sweep=7)
    om = host(Om.ω)
    beta, gamma = A.auglik_potential_and_precision(lik, Om, dev(y), ctx=ctx)
    rb, rg = R.sampled_potential_precision(s, y, om)
    assert np.allclose(host(beta[0]), rb, rtol=1e-11, atol=1e-14) and np.allclose(host(gamma[0]), rg, rtol=1e-11, atol=0)
    assert A.logtilt(lik, Om, dev(y), dev(f), ctx=ctx) == pytest.approx(R.logtilt(s, y, om, f), rel=1e-11)
    prior = A.aux_prior_logpdf(lik, Om, dev(y), ctx=ctx)
    assert A.aug_loglik(lik, Om, dev(y), dev(f), ctx=ctx) == pytest.approx(R.logtilt(s, y, om, f) + prior, rel=1e-9)
    c_ref = R.aux_posterior(s, y, mu, var)
    for dt, rtol in ((torch.float64, 1e-12), (torch.float32, 3e-6)):
        q = A.aux_posterior(lik, dev(y, dt), (dev(mu, dt), dev(var, dt)), ctx=ctx)
        assert q.inds[0]["c"].dtype == dt and np.allclose(host(q.inds[0]["c"]).astype(np.float64), c_ref, rtol=rtol, atol=1e-30)
        bt, gm = A.expected_auglik_potential_and_precision(lik, q, dev(y, dt), ctx=ctx)
        rb, rg = R.expected_potential_precision(s, y, c_ref)
        assert np.allclose(host(bt[0]).astype(np.float64), rb, rtol=10 * rtol, atol=1e-6 if dt == torch.float32 else 1e-14)
        assert np.allclose(host(gm[0]).astype(np.float64), rg, rtol=10 * rtol, atol=0)
        if dt == torch.float64:
            qf = (dev(mu), dev(var))
            assert A.expected_logtilt(lik, q, dev(y), qf, ctx=ctx) == pytest.approx(R.expected_logtilt(s, y, c_ref, mu, var), rel=1e-11)
            assert A.aux_kldivergence(lik, q, dev(y), ctx=ctx) == pytest.approx(R.aux_kl(c_ref), rel=1e-10)
            want = R.expected_logtilt(s, y, c_ref, mu, var) + R.aux_kl(c_ref)  # generic.jl:52-54, the reference's sign
            assert A.expected_aug_loglik(lik, q, dev(y), qf, ctx=ctx) == pytest.approx(want, rel=1e-11)


# ------------------------------------------------------------------------------------------ (d) Gibbs
@pytest.mark.parametrize("M", [5, 300])
def test_gibbs_sweep_against_the_reference_and_sharded(A, oracle, M):
    s = 0.4
    Phi, kd, y, mu0 = sparse_problem(M, s, seed=4)
    lik = A.LogisticNoiseLikelihood(s)
    gib = A.SparseGibbs(lik, dev(Phi), dev(kd), dev(y), mu0=dev(mu0[None]), ctx=A.Context(0, seed=777), keep_points=True)
    gib.sweep()
    om, f = host(gib.omega)[:, 0], host(gib.f)[:, 0]
    assert np.isfinite(om).all() and (om > 0).all()
    beta, gamma = R.sampled_potential_precision(s, y.astype(np.float64), om)
    Phi_d = host(gib.plan.features())
    Gr, gr = oracle.accumulate(Phi_d, beta.astype(np.float32).astype(np.float64)[None], gamma.astype(np.float32).astype(np.float64)[None])
    assert relmax(host(gib.G), Gr) < 5e-6 and relmax(host(gib.g), gr) < 5e-6
    for lo, hi in ((0, SPLIT), (SPLIT, N)):  # two shards with their point offsets: the single-process omega and f, bit for bit
        part = A.SparseGibbs(lik, dev(Phi[lo:hi]), dev(kd[lo:hi]), dev(y[lo:hi]), mu0=dev(mu0[None, lo:hi]), ctx=A.Context(0, seed=777),
                             keep_points=True, point_offset=lo)
        part.sweep()
        assert np.array_equal(host(part.omega)[:, 0], om[lo:hi]) and np.array_equal(host(part.f)[:, 0], f[lo:hi])


def test_dense_gibbs_step_against_the_reference(A, oracle):
    import scipy.linalg as sla

    Nd, s = 300, 0.4
    rng = np.random.default_rng(31)
    x = np.sort(rng.uniform(-10, 10, size=Nd))
    K = np.exp(-0.5 * ((x[:, None] - x[None, :]) / 2.0) ** 2) + 1e-6 * np.eye(Nd)
    y = R.inverse_cdf(s, 2 * np.sin(0.7 * x), rng.uniform(size=Nd))
    dg = A.DenseGibbs(A.LogisticNoiseLikelihood(s), dev(K), dev(y), ctx=A.Context(0, seed=4242))
    Lk = np.linalg.cholesky(K)
    for _ in range(2):
        dg.sweep()
        beta, gamma = R.sampled_potential_precision(s, y, host(dg.omega))
        z = oracle.randn(4242, 0, (dg.sweep_index | 0x80000000) & 0xFFFFFFFF, 2 * Nd)  # the step of oracle.dense_gibbs_step
        f0 = Lk @ z[:Nd]
        sg = np.sqrt(gamma)
        r = beta / sg - sg * f0 - z[Nd:]
        f = f0 + K @ (sg * sla.cho_solve(sla.cho_factor(np.eye(Nd) + sg[:, None] * K * sg[None, :], lower=True), r))
        assert np.abs(host(dg.f) - f).max() < 1e-6 * max(1.0, np.abs(f).max())


# ------------------------------------------------------------------------------------------ (e), (g) the prediction end
def _check_tails(got, want):
    assert np.abs(got - want).max() <= 1e-8
    big = want >= 1e-12
    assert (np.abs(got - want)[big] <= 1e-4 * want[big]).all(), (np.abs(got - want)[big] / want[big]).max()


def test_predictive_over_the_domain_grid(A, ctx):
    """s in {1e-3, 1, 1e3} x sqrt(var) in {0, 1e-8, 1, 50} x (y - mu) / sd in {0, +-1, +-8, +-50}, point by point against 50-digit
    values: log p, both tails, the moments, the expected log-likelihood and its gradient."""
    g = R.grid()
    for s in R.SCALES:
        r = g[g[:, 0] == s]
        lik = A.LogisticNoiseLikelihood(s)
        mu, var, y = np.full(len(r), R.GRID_MU), r[:, 1], r[:, 2]
        me, va, lp = (host(t) for t in A.predictive(lik, (dev(mu), dev(var)), dev(y), ctx=ctx))
        rva = var + s * s * math.pi ** 2 / 3.0
        assert np.array_equal(me, mu) and (np.abs(va - rva) <= 1e-5 * rva + 1e-9).all()
        print(f"LOGISTIC NOISE grid s = {s}: worst |log p - mpmath| = {np.abs(lp - r[:, 3]).max():.3e}")
        assert np.abs(lp - r[:, 3]).max() <= 1e-4
        cdf, sf = (host(t) for t in A.predictive_cdf(lik, (dev(mu), dev(var)), dev(y), ctx=ctx))
        _check_tails(cdf, r[:, 4])
        _check_tails(sf, r[:, 5])
        _, _, ell, dell = A.expected_loglik(lik, dev(mu), dev(var), dev(y), ctx=ctx, per_point=True)
        fig = max((np.abs(host(ell) - r[:, 6]) / np.maximum(1.0, np.abs(r[:, 6]))).max(),
                  (np.abs(host(dell)[:, 0] - r[:, 7]) / np.maximum(1.0, np.abs(r[:, 7]))).max())
        print(f"LOGISTIC NOISE grid s = {s}: expected_loglik worst |device - mpmath| / max(1, |ref|) = {fig:.3e}")
        assert fig <= ELL_TOL


@pytest.mark.parametrize("n", NPRED)
def test_predictive_against_the_reference(A, ctx, n):
    """n prediction points; R = sqrt(var) / s runs from 0 through the thresholds 1e-3 and 1 between the rules (the points beside
    them are set by hand) to 60."""
    s = 0.7
    rng = np.random.default_rng([6, n])
    lik = A.LogisticNoiseLikelihood(s)
    mu, y = rng.normal(size=n) * 2.0, rng.normal(size=n) * 3.0
    R_ = np.exp(rng.uniform(np.log(0.05), np.log(60.0), size=n))
    R_[:7] = (0.0, 0.999, 1.0, 1.001, 0.3, 25.0, 60.0)[:min(n, 7)]
    R_[7:10] = (0.999e-3, 1e-3, 1.001e-3)[:max(0, min(n, 10) - 7)]  # the threshold R^2 = 1e-6 of the narrow expansion
    var = (R_ * s) ** 2
    k = min(n, 7)
    if k > 3:  # far observations, out to the domain's 50 predictive standard deviations
        y[3:k] = mu[3:k] + np.array((-6.0, 5.0, 30.0, -50.0))[:k - 3] * np.sqrt(var[3:k] + s * s * R.VAR_LOGISTIC)
    qf = (dev(mu), dev(var))
    idx = np.arange(min(n, 10))  # (the reference integrates each point at 50 digits; the hand-set points are the first seven)
    me, va, lp = (host(t) for t in A.predictive(lik, qf, dev(y), ctx=ctx))
    rva = R.moments(s, mu, var)[1]
    assert np.array_equal(me, mu) and (np.abs(va - rva) <= 1e-5 * rva + 1e-9).all()
    assert np.abs(lp[idx] - np.array([R.logp(s, y[i], mu[i], var[i]) for i in idx])).max() <= 1e-4
    cdf, sf = (host(t) for t in A.predictive_cdf(lik, qf, dev(y), ctx=ctx))
    ref = np.array([R.cdf(s, y[i], mu[i], var[i]) for i in idx])
    _check_tails(cdf[idx], ref[:, 0])
    _check_tails(sf[idx], ref[:, 1])
    assert np.abs(cdf + sf - 1.0).max() <= 1e-8
    probs = (0.001, 0.05, 0.5, 0.9, 0.999)
    q = host(A.predictive_quantile(lik, qf, probs, ctx=ctx))
    assert q.shape == (n, len(probs)) and np.isfinite(q).all() and (np.diff(q, axis=1) >= 0).all()
    worst = 0.0
    for i in idx[1:4]:  # (R = 0.999, 1, 1.001: both rules)
        for j, pj in enumerate(probs):
            worst = max(worst, abs(R.tail(s, float(q[i, j]), mu[i], var[i], upper=pj > 0.5) - min(pj, 1.0 - pj)))
    print(f"LOGISTIC NOISE quantiles n = {n}: worst |F_ref(q) - p| = {worst:.3e}")
    assert worst <= 2e-8
    tot, grad, ell, dell = A.expected_loglik(lik, dev(mu), dev(var), dev(y), ctx=ctx, per_point=True)
    rell, rdell = R.expected_loglik(s, y[idx], mu[idx], var[idx])
    fig = max((np.abs(host(ell)[idx] - rell) / np.maximum(1.0, np.abs(rell))).max(),
              (np.abs(host(dell)[idx, 0] - rdell) / np.maximum(1.0, np.abs(rdell))).max())
    print(f"LOGISTIC NOISE expected_loglik n = {n}: worst |device - ref| / max(1, |ref|) = {fig:.3e}")
    assert fig <= ELL_TOL
    assert tot == pytest.approx(float(host(ell).sum()), rel=1e-11, abs=1e-11) and float(grad[0]) == pytest.approx(float(host(dell).sum()), rel=1e-11, abs=1e-11)


def test_conventions_are_the_laplace_kinds(A, ctx):
    """A non-finite y and a bad marginal (NaN mean, negative variance) give what the Laplace kind gives, output for output."""
    ln, lap = A.LogisticNoiseLikelihood(0.5), A.LaplaceLikelihood(1.0)
    mu = dev(np.array([0.3, 0.3, 0.3, 0.3, math.nan, 0.3, 0.3, 0.3]))
    var = dev(np.array([1.0, 1.0, 1.0, 0.0, 1.0, -1.0, 0.0, 0.0]))
    y = dev(np.array([math.inf, -math.inf, math.nan, 0.1, 0.1, 0.1, math.inf, math.nan]))
    kind = lambda a: np.where(np.isnan(a), 0, np.where(np.isposinf(a), 1, np.where(np.isneginf(a), 2, 3)))
    for fn in (lambda l: A.predictive(l, (mu, var), y, ctx=ctx), lambda l: A.predictive_cdf(l, (mu, var), y, ctx=ctx),
               lambda l: A.expected_loglik(l, mu, var, y, ctx=ctx, per_point=True)[2:]):
        for a, b in zip(fn(ln), fn(lap)):
            assert np.array_equal(kind(host(a)), kind(host(b))), (host(a), host(b))


# ------------------------------------------------------------------------------------------ (f) draws of y
def test_draws_are_the_inverse_cdf_of_the_streams_uniform(A, oracle):
    from sample_y_reference import Stream

    s = 0.7
    T, Ns, point0, draw0, sweep = 3, 97, 2 ** 32 - 40, 65534, 11
    rng = np.random.default_rng(7)
    F = rng.uniform(-4, 4, size=(T, 1, Ns)).astype(np.float32)
    F[0, 0, 0] = np.nan
    sctx = A.Context(0, seed=SEED)
    lik = A.LogisticNoiseLikelihood(s)
    got = host(A.sample_y(lik, dev(F), point0=point0, draw0=draw0, sweep=sweep, ctx=sctx))
    u = np.array([[Stream(oracle, SEED, point0 + i, sweep, draw0 + t).u01() for i in range(Ns)] for t in range(T)])
    f64 = F[:, 0, :].astype(np.float64)
    ref = R.inverse_cdf(s, f64, u)
    assert np.isnan(got[0, 0]) and got.dtype == np.float64
    ok = np.isfinite(ref)
    # 4 ulp of the largest operand: y = f + s (log u - log1p(-u)) is rounded once per operation, the two logarithms carry an ulp or
    # two of their own, and where operands nearly cancel an ulp of the result says nothing about either
    big = np.maximum.reduce([np.abs(ref), np.abs(f64), s * np.abs(np.log(u)), s * np.abs(np.log1p(-u))])
    ulp = np.spacing(big)
    print(f"LOGISTIC NOISE draws: worst |device - reference| = {np.nanmax(np.abs(got - ref)[ok] / ulp[ok]):.2f} ulp")
    assert ok.sum() == T * Ns - 1 and (np.abs(got - ref)[ok] <= 4.0 * ulp[ok]).all()
    s1, s2 = A.Context(0, seed=SEED), A.Context(0, seed=SEED)
    s1.set_point_offset(point0)
    s2.set_point_offset(point0 + 50)
    left = host(A.sample_y(lik, dev(F[:, :, :50]), sweep=sweep, draw0=draw0, ctx=s1))
    right = host(A.sample_y(lik, dev(F[:, :, 50:]), sweep=sweep, draw0=draw0, ctx=s2))
    assert np.concatenate([left, right], axis=1).tobytes() == got.tobytes()


# ------------------------------------------------------------------------------------------ (i) learning the scale
def test_learn_likelihood_learns_the_scale(A, ctx):
    """Data drawn at scale 0.7, started at 2: every outer step is the Adam step lr in the direction of the reference's gradient at
    the marginals it was taken at, and the bound rises from step to step."""
    lr = 0.05
    rng = np.random.default_rng(9)
    M = 24
    Phi = (rng.normal(size=(N, M)) / math.sqrt(M)).astype(np.float32)
    kd = rng.uniform(0.05, 0.3, size=N).astype(np.float32)
    y = R.inverse_cdf(0.7, Phi.astype(np.float64) @ rng.normal(size=M), rng.uniform(size=N)).astype(np.float32)
    cavi = A.SparseCAVI(A.LogisticNoiseLikelihood(2.0), dev(Phi), dev(kd), dev(y), ctx=ctx)
    bounds, sc = [], [2.0]
    idx = np.arange(0, N, 40)
    for step in range(6):
        tr = A.learn_likelihood(cavi, nouter=1, nsweeps=3, lr=lr)  # (one outer step a call: Adam's first step is lr sign(g))
        mu, var = (host(t)[0].astype(np.float64) for t in cavi.marginals())
        _, dref = R.expected_loglik(sc[-1], y.astype(np.float64)[idx], mu[idx], var[idx], value=False)  # (every 40th point: the sign is far from close)
        d = float(tr["lik"][1, 0] - tr["lik"][0, 0])
        assert np.sign(d) == np.sign(dref.sum()) and abs(abs(d) - lr) <= 1e-6 * lr
        sc.append(cavi.lik.scale)
        cavi.sweep()
        bounds.append(cavi.bound())
    print(f"LOGISTIC NOISE learn_likelihood: scale {sc}, bound {bounds}")
    assert sc[-1] < sc[0] and abs(math.log(sc[-1]) - math.log(0.7)) < abs(math.log(2.0) - math.log(0.7))
    assert all(b >= a for a, b in zip(bounds, bounds[1:])), bounds
