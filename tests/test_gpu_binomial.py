"""GPU tests of the binomial likelihood (AGPL_LIK_BINOMIAL = 8, Binomial(n, sigma(f)); run with -m gpu on an MI355X) through every
layer that takes a likelihood descriptor, against tests/binomial_reference.py (float64 numpy; the oracle does not know the kind)
and against the negative-binomial kind, whose PG(b, c) code the oracle already checks: Binomial(n) and NegBinomial(r = 1) with
y = n - 1 at every point have the same b = n.

Bars, all read from where the project states them for the kinds it has: float64 operators 1e-12 (c), 1e-11 (potentials, logtilt,
expected_logtilt), aug_loglik 1e-9, float32 operators 3e-6 / 3e-5 (tests/test_gpu_parity.py, negative-binomial cases); natural
parameters after ten sweeps 1e-5 of max|ref|; Gibbs G, g 5e-6 and the dense step 1e-6 max(1, max|f|)
(tests/test_gpu_parity.py); log p 1e-4 absolute, moments 1e-5 relative + 1e-9 absolute (include/agpl_predictive.h as
tests/test_gpu_predictive_domain.py holds it); cdf and sf 1e-8 and 1e-4 relative from 1e-12 up (tests/test_gpu_quantile.py);
expected log-likelihood 10 x 2.526e-12 of max(1, |ref|) (tests/test_gpu_likgrad.py, Bernoulli)."""
import ctypes as C
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import binomial_reference as B  # noqa: E402
from test_binomial_reference_cpu import LEVELS, QUANTILE_CASES  # noqa: E402

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

SEED = 20261020
N = 777
SPLIT = 400  # the two-way split of the points in the Gibbs test
NS = (1, 2, 7, 1000)
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


def counts(rng, n, size, f=None):
    """y ~ Binomial(n, sigma(f)) from numpy, with 0 and n at the first points."""
    p = 0.5 if f is None else 1.0 / (1.0 + np.exp(-f))
    y = rng.binomial(n, p, size=size).astype(np.int32)
    y[0], y[1] = 0, n
    return y


def features(rng, n, M, scale):
    return (rng.normal(size=(n, M)) * scale).astype(np.float32)


def sparse_problem(M, n, seed=3):
    """Features with |phi|^2 ~ 1, a positive residual, a smooth truth and binomial counts of it."""
    rng = np.random.default_rng([seed, M, n])
    Phi = features(rng, N, M, 1.0 / math.sqrt(M))
    # one largest entry, the same in both halves of the two-way split of the Gibbs test: a plan scales its float16 images by a
    # power of two chosen from max |Phi| of the points IT holds, so shards reproduce the single-process features -- and with them
    # f and omega -- bit for bit only if their largest entries share a binade (|N(0, 1)| / sqrt(M) stays below 0.75 here)
    assert np.abs(Phi).max() < 0.75
    Phi[0, 0] = Phi[SPLIT, 0] = 0.75
    kd = rng.uniform(0.05, 0.3, size=N).astype(np.float32)
    w = rng.normal(size=M)
    f = Phi.astype(np.float64) @ w
    return Phi, kd, counts(rng, n, N, f)


# ------------------------------------------------------------------------------------------ 1. accepted where it was refused
def test_every_entry_point_accepts_the_kind(A, ctx):
    """Each call below raised ArgumentError (AGPL_ERR_INVALID_ARGUMENT, unknown likelihood kind 8) before the kind existed."""
    rng = np.random.default_rng(1)
    lik = A.BinomialLikelihood(7)
    f = dev(rng.normal(size=N))
    mu, var = dev(rng.normal(size=N)), dev(rng.uniform(0.1, 2.0, size=N))
    y = dev(counts(rng, 7, N))
    Om = A.aux_sample(lik, y, f, ctx=ctx, sweep=1)
    assert np.isfinite(host(Om.ω)).all() and (host(Om.ω) > 0).all()
    A.auglik_potential_and_precision(lik, Om, y, ctx=ctx)
    assert np.isfinite(A.logtilt(lik, Om, y, f, ctx=ctx)) and np.isfinite(A.aug_loglik(lik, Om, y, f, ctx=ctx))
    assert np.isfinite(A.aux_prior_logpdf(lik, Om, y, ctx=ctx))
    for dt in (torch.float64, torch.float32):
        q = A.aux_posterior(lik, y, (mu.to(dt), var.to(dt)), ctx=ctx)
        A.expected_auglik_potential_and_precision(lik, q, y, ctx=ctx)
    q = A.aux_posterior(lik, y, (mu, var), ctx=ctx)
    for fn in (A.expected_logtilt, A.expected_aug_loglik):
        assert np.isfinite(fn(lik, q, y, (mu, var), ctx=ctx))
    assert np.isfinite(A.aux_kldivergence(lik, q, y, ctx=ctx))
    Phi, kd, yy = sparse_problem(64, 7)
    p = lambda t: C.c_void_p(t.data_ptr() if t is not None else 0)
    d = lik.desc()
    Phi128 = np.zeros((N, 128), dtype=np.float32)
    Phi128[:, :64] = Phi
    dP, dk, dy = dev(Phi128), dev(kd), dev(yy)
    G, g = torch.empty((1, 128, 128), dtype=torch.float64, device="cuda"), torch.empty((1, 128), dtype=torch.float64, device="cuda")
    W, al = torch.zeros((1, 128, 128), dtype=torch.float32, device="cuda"), torch.zeros((1, 128), dtype=torch.float32, device="cuda")
    ctx.call("agpl_cavi_pass", C.byref(d), C.c_int64(N), C.c_int32(128), p(dP), p(dk), p(None), p(dy), p(W), p(al), p(G), p(g), p(None),
             p(None), p(None))
    v = dev(rng.normal(size=(1, 128)))
    ctx.call("agpl_gibbs_pass", C.byref(d), C.c_int64(N), C.c_int32(128), p(dP), p(dk), p(None), p(dy), p(v), C.c_uint32(3), p(G), p(g),
             p(None), p(None), p(None), p(None))
    cavi = A.SparseCAVI(lik, dev(Phi), dk, dy, ctx=ctx, track_elbo=True)  # agpl_cavi_pass_plan, the fused kernel's ELBO instantiation
    cavi.sweep()
    cavi.check()
    A.SparseGibbs(lik, dev(Phi), dk, dy, ctx=ctx).sweep()  # agpl_gibbs_pass_plan
    K = np.exp(-0.5 * (np.subtract.outer(np.arange(64.0), np.arange(64.0)) / 8.0) ** 2) + 1e-6 * np.eye(64)
    A.DenseGibbs(lik, dev(K), dev(counts(rng, 7, 64)), ctx=ctx).sweep()  # agpl_dense_gibbs_step
    assert all(np.isfinite(host(t)).all() for t in A.predictive(lik, (mu, var), y, ctx=ctx))
    assert all(np.isfinite(host(t)).all() for t in A.predictive_cdf(lik, (mu, var), y, ctx=ctx))
    assert np.isfinite(host(A.predictive_quantile(lik, (mu, var), LEVELS, ctx=ctx))).all()
    assert np.isfinite(A.expected_loglik(lik, mu, var, y, ctx=ctx)[0])
    ys = host(A.sample_y(lik, f.to(torch.float32).reshape(1, 1, N), sweep=2, ctx=ctx))
    assert ys.min() >= 0 and ys.max() <= 7
    ctx.synchronize()


@pytest.mark.parametrize("n", [0, 2.5, 2 ** 22, -3, float("nan")])
def test_a_bad_trial_count_is_refused_with_a_message(A, ctx, n):
    lik = A.BinomialLikelihood(n)
    z = torch.zeros(4, dtype=torch.float64, device="cuda")
    y = torch.zeros(4, dtype=torch.int32, device="cuda")
    calls = [lambda: A.aux_sample(lik, y, z, ctx=ctx, sweep=1), lambda: A.aux_posterior(lik, y, (z, z + 1), ctx=ctx),
             lambda: A.predictive(lik, (z, z + 1), y, ctx=ctx), lambda: A.predictive_cdf(lik, (z, z + 1), y, ctx=ctx),
             lambda: A.expected_loglik(lik, z, z + 1, y, ctx=ctx), lambda: A.sample_y(lik, z.to(torch.float32).reshape(1, 1, 4), sweep=1, ctx=ctx)]
    for call in calls:
        with pytest.raises(A.ArgumentError, match="trials n"):
            call()
    assert A.BinomialLikelihood(2 ** 22 - 1).desc().p[0] == 2 ** 22 - 1
    A.aux_posterior(A.BinomialLikelihood(2 ** 22 - 1), y, (z, z + 1), ctx=ctx)


# ------------------------------------------------------------------------------------------ 2. the negative-binomial twin
@pytest.mark.parametrize("n", NS)
def test_negative_binomial_twin_is_bit_identical(A, n):
    """The same functions of (b, c) on the same Philox streams: omega, the uniforms consumed, the series index, c, the expected
    precision in both precisions, the KL and the prior density are equal bit for bit, with a point offset set."""
    rng = np.random.default_rng([2, n])
    bi, nb = A.BinomialLikelihood(n), A.NegativeBinomialLikelihood(1.0)
    f = dev(rng.normal(size=N) * 2.0)
    mu, var = dev(rng.normal(size=N) * 1.5), dev(rng.uniform(0.05, 2.0, size=N))
    y_bi, y_nb = dev(counts(rng, n, N)), torch.full((N,), n - 1, dtype=torch.int32, device="cuda")
    c1, c2 = A.Context(0, seed=SEED), A.Context(0, seed=SEED)
    c1.set_point_offset(12345)
    c2.set_point_offset(12345)
    o1, u1, t1 = A.aux_sample_(A.init_aux_variables(bi, N, ctx=c1), bi, y_bi, f, ctx=c1, sweep=5, stats=True)
    o2, u2, t2 = A.aux_sample_(A.init_aux_variables(nb, N, ctx=c2), nb, y_nb, f, ctx=c2, sweep=5, stats=True)
    assert torch.equal(o1.ω, o2.ω) and torch.equal(u1, u2) and torch.equal(t1, t2)
    assert A.aux_prior_logpdf(bi, o1, y_bi, ctx=c1) == A.aux_prior_logpdf(nb, o2, y_nb, ctx=c2)
    for dt in (torch.float64, torch.float32):
        q1 = A.aux_posterior(bi, y_bi, (mu.to(dt), var.to(dt)), ctx=c1)
        q2 = A.aux_posterior(nb, y_nb, (mu.to(dt), var.to(dt)), ctx=c2)
        assert torch.equal(q1.inds[0]["c"], q2.inds[0]["c"])
        g1 = A.expected_auglik_precision(bi, q1, y_bi, ctx=c1)[0]
        g2 = A.expected_auglik_precision(nb, q2, y_nb, ctx=c2)[0]
        assert g1.dtype == dt and torch.equal(g1, g2)
        if dt == torch.float64:
            assert A.aux_kldivergence(bi, q1, y_bi, ctx=c1) == A.aux_kldivergence(nb, q2, y_nb, ctx=c2)


# ------------------------------------------------------------------------------------------ 3. against the float64 reference
@pytest.mark.parametrize("n", NS)
def test_operators_against_the_reference(A, ctx, oracle, n):
    rng = np.random.default_rng([3, n])
    lik = A.BinomialLikelihood(n)
    f = rng.normal(size=N) * 2.0
    mu, var = rng.normal(size=N) * 1.5, rng.uniform(0.05, 2.0, size=N)
    y = counts(rng, n, N, f)
    yf = y.astype(np.float64)
    Om = A.aux_sample(lik, dev(y), dev(f), ctx=ctx, sweep=7)
    om = host(Om.ω)
    beta, gamma = A.auglik_potential_and_precision(lik, Om, dev(y), ctx=ctx)
    rb, rg = B.sampled_potential_precision(n, yf, om)
    assert np.allclose(host(beta[0]), rb, rtol=1e-10, atol=1e-300) and np.array_equal(host(gamma[0]), rg)
    assert A.logtilt(lik, Om, dev(y), dev(f), ctx=ctx) == pytest.approx(B.logtilt(n, yf, om, f), rel=1e-11)
    prior = sum(oracle.pg_logpdf(float(n), 0.0, float(w)) for w in om)
    assert A.aug_loglik(lik, Om, dev(y), dev(f), ctx=ctx) == pytest.approx(B.logtilt(n, yf, om, f) + prior, rel=1e-9)
    for dt, rtol in ((torch.float64, 1e-12), (torch.float32, 3e-6)):
        q = A.aux_posterior(lik, dev(y), (dev(mu, dt), dev(var, dt)), ctx=ctx)
        c_ref = B.aux_posterior(mu, var)
        assert np.allclose(host(q.inds[0]["c"]).astype(np.float64), c_ref, rtol=rtol, atol=1e-30)
        bt, gm = A.expected_auglik_potential_and_precision(lik, q, dev(y), ctx=ctx)
        rb, rg = B.expected_potential_precision(n, yf, c_ref)
        assert np.allclose(host(bt[0]).astype(np.float64), rb, rtol=10 * rtol, atol=1e-6 if dt == torch.float32 else 1e-14)
        assert np.allclose(host(gm[0]).astype(np.float64), rg, rtol=10 * rtol, atol=0)
        if dt == torch.float64:
            el = A.expected_logtilt(lik, q, dev(y), (dev(mu), dev(var)), ctx=ctx)
            assert el == pytest.approx(B.expected_logtilt(n, yf, c_ref, mu, var), rel=1e-11)
            kl = A.aux_kldivergence(lik, q, dev(y), ctx=ctx)
            assert kl == pytest.approx(B.aux_kl(n, c_ref), rel=1e-10)
    # a count outside 0 .. n: -inf at that point, no error
    for bad in (-1, n + 1):
        yb = y.copy()
        yb[5] = bad
        assert A.logtilt(lik, Om, dev(yb), dev(f), ctx=ctx) == -math.inf
        assert A.aug_loglik(lik, Om, dev(yb), dev(f), ctx=ctx) == -math.inf
        lp = host(A.predictive(lik, (dev(mu), dev(var)), dev(yb), ctx=ctx)[2])
        assert lp[5] == -math.inf and np.isfinite(np.delete(lp, 5)).all()
        assert host(A.expected_loglik(lik, dev(mu), dev(var), dev(yb), ctx=ctx, per_point=True)[2])[5] == -math.inf


# ------------------------------------------------------------------------------------------ 4. sweeps
@pytest.mark.parametrize("M", [64, 200])
@pytest.mark.parametrize("n", [1, 7, 1000])
def test_cavi_sweeps_against_the_reference(A, ctx, M, n):
    Phi, kd, y = sparse_problem(M, n)
    lik = A.BinomialLikelihood(n)
    cavi = A.SparseCAVI(lik, dev(Phi), dev(kd), dev(y), ctx=ctx, keep_points=True)
    Phi_d = host(cavi.plan.features()).astype(np.float64)  # what the plan's images hold: the features to 2^-22
    assert np.abs(Phi_d - Phi).max() <= 2.0 ** -21 * np.abs(Phi).max()
    ref = B.cavi_sweeps(n, Phi_d, host(cavi.plan.resid).astype(np.float64), y, 11)
    elbos = []
    for it in range(10):
        elbos.append(cavi.elbo())
        cavi.sweep()
        if it in (0, 9):
            assert relmax(host(cavi.G)[0], ref["G"][it]) < NAT_TOL, (it, relmax(host(cavi.G)[0], ref["G"][it]))
            assert relmax(host(cavi.g)[0], ref["g"][it]) < NAT_TOL
    elbos.append(cavi.elbo())
    # (elbo() reads float32 marginals: each per-point term carries their 2^-23 relative rounding through slopes of order n, so
    #  two evaluations of an unchanged bound differ by up to ~1e-6 of it; the float64 restatement has no such slack)
    assert all(b >= a - 1e-6 * abs(a) for a, b in zip(elbos, elbos[1:])), elbos
    assert all(b >= a - 1e-12 * abs(a) for a, b in zip(ref["elbo"], ref["elbo"][1:]))
    assert np.allclose(elbos, ref["elbo"], rtol=1e-5)
    Lam, eta = cavi.natural_parameters()
    assert relmax(host(Lam)[0], np.eye(M) + ref["G"][9]) < NAT_TOL and relmax(host(eta)[0], ref["g"][9]) < NAT_TOL
    if n == 1:  # the Bernoulli kind on the same data: the same sweeps
        bern = A.SparseCAVI(A.BernoulliLikelihood(), dev(Phi), dev(kd), dev(y.astype(np.uint8)), ctx=ctx)
        bern.run(10)
        cavi.check()
        assert relmax(host(cavi.m), host(bern.m)) < NAT_TOL and relmax(host(cavi.S), host(bern.S)) < NAT_TOL
    # 8. leave-one-out after the ten sweeps
    loo = cavi.loo()
    assert np.isfinite(loo.elpd) and np.isfinite(host(loo.logp)).all() and loo.n_bad == 0
    cdf, sf = cavi.loo_cdf()
    assert ((host(cdf) >= 0) & (host(cdf) <= 1)).all() and ((host(sf) >= 0) & (host(sf) <= 1)).all()


@pytest.mark.parametrize("M", [64, 200])
@pytest.mark.parametrize("n", [2, 1000])
def test_gibbs_sweep_against_the_reference_and_sharded(A, oracle, M, n):
    Phi, kd, y = sparse_problem(M, n, seed=4)
    lik = A.BinomialLikelihood(n)
    gctx = A.Context(0, seed=777)
    gib = A.SparseGibbs(lik, dev(Phi), dev(kd), dev(y), ctx=gctx, keep_points=True)
    gib.sweep()
    om, f = host(gib.omega)[:, 0], host(gib.f)[:, 0]
    assert np.isfinite(om).all() and (om > 0).all()
    beta, gamma = B.sampled_potential_precision(n, y.astype(np.float64), om)
    Phi_d = host(gib.plan.features())
    Gr, gr = oracle.accumulate(Phi_d, beta.astype(np.float32).astype(np.float64)[None], gamma.astype(np.float32).astype(np.float64)[None])
    assert relmax(host(gib.G), Gr) < 5e-6 and relmax(host(gib.g), gr) < 5e-6
    # two shards with their point offsets draw the single-process omega and f, bit for bit (contexts on the same seed and at the
    # same draw counter start from the same prior draw v: a function of the seed, M and the counter)
    for lo, hi in ((0, SPLIT), (SPLIT, N)):
        sctx = A.Context(0, seed=777)
        part = A.SparseGibbs(lik, dev(Phi[lo:hi]), dev(kd[lo:hi]), dev(y[lo:hi]), ctx=sctx, keep_points=True, point_offset=lo)
        part.sweep()
        assert np.array_equal(host(part.omega)[:, 0], om[lo:hi]) and np.array_equal(host(part.f)[:, 0], f[lo:hi])


def test_dense_gibbs_step_against_the_reference(A, oracle):
    import scipy.linalg as sla

    Nd, n = 300, 7
    rng = np.random.default_rng(31)
    x = np.sort(rng.uniform(-10, 10, size=Nd))
    K = np.exp(-0.5 * ((x[:, None] - x[None, :]) / 2.0) ** 2) + 1e-6 * np.eye(Nd)
    y = counts(rng, n, Nd, 2 * np.sin(0.7 * x))
    dctx = A.Context(0, seed=4242)
    dg = A.DenseGibbs(A.BinomialLikelihood(n), dev(K), dev(y), ctx=dctx)
    Lk = np.linalg.cholesky(K)
    for _ in range(2):
        dg.sweep()
        om = host(dg.omega)
        beta, gamma = B.sampled_potential_precision(n, y.astype(np.float64), om)
        z = oracle.randn(4242, 0, (dg.sweep_index | 0x80000000) & 0xFFFFFFFF, 2 * Nd)  # the step of oracle.dense_gibbs_step
        f0 = Lk @ z[:Nd]
        sg = np.sqrt(gamma)
        r = beta / sg - sg * f0 - z[Nd:]
        s = sla.cho_solve(sla.cho_factor(np.eye(Nd) + sg[:, None] * K * sg[None, :], lower=True), r)
        f = f0 + K @ (sg * s)
        assert np.abs(host(dg.f) - f).max() < 1e-6 * max(1.0, np.abs(f).max())


# ------------------------------------------------------------------------------------------ 5. predictive, cdf, quantiles
@pytest.fixture(scope="module")
def predictive_grid():
    """The domain grid and its float64 reference, computed once."""
    rows = []
    for n in (1, 7, 1000):
        for s in (1e-8, 0.1, 1.0, 10.0, 50.0):
            for mu in (-40.0, -3.0, 0.0, 3.0, 40.0):
                me, va = B.ref_moments_direct(n, mu, s * s)
                for y in sorted({0, 1, n // 2, n}):
                    lp, err = B.ref_logp(n, y, mu, s * s)
                    assert err < 1e-8
                    rows.append((n, s, mu, y, lp, me, va))
    return np.array(rows)


def test_predictive_over_the_domain(A, ctx, predictive_grid):
    g = predictive_grid
    worst = dict(logp=0.0, mean=0.0, var=0.0)
    for n in (1, 7, 1000):
        r = g[g[:, 0] == n]
        me, va, lp = (host(t) for t in A.predictive(A.BinomialLikelihood(n), (dev(r[:, 2]), dev(r[:, 1] ** 2)), dev(r[:, 3].astype(np.int32)), ctx=ctx))
        figs = dict(logp=np.abs(lp - r[:, 4]) / 1e-4, mean=np.abs(me - r[:, 5]) / (1e-5 * np.abs(r[:, 5]) + 1e-9),
                    var=np.abs(va - r[:, 6]) / (1e-5 * np.abs(r[:, 6]) + 1e-9))
        for k, v in figs.items():
            worst[k] = max(worst[k], float(v.max()))
            print(f"BINOMIAL predictive n = {n}: worst {k} = {v.max():.3e} of its bar (|logp err| max {np.abs(lp - r[:, 4]).max():.3e})")
    assert max(worst.values()) <= 1.0, worst


def test_zero_variance_is_the_binomial_mass_function(A, ctx):
    for n in (1, 7, 1000):
        mu = np.array([-40.0, -3.0, 0.0, 0.3, 3.0, 40.0])
        for y in sorted({0, 1, n // 2, n}):
            lp = host(A.predictive(A.BinomialLikelihood(n), (dev(mu), dev(np.zeros(6))), dev(np.full(6, y, dtype=np.int32)), ctx=ctx)[2])
            ref = np.array([B.loglik(n, y, m) for m in mu])
            assert np.allclose(lp, ref, rtol=1e-13, atol=1e-13), (n, y, lp - ref)


@pytest.mark.parametrize("n,mu,s", QUANTILE_CASES)
def test_cdf_and_quantiles(A, ctx, n, mu, s):
    lik = A.BinomialLikelihood(n)
    cdf_r, sf_r = B.cdf_all(n, mu, s)
    ys = np.arange(n + 1, dtype=np.int32)
    qf = (dev(np.full(n + 1, mu)), dev(np.full(n + 1, s * s)))
    cdf, sf = (host(t) for t in A.predictive_cdf(lik, qf, dev(ys), ctx=ctx))
    assert cdf[n] == 1.0 and sf[n] == 0.0  # exactly
    for got, want in ((cdf, cdf_r), (sf, sf_r)):
        assert np.abs(got - want).max() <= 1e-8, np.abs(got - want).max()
        big = want >= 1e-12
        assert (np.abs(got - want)[big] <= 1e-4 * want[big]).all()
    q = host(A.predictive_quantile(lik, (dev(np.array([mu])), dev(np.array([s * s]))), LEVELS, ctx=ctx))[0]
    assert [int(v) for v in q] == [B.quantile(cdf_r, p) for p in LEVELS]
    # thresholds outside the support
    c2, s2 = (host(t) for t in A.predictive_cdf(lik, (qf[0][:2], qf[1][:2]), dev(np.array([-1, n + 5], dtype=np.int32)), ctx=ctx))
    assert list(c2) == [0.0, 1.0] and list(s2) == [1.0, 0.0]


# ------------------------------------------------------------------------------------------ 6. draws of y
@pytest.mark.parametrize("n", [1, 7, 64, 65])
def test_draws_equal_the_headers_rule(A, oracle, n):
    """n = 64 and 65 sit on the two sides of the rule's switch from the sum of comparisons; at 65 the latents below reach both the
    inverse-cdf walk (n q < 10) and the transformed rejection."""
    T, Ns, point0, draw0, sweep = 3, 97, 2 ** 32 - 40, 65534, 11
    rng = np.random.default_rng([6, n])
    F = rng.uniform(-4, 4, size=(T, 1, Ns)).astype(np.float32)
    F[0, 0, :4] = (-30.0, 30.0, -2.5, 2.5)
    sctx = A.Context(0, seed=SEED)
    lik = A.BinomialLikelihood(n)
    got = host(A.sample_y(lik, dev(F), point0=point0, draw0=draw0, sweep=sweep, ctx=sctx))
    ref, margin = B.sample_y(oracle, n, F, SEED, point0, draw0, sweep)
    assert margin.min() > 1e-9, margin.min()  # no comparison within a libm difference of a tie
    assert np.array_equal(got, ref)
    assert got.min() >= 0 and got.max() <= n
    if n == 65:
        q = np.minimum(1 / (1 + np.exp(-F.astype(np.float64))), 1 / (1 + np.exp(F.astype(np.float64))))
        assert (n * q < B.BINOMIAL_WALK).any() and (n * q >= B.BINOMIAL_WALK).any()
    # chunks of draws and a two-way split of the points: the same integers
    a = host(A.sample_y(lik, dev(F[:1]), point0=point0, draw0=draw0, sweep=sweep, ctx=sctx))
    b = host(A.sample_y(lik, dev(F[1:]), point0=point0, draw0=draw0 + 1, sweep=sweep, ctx=sctx))
    assert np.array_equal(np.concatenate([a, b]), got)
    s1, s2 = A.Context(0, seed=SEED), A.Context(0, seed=SEED)
    s1.set_point_offset(point0)
    s2.set_point_offset(point0 + 50)
    left = host(A.sample_y(lik, dev(F[:, :, :50]), sweep=sweep, draw0=draw0, ctx=s1))
    right = host(A.sample_y(lik, dev(F[:, :, 50:]), sweep=sweep, draw0=draw0, ctx=s2))
    assert np.array_equal(np.concatenate([left, right], axis=1), got)


@pytest.mark.parametrize("n", [7, 65, 1000])
def test_draws_have_the_binomial_mean(A, n):
    T = 4096
    sctx = A.Context(0, seed=SEED + 1)
    for f in (-2.0, 0.4, 3.0):
        F = torch.full((T, 1, 1), f, dtype=torch.float32, device="cuda")
        y = host(A.sample_y(A.BinomialLikelihood(n), F, sweep=3, ctx=sctx)).astype(np.float64)
        assert y.min() >= 0 and y.max() <= n
        mean, var = B.ref_moments(n, float(np.float32(f)), 0.0)
        assert abs(y.mean() - mean) <= 6.0 * math.sqrt(var / T), (n, f, y.mean(), mean)


# ------------------------------------------------------------------------------------------ 7. expected log-likelihood
@pytest.mark.parametrize("n", [1, 7, 1000])
def test_expected_loglik_against_quadrature(A, ctx, n):
    rng = np.random.default_rng([7, n])
    m = 96
    mu, s = rng.uniform(-4, 4, size=m), np.exp(rng.uniform(np.log(0.05), np.log(3.0), size=m))
    var = s * s
    var[:3] = 0.0
    y = counts(rng, n, m, mu)
    lik = A.BinomialLikelihood(n)
    tot, grad, ell, dell = A.expected_loglik(lik, dev(mu), dev(var), dev(y), ctx=ctx, per_point=True)
    ell = host(ell)
    ref = B.expected_loglik(n, y.astype(np.float64), mu, var)
    fig = (np.abs(ell - ref) / np.maximum(1.0, np.abs(ref))).max()
    print(f"BINOMIAL expected_loglik n = {n}: worst |device - quad| / max(1, |quad|) = {fig:.3e}")
    assert fig <= ELL_TOL
    assert tot == pytest.approx(ell.sum(), rel=1e-12) and dell is None and (grad is None or grad.numel() == 0)
    if n == 1:
        eb = host(A.expected_loglik(A.BernoulliLikelihood(), dev(mu), dev(var), dev(y.astype(np.uint8)), ctx=ctx, per_point=True)[2])
        assert (np.abs(ell - eb) / np.maximum(1.0, np.abs(eb))).max() <= ELL_TOL
