"""GPU tests of the asymmetric Laplace likelihood (AGPL_LIK_ASYMLAPLACE = 9; run with -m gpu on an MI355X) through every layer that
takes a likelihood descriptor, against tests/asymlaplace_reference.py (float64 numpy, held by tests/test_asymlaplace_reference_cpu.py
to mpmath and quadrature; the oracle does not know the kind) and against the Laplace kind at beta = 2 sigma, which the oracle checks.

Bars, as tests/test_gpu_binomial.py lists where the project states them: float64 operators 1e-12 (the auxiliary posterior), 1e-11
(potentials, logtilt, expected_logtilt), 1e-10 (KL), aug_loglik 1e-9, float32 operators 3e-6 / 3e-5 (tests/test_gpu_parity.py);
natural parameters after ten sweeps 1e-5 of max|ref|; Gibbs G, g 5e-6 and the dense step 1e-6 max(1, max|f|)
(tests/test_gpu_parity.py); log p 1e-4 absolute, moments 1e-5 relative + 1e-9 absolute (tests/test_gpu_predictive_domain.py); cdf and
sf 1e-8 and 1e-4 relative from 1e-12 up, quantiles by the residual |F_ref(q) - p| <= 2e-8 (tests/test_gpu_quantile.py); expected
log-likelihood and gradient 10 x 2.526e-12 of max(1, |ref|), the first Adam step within 1e-6 of lr (tests/test_gpu_likgrad.py);
leave-one-out: the cavity's bar of tests/test_gpu_loo.py (T_v = 2e-5 max var, T_m = 2e-5 max(1, max|mu|) carried through the
cavity's formulas), carried on through the predictive's derivatives to log p and to the probability integral transform."""
import ctypes as C
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import asymlaplace_reference as R  # noqa: E402

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

SEED = 20261021
N = 777
SPLIT = 400
NPRED = (1, 2, 7, 1000)
NAT_TOL = 1e-5
ELL_TOL = 10.0 * 2.526e-12
TAUS = (0.05, 0.9)


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
    """(y, f, mu, var, omega): real observations with a few far from the latent, in float32-exact values for y."""
    y = (rng.normal(size=n) * 1.5).astype(np.float32).astype(np.float64)
    y[:3] = (-9.0, 0.0, 11.0)
    return y, rng.normal(size=n), rng.normal(size=n) * 1.2, rng.uniform(0.05, 2.0, size=n), rng.uniform(0.05, 4.0, size=n)


def sparse_problem(M, tau, seed=3):
    """Features with |phi|^2 ~ 1 (one largest entry shared by both halves of the two-way split, as tests/test_gpu_binomial.py
    explains), a positive residual, a smooth truth, asymmetric-Laplace noise about it and a non-zero prior mean."""
    rng = np.random.default_rng([seed, M, int(100 * tau)])
    Phi = (rng.normal(size=(N, M)) / math.sqrt(M)).astype(np.float32)
    assert np.abs(Phi).max() < 0.9 or M < 16
    big = max(0.75, float(np.ceil(np.abs(Phi).max() * 4) / 4))
    Phi[0, 0] = Phi[SPLIT, 0] = big
    kd = rng.uniform(0.05, 0.3, size=N).astype(np.float32)
    mu0 = (0.3 * np.sin(np.arange(N) / 40.0)).astype(np.float32)
    f = Phi.astype(np.float64) @ rng.normal(size=M) + mu0
    y = R.inverse_cdf(0.4, tau, f, rng.uniform(size=N)).astype(np.float32)
    return Phi, kd, y, mu0


# ------------------------------------------------------------------------------------------ 1. accepted where it was refused
def test_every_entry_point_accepts_the_kind(A, ctx):
    """Each call below raised ArgumentError (AGPL_ERR_INVALID_ARGUMENT, unknown likelihood kind 9) before the kind existed."""
    rng = np.random.default_rng(1)
    lik = A.AsymmetricLaplaceLikelihood(0.9, 0.7)
    yh, fh, muh, varh, _ = points(rng)
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
    Phi, kd, yy, _ = sparse_problem(64, 0.9)
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
    # (not the first points: y = 0 there meets the chain's start f = 0, where the draw of omega has an infinite mean, as Laplace's has)
    A.DenseGibbs(lik, dev(K), dev(yh[3:67]), ctx=ctx).sweep()  # agpl_dense_gibbs_step
    assert all(np.isfinite(host(t)).all() for t in A.predictive(lik, (mu, var), y, ctx=ctx))
    assert all(np.isfinite(host(t)).all() for t in A.predictive_cdf(lik, (mu, var), y, ctx=ctx))
    assert np.isfinite(host(A.predictive_quantile(lik, (mu, var), (0.1, 0.5, 0.9), ctx=ctx))).all()
    tot, grad = A.expected_loglik(lik, mu, var, y, ctx=ctx)[:2]
    assert np.isfinite(tot) and grad.numel() == 1
    assert np.isfinite(host(A.sample_y(lik, f.to(torch.float32).reshape(1, 1, N), sweep=2, ctx=ctx))).all()
    ctx.synchronize()


# ------------------------------------------------------------------------------------------ 2. invalid (sigma, tau)
@pytest.mark.parametrize("sigma,tau", [(0.0, 0.5), (-1.0, 0.5), (math.inf, 0.5), (math.nan, 0.5), (1.0, 0.0), (1.0, 1.0), (1.0, -0.2),
                                       (1.0, 1.5), (1.0, math.nan)])
def test_bad_parameters_are_refused_with_a_message(A, ctx, sigma, tau):
    lik = A.AsymmetricLaplaceLikelihood(tau, sigma)
    z = torch.zeros(4, dtype=torch.float64, device="cuda")
    out = torch.full((4,), 7.0, dtype=torch.float64, device="cuda")
    calls = [lambda: A.aux_sample(lik, z, z, ctx=ctx, sweep=1), lambda: A.aux_posterior(lik, z, (z, z + 1), ctx=ctx),
             lambda: A.predictive(lik, (z, z + 1), z, ctx=ctx), lambda: A.predictive_cdf(lik, (z, z + 1), z, ctx=ctx),
             lambda: A.predictive_quantile(lik, (z, z + 1), (0.5,), ctx=ctx), lambda: A.expected_loglik(lik, z, z + 1, z, ctx=ctx),
             lambda: A.sample_y(lik, z.to(torch.float32).reshape(1, 1, 4), sweep=1, ctx=ctx)]
    for call in calls:
        with pytest.raises(A.ArgumentError, match="AsymmetricLaplace needs"):
            call()
    # no device work follows a refusal: the output of a raw call is untouched
    d = lik.desc()
    p = lambda t: C.c_void_p(t.data_ptr())
    with pytest.raises(A.ArgumentError):
        ctx.call("agpl_aux_posterior", C.byref(d), C.c_int32(1), C.c_int64(4), p(z), p(z), p(z + 1), p(out), C.c_void_p(0), C.c_void_p(0))
    ctx.synchronize()
    assert (host(out) == 7.0).all()


# ------------------------------------------------------------------------------------------ 3. tau does not reach omega
@pytest.mark.parametrize("sigma", [0.25, 3.0])
@pytest.mark.parametrize("tau", [0.01, 0.3, 0.5, 0.99])
def test_tau_does_not_reach_the_auxiliary_variable(A, tau, sigma):
    """The same context seed, f and y: the draws of omega (and the uniforms they consumed) and the out1 of aux_posterior in both
    precisions are the Laplace kind's at beta = 2 sigma byte for byte, with a point offset set."""
    rng = np.random.default_rng([3, int(1000 * tau), int(100 * sigma)])
    ald, lap = A.AsymmetricLaplaceLikelihood(tau, sigma), A.LaplaceLikelihood(2.0 * sigma)
    yh, fh, muh, varh, _ = points(rng)
    y, f, mu, var = dev(yh), dev(fh), dev(muh), dev(varh)
    c1, c2 = A.Context(0, seed=SEED), A.Context(0, seed=SEED)
    c1.set_point_offset(12345)
    c2.set_point_offset(12345)
    o1, u1, t1 = A.aux_sample_(A.init_aux_variables(ald, N, ctx=c1), ald, y, f, ctx=c1, sweep=5, stats=True)
    o2, u2, t2 = A.aux_sample_(A.init_aux_variables(lap, N, ctx=c2), lap, y, f, ctx=c2, sweep=5, stats=True)
    assert torch.equal(o1.ω, o2.ω) and torch.equal(u1, u2) and torch.equal(t1, t2)
    for dt in (torch.float64, torch.float32):
        q1 = A.aux_posterior(ald, y.to(dt), (mu.to(dt), var.to(dt)), ctx=c1)
        q2 = A.aux_posterior(lap, y.to(dt), (mu.to(dt), var.to(dt)), ctx=c2)
        assert q1.inds[0]["μ"].dtype == dt and torch.equal(q1.inds[0]["μ"], q2.inds[0]["μ"])
        # ... and so is the precision, which is 2 out1 for both kinds
        assert torch.equal(A.expected_auglik_precision(ald, q1, y.to(dt), ctx=c1)[0], A.expected_auglik_precision(lap, q2, y.to(dt), ctx=c2)[0])
    assert A.aux_prior_logpdf(ald, o1, y, ctx=c1) == A.aux_prior_logpdf(lap, o2, y, ctx=c2)
    assert A.aux_kldivergence(ald, q1, y, ctx=c1) == A.aux_kldivergence(lap, q2, y, ctx=c2)


# ------------------------------------------------------------------------------------------ 4. tau = 1/2 is Laplace
@pytest.mark.parametrize("sigma", [0.25, 3.0])
def test_tau_half_is_the_laplace_kind(A, ctx, sigma):
    """Byte-identical pairs (kappa = 0 is subtracted exactly, sigma / (1 - tau) = 2 sigma exactly): omega, out1, both potentials and
    precisions in both precisions, the KL, the prior density, the predictive mean and the draws of y.  The tilts add log(4 tau (1 - tau))
    = 0 and kappa d = 0 after Laplace's expression and the closed forms multiply by a = tau / sigma where Laplace divides by beta:
    those are held to the operator bars."""
    rng = np.random.default_rng([4, int(100 * sigma)])
    ald, lap = A.AsymmetricLaplaceLikelihood(0.5, sigma), A.LaplaceLikelihood(2.0 * sigma)
    yh, fh, muh, varh, _ = points(rng)
    y, f, mu, var = dev(yh), dev(fh), dev(muh), dev(varh)
    c1, c2 = A.Context(0, seed=SEED), A.Context(0, seed=SEED)
    O1, O2 = A.aux_sample(ald, y, f, ctx=c1, sweep=9), A.aux_sample(lap, y, f, ctx=c2, sweep=9)
    assert torch.equal(O1.ω, O2.ω)
    for a, b in zip(A.auglik_potential_and_precision(ald, O1, y, ctx=c1), A.auglik_potential_and_precision(lap, O2, y, ctx=c2)):
        assert torch.equal(a[0], b[0])
    assert A.logtilt(ald, O1, y, f, ctx=c1) == pytest.approx(A.logtilt(lap, O2, y, f, ctx=c2), rel=1e-11)
    assert A.aug_loglik(ald, O1, y, f, ctx=c1) == pytest.approx(A.aug_loglik(lap, O2, y, f, ctx=c2), rel=1e-9)
    for dt in (torch.float64, torch.float32):
        q1 = A.aux_posterior(ald, y.to(dt), (mu.to(dt), var.to(dt)), ctx=c1)
        q2 = A.aux_posterior(lap, y.to(dt), (mu.to(dt), var.to(dt)), ctx=c2)
        for a, b in zip(A.expected_auglik_potential_and_precision(ald, q1, y.to(dt), ctx=c1),
                        A.expected_auglik_potential_and_precision(lap, q2, y.to(dt), ctx=c2)):
            assert torch.equal(a[0], b[0])
    assert A.expected_logtilt(ald, q1, y, (mu, var), ctx=c1) == pytest.approx(A.expected_logtilt(lap, q2, y, (mu, var), ctx=c2), rel=1e-11)
    assert A.aux_kldivergence(ald, q1, y, ctx=c1) == A.aux_kldivergence(lap, q2, y, ctx=c2)
    # the prediction end
    (m1, v1, l1), (m2, v2, l2) = A.predictive(ald, (mu, var), y, ctx=c1), A.predictive(lap, (mu, var), y, ctx=c2)
    assert torch.equal(m1, m2) and np.allclose(host(v1), host(v2), rtol=1e-12, atol=0) and np.allclose(host(l1), host(l2), rtol=1e-12, atol=1e-12)
    for a, b in zip(A.predictive_cdf(ald, (mu, var), y, ctx=c1), A.predictive_cdf(lap, (mu, var), y, ctx=c2)):
        assert np.allclose(host(a), host(b), rtol=1e-12, atol=1e-15)
    probs = (0.01, 0.1, 0.5, 0.9, 0.99)
    q1, q2 = host(A.predictive_quantile(ald, (mu, var), probs, ctx=c1)), host(A.predictive_quantile(lap, (mu, var), probs, ctx=c2))
    for j, pj in enumerate(probs):  # both answers solve the Laplace kind's equation to the quantile test's residual
        for q in (q1, q2):
            c, s = (host(t) for t in A.predictive_cdf(lap, (mu, var), dev(q[:, j]), ctx=c2))
            assert np.abs(c - pj).max() <= 2e-8 and np.abs(s - (1.0 - pj)).max() <= 2e-8
    t1, g1, e1, d1 = A.expected_loglik(ald, mu, var, y, ctx=c1, per_point=True)
    t2, g2, e2, d2 = A.expected_loglik(lap, mu, var, y, ctx=c2, per_point=True)
    assert (np.abs(host(e1) - host(e2)) <= ELL_TOL * np.maximum(1.0, np.abs(host(e2)))).all()
    assert (np.abs(host(d1) - host(d2)) <= ELL_TOL * np.maximum(1.0, np.abs(host(d2)))).all()  # d / d log sigma = d / d log beta
    assert t1 == pytest.approx(t2, rel=1e-12) and float(g1[0]) == pytest.approx(float(g2[0]), rel=1e-12)
    F = dev(rng.uniform(-3, 3, size=(3, 1, 97)).astype(np.float32))
    assert torch.equal(A.sample_y(ald, F, point0=77, draw0=5, sweep=11, ctx=c1), A.sample_y(lap, F, point0=77, draw0=5, sweep=11, ctx=c2))
    # ten sweeps
    Phi, kd, yy, mu0 = sparse_problem(64, 0.5)
    s1 = A.SparseCAVI(ald, dev(Phi), dev(kd), dev(yy), mu0=dev(mu0[None]), ctx=c1)
    s2 = A.SparseCAVI(lap, dev(Phi), dev(kd), dev(yy), mu0=dev(mu0[None]), ctx=c2)
    s1.run(10)
    s2.run(10)
    assert relmax(host(s1.G), host(s2.G)) < NAT_TOL and relmax(host(s1.g), host(s2.g)) < NAT_TOL


# ------------------------------------------------------------------------------------------ 5. tau != 1/2 against the reference
@pytest.mark.parametrize("tau", TAUS)
def test_operators_against_the_reference(A, ctx, tau):
    sigma = 0.7
    rng = np.random.default_rng([5, int(100 * tau)])
    lik = A.AsymmetricLaplaceLikelihood(tau, sigma)
    y, f, mu, var, _ = points(rng)
    Om = A.aux_sample(lik, dev(y), dev(f), ctx=ctx, sweep=7)
    om = host(Om.ω)
    beta, gamma = A.auglik_potential_and_precision(lik, Om, dev(y), ctx=ctx)
    rb, rg = R.sampled_potential_precision(sigma, tau, y, om)
    assert np.allclose(host(beta[0]), rb, rtol=1e-10, atol=1e-14) and np.array_equal(host(gamma[0]), rg)
    assert A.logtilt(lik, Om, dev(y), dev(f), ctx=ctx) == pytest.approx(R.logtilt(sigma, tau, y, om, f), rel=1e-11)
    assert A.aux_prior_logpdf(lik, Om, dev(y), ctx=ctx) == pytest.approx(R.aux_prior_logpdf(sigma, om), rel=1e-11)
    assert A.aug_loglik(lik, Om, dev(y), dev(f), ctx=ctx) == pytest.approx(R.aug_loglik(sigma, tau, y, om, f), rel=1e-9)
    o1_ref = R.aux_posterior(sigma, y, mu, var)
    for dt, rtol in ((torch.float64, 1e-12), (torch.float32, 3e-6)):
        q = A.aux_posterior(lik, dev(y, dt), (dev(mu, dt), dev(var, dt)), ctx=ctx)
        assert np.allclose(host(q.inds[0]["μ"]).astype(np.float64), o1_ref, rtol=rtol, atol=1e-30)
        bt, gm = A.expected_auglik_potential_and_precision(lik, q, dev(y, dt), ctx=ctx)
        rb, rg = R.expected_potential_precision(sigma, tau, y, o1_ref)
        assert np.allclose(host(bt[0]).astype(np.float64), rb, rtol=10 * rtol, atol=1e-6 if dt == torch.float32 else 1e-14)
        assert np.allclose(host(gm[0]).astype(np.float64), rg, rtol=10 * rtol, atol=0)
        if dt == torch.float64:
            qf = (dev(mu), dev(var))
            assert A.expected_logtilt(lik, q, dev(y), qf, ctx=ctx) == pytest.approx(R.expected_logtilt(sigma, tau, y, o1_ref, mu, var), rel=1e-11)
            assert A.aux_kldivergence(lik, q, dev(y), ctx=ctx) == pytest.approx(R.aux_kl(sigma, o1_ref), rel=1e-10)
            want = R.expected_logtilt(sigma, tau, y, o1_ref, mu, var) + R.aux_kl(sigma, o1_ref)  # generic.jl:52-54, the reference's sign
            assert A.expected_aug_loglik(lik, q, dev(y), qf, ctx=ctx) == pytest.approx(want, rel=1e-11)


@pytest.mark.parametrize("M", [5, 300])
@pytest.mark.parametrize("tau", TAUS)
def test_cavi_sweeps_against_the_reference(A, ctx, M, tau):
    """Ten sweeps with a prior mean, M = 5 and 300 (one and two 256-blocks of the padded plan): natural parameters, the fused kernel's
    ELBO terms and the operator kernels' elbo(), then leave-one-out at the fitted q(v)."""
    sigma = 0.4
    Phi, kd, y, mu0 = sparse_problem(M, tau)
    lik = A.AsymmetricLaplaceLikelihood(tau, sigma)
    cavi = A.SparseCAVI(lik, dev(Phi), dev(kd), dev(y), mu0=dev(mu0[None]), ctx=ctx, keep_points=True, track_elbo=True)
    Phi_d = host(cavi.plan.features()).astype(np.float64)  # what the plan's images hold
    assert np.abs(Phi_d - Phi).max() <= 2.0 ** -21 * np.abs(Phi).max()
    ref = R.cavi_sweeps(sigma, tau, Phi_d, host(cavi.plan.resid).astype(np.float64), y, 11, mu0=mu0)
    for it in range(10):
        e_ops = cavi.elbo()
        cavi.sweep()
        assert e_ops == pytest.approx(ref["elbo"][it], rel=1e-5)
        assert cavi.elbo_entering() == pytest.approx(ref["elbo"][it], rel=1e-5)  # agpl_fused_point_kernel<true, 9>
        if it in (0, 9):
            figs = relmax(host(cavi.G)[0], ref["G"][it]), relmax(host(cavi.g)[0], ref["g"][it])
            print(f"ASYMLAPLACE CAVI M = {M} tau = {tau} sweep {it + 1}: G {figs[0]:.3e}, g {figs[1]:.3e} of max|ref|")
            assert max(figs) < NAT_TOL, (it, figs)
    Lam, eta = cavi.natural_parameters()
    assert relmax(host(Lam)[0], np.eye(M) + ref["G"][9]) < NAT_TOL and relmax(host(eta)[0], ref["g"][9]) < NAT_TOL
    # 8. leave-one-out: the rule of include/agpl_loo.h on the reference's sites, the predictive of the reference at that cavity
    import loo_reference as LR

    gam, bet, d = ref["gamma"][9][None], ref["beta"][9][None], host(cavi.plan.resid).astype(np.float64)
    cm, cv, h = LR.closed_form(Phi_d, d, gam, bet, mu0=mu0[None].astype(np.float64))
    # the cavity's bars of tests/test_gpu_loo.py::test_end_to_end_against_the_refit ...
    mu_m, var_m = ref["mu"][10][None], ref["var"][10][None]
    Tv, Tm = 2e-5 * np.abs(var_m).max(), 2e-5 * max(1.0, np.abs(mu_m).max())
    q, a = var_m - d[None], mu_m - mu0[None]
    bar_v = Tv / (1 - h) ** 2
    bar_m = (Tm + np.abs(bet) * Tv) / (1 - h) + np.abs(a - bet * q) * gam * Tv / (1 - h) ** 2
    # ... carried through the predictive: |d log p / d mu| <= r = max(tau, 1 - tau) / sigma, |d log p / d var| <= r^2 / 2 (the
    # density solves the heat equation in var), |dF / d mu| = p <= tau (1 - tau) / sigma =: p0, |dF / d var| = |p'| / 2 <= r p0 / 2
    r, p0 = max(tau, 1.0 - tau) / sigma, tau * (1.0 - tau) / sigma
    bar_lp, bar_F = (r * bar_m + 0.5 * r * r * bar_v)[0], (p0 * bar_m + 0.5 * r * p0 * bar_v)[0]
    lp_ref = np.array([R.logp(sigma, tau, float(y[i]), cm[0, i], cv[0, i]) for i in range(N)])
    loo = cavi.loo()
    lp = host(loo.logp)
    print(f"ASYMLAPLACE LOO M = {M} tau = {tau}: elpd {loo.elpd:.6f} ref {lp_ref.sum():.6f}, worst |logp - ref| / bar {(np.abs(lp - lp_ref) / bar_lp).max():.3e}")
    assert loo.n_bad == 0 and (np.abs(lp - lp_ref) <= bar_lp).all() and abs(loo.elpd - lp_ref.sum()) <= bar_lp.sum()
    assert abs(loo.elpd - float(np.sum(lp.astype(np.longdouble)))) <= N * 2.0 ** -53 * np.abs(lp).sum()  # tests/test_gpu_loo.py
    cdf, sf = (host(t) for t in cavi.loo_cdf())
    pit = np.array([R.cdf(sigma, tau, float(y[i]), cm[0, i], cv[0, i]) for i in range(N)])
    assert (np.abs(cdf - pit[:, 0]) <= bar_F).all() and (np.abs(sf - pit[:, 1]) <= bar_F).all()


@pytest.mark.parametrize("M", [5, 300])
@pytest.mark.parametrize("tau", TAUS)
def test_gibbs_sweep_against_the_reference_and_sharded(A, oracle, M, tau):
    sigma = 0.4
    Phi, kd, y, mu0 = sparse_problem(M, tau, seed=4)
    lik = A.AsymmetricLaplaceLikelihood(tau, sigma)
    gctx = A.Context(0, seed=777)
    gib = A.SparseGibbs(lik, dev(Phi), dev(kd), dev(y), mu0=dev(mu0[None]), ctx=gctx, keep_points=True)
    gib.sweep()
    om, f = host(gib.omega)[:, 0], host(gib.f)[:, 0]
    assert np.isfinite(om).all() and (om > 0).all()
    beta, gamma = R.sampled_potential_precision(sigma, tau, y.astype(np.float64), om)
    Phi_d = host(gib.plan.features())
    Gr, gr = oracle.accumulate(Phi_d, beta.astype(np.float32).astype(np.float64)[None], gamma.astype(np.float32).astype(np.float64)[None])
    assert relmax(host(gib.G), Gr) < 5e-6 and relmax(host(gib.g), gr) < 5e-6
    for lo, hi in ((0, SPLIT), (SPLIT, N)):  # two shards with their point offsets: the single-process omega and f, bit for bit
        sctx = A.Context(0, seed=777)
        part = A.SparseGibbs(lik, dev(Phi[lo:hi]), dev(kd[lo:hi]), dev(y[lo:hi]), mu0=dev(mu0[None, lo:hi]), ctx=sctx, keep_points=True,
                             point_offset=lo)
        part.sweep()
        assert np.array_equal(host(part.omega)[:, 0], om[lo:hi]) and np.array_equal(host(part.f)[:, 0], f[lo:hi])


@pytest.mark.parametrize("tau", TAUS)
def test_dense_gibbs_step_against_the_reference(A, oracle, tau):
    import scipy.linalg as sla

    Nd, sigma = 300, 0.4
    rng = np.random.default_rng([31, int(100 * tau)])
    x = np.sort(rng.uniform(-10, 10, size=Nd))
    K = np.exp(-0.5 * ((x[:, None] - x[None, :]) / 2.0) ** 2) + 1e-6 * np.eye(Nd)
    y = R.inverse_cdf(sigma, tau, 2 * np.sin(0.7 * x), rng.uniform(size=Nd))
    dctx = A.Context(0, seed=4242)
    dg = A.DenseGibbs(A.AsymmetricLaplaceLikelihood(tau, sigma), dev(K), dev(y), ctx=dctx)
    Lk = np.linalg.cholesky(K)
    for _ in range(2):
        dg.sweep()
        om = host(dg.omega)
        beta, gamma = R.sampled_potential_precision(sigma, tau, y, om)
        z = oracle.randn(4242, 0, (dg.sweep_index | 0x80000000) & 0xFFFFFFFF, 2 * Nd)  # the step of oracle.dense_gibbs_step
        f0 = Lk @ z[:Nd]
        sg = np.sqrt(gamma)
        r = beta / sg - sg * f0 - z[Nd:]
        s = sla.cho_solve(sla.cho_factor(np.eye(Nd) + sg[:, None] * K * sg[None, :], lower=True), r)
        f = f0 + K @ (sg * s)
        assert np.abs(host(dg.f) - f).max() < 1e-6 * max(1.0, np.abs(f).max())


@pytest.mark.parametrize("n", NPRED)
@pytest.mark.parametrize("tau", TAUS)
def test_predictive_against_the_reference(A, ctx, tau, n):
    """Moments, log p, cdf, upper tail, quantiles and the expected log-likelihood with its gradient at n prediction points."""
    sigma = 0.7
    rng = np.random.default_rng([6, int(100 * tau), n])
    lik = A.AsymmetricLaplaceLikelihood(tau, sigma)
    mu, var, y = rng.normal(size=n) * 2.0, np.exp(rng.uniform(np.log(1e-3), np.log(9.0), size=n)), rng.normal(size=n) * 3.0
    var[0] = 0.0
    qf = (dev(mu), dev(var))
    me, va, lp = (host(t) for t in A.predictive(lik, qf, dev(y), ctx=ctx))
    rme, rva = R.moments(sigma, tau, mu, var)
    assert (np.abs(me - rme) <= 1e-5 * np.abs(rme) + 1e-9).all() and (np.abs(va - rva) <= 1e-5 * np.abs(rva) + 1e-9).all()
    assert np.abs(lp - np.array([R.logp(sigma, tau, y[i], mu[i], var[i]) for i in range(n)])).max() <= 1e-4
    cdf, sf = (host(t) for t in A.predictive_cdf(lik, qf, dev(y), ctx=ctx))
    ref = np.array([R.cdf(sigma, tau, y[i], mu[i], var[i]) for i in range(n)])
    for got, want in ((cdf, ref[:, 0]), (sf, ref[:, 1])):
        assert np.abs(got - want).max() <= 1e-8
        big = want >= 1e-12
        assert (np.abs(got - want)[big] <= 1e-4 * want[big]).all()
    probs = (0.001, 0.05, 0.5, 0.9, 0.999)
    q = host(A.predictive_quantile(lik, qf, probs, ctx=ctx))
    assert q.shape == (n, len(probs)) and np.isfinite(q).all() and (np.diff(q, axis=1) >= 0).all()
    worst = 0.0
    for i in range(min(n, 64)):
        for j, pj in enumerate(probs):
            c, s = R.cdf(sigma, tau, float(q[i, j]), mu[i], var[i])
            worst = max(worst, abs(c - pj) if pj <= 0.5 else abs(s - (1.0 - pj)))
    print(f"ASYMLAPLACE quantiles tau = {tau} n = {n}: worst |F_ref(q) - p| = {worst:.3e}")
    assert worst <= 2e-8
    tot, grad, ell, dell = A.expected_loglik(lik, dev(mu), dev(var), dev(y), ctx=ctx, per_point=True)
    rell, rdell = R.expected_loglik(sigma, tau, y, mu, var)
    fig = max((np.abs(host(ell) - rell) / np.maximum(1.0, np.abs(rell))).max(), (np.abs(host(dell)[:, 0] - rdell) / np.maximum(1.0, np.abs(rdell))).max())
    print(f"ASYMLAPLACE expected_loglik tau = {tau} n = {n}: worst |device - ref| / max(1, |ref|) = {fig:.3e}")
    assert fig <= ELL_TOL
    assert tot == pytest.approx(rell.sum(), rel=1e-11, abs=1e-11) and float(grad[0]) == pytest.approx(rdell.sum(), rel=1e-11, abs=1e-11)


# ------------------------------------------------------------------------------------------ 6. predictive edges
def test_predictive_edges_against_mpmath(A, ctx):
    """The CPU test's grid (var = 0; var = 1e4 with sigma = 1e-3; |d| at 40 scale units on both sides; tau = 0.01 and 0.99), point
    by point against its 50-digit values."""
    g = R.grid()
    worst = dict(logp=0.0, tail=0.0, rel=0.0)
    for sigma in R.SIGMAS:
        for tau in R.TAUS:
            r = g[(g[:, 0] == sigma) & (g[:, 1] == tau)]
            lik = A.AsymmetricLaplaceLikelihood(tau, sigma)
            qf = (dev(np.full(len(r), R.GRID_MU)), dev(r[:, 2]))
            lp = host(A.predictive(lik, qf, dev(r[:, 3]), ctx=ctx)[2])
            worst["logp"] = max(worst["logp"], float(np.abs(lp - r[:, 4]).max()))
            for got, want in zip((host(t) for t in A.predictive_cdf(lik, qf, dev(r[:, 3]), ctx=ctx)), (r[:, 5], r[:, 6])):
                worst["tail"] = max(worst["tail"], float(np.abs(got - want).max()))
                big = want >= 1e-12
                worst["rel"] = max(worst["rel"], float((np.abs(got - want)[big] / want[big]).max()))
    print(f"ASYMLAPLACE edges, {len(g)} points: worst |log p - mpmath| {worst['logp']:.3e}, tails {worst['tail']:.3e} absolute, "
          f"{worst['rel']:.3e} relative from 1e-12 up")
    assert worst["logp"] <= 1e-4 and worst["tail"] <= 1e-8 and worst["rel"] <= 1e-4


def test_conventions_are_the_laplace_kinds(A, ctx):
    """A non-finite y and a bad marginal (NaN mean, negative variance) give what the Laplace kind gives, output for output."""
    ald, lap = A.AsymmetricLaplaceLikelihood(0.2, 0.5), A.LaplaceLikelihood(1.0)
    mu = dev(np.array([0.3, 0.3, 0.3, 0.3, math.nan, 0.3, 0.3, 0.3]))
    var = dev(np.array([1.0, 1.0, 1.0, 0.0, 1.0, -1.0, 0.0, 0.0]))
    y = dev(np.array([math.inf, -math.inf, math.nan, 0.1, 0.1, 0.1, math.inf, math.nan]))
    kind = lambda a: np.where(np.isnan(a), 0, np.where(np.isposinf(a), 1, np.where(np.isneginf(a), 2, 3)))
    for fn in (lambda l: A.predictive(l, (mu, var), y, ctx=ctx), lambda l: A.predictive_cdf(l, (mu, var), y, ctx=ctx),
               lambda l: A.expected_loglik(l, mu, var, y, ctx=ctx, per_point=True)[2:]):
        for a, b in zip(fn(ald), fn(lap)):
            assert np.array_equal(kind(host(a)), kind(host(b))), (host(a), host(b))
    c, s = (host(t) for t in A.predictive_cdf(ald, (mu, var), y, ctx=ctx))
    assert (c[0], s[0], c[1], s[1]) == (1.0, 0.0, 0.0, 1.0)
    q = host(A.predictive_quantile(ald, (mu, var), (0.5,), ctx=ctx))[:, 0]
    assert np.isnan(q[4]) and np.isnan(q[5]) and np.isfinite(q[:4]).all()


# ------------------------------------------------------------------------------------------ 7. draws of y
@pytest.mark.parametrize("tau", [0.05, 0.5, 0.9])
def test_draws_are_the_inverse_cdf_of_the_streams_uniform(A, oracle, tau):
    from sample_y_reference import Stream

    sigma = 0.7
    T, Ns, point0, draw0, sweep = 3, 97, 2 ** 32 - 40, 65534, 11
    rng = np.random.default_rng([7, int(100 * tau)])
    F = rng.uniform(-4, 4, size=(T, 1, Ns)).astype(np.float32)
    F[0, 0, 0] = np.nan
    sctx = A.Context(0, seed=SEED)
    lik = A.AsymmetricLaplaceLikelihood(tau, sigma)
    got = host(A.sample_y(lik, dev(F), point0=point0, draw0=draw0, sweep=sweep, ctx=sctx))
    u = np.array([[Stream(oracle, SEED, point0 + i, sweep, draw0 + t).u01() for i in range(Ns)] for t in range(T)])
    ref = R.inverse_cdf(sigma, tau, F[:, 0, :].astype(np.float64), u)
    assert np.isnan(got[0, 0]) and got.dtype == np.float64
    ok = np.isfinite(ref)
    # 4 ulp of the sum's larger operand: y = f + t is rounded once, t carries the few ulp of log1p, and where f and t nearly cancel
    # an ulp of y itself says nothing about either
    f64 = F[:, 0, :].astype(np.float64)
    ulp = np.spacing(np.maximum(np.abs(ref), np.maximum(np.abs(f64), np.abs(ref - f64))))
    print(f"ASYMLAPLACE draws tau = {tau}: worst |device - reference| = {np.nanmax(np.abs(got - ref)[ok] / ulp[ok]):.2f} ulp")
    assert ok.sum() == T * Ns - 1 and (np.abs(got - ref)[ok] <= 4.0 * ulp[ok]).all()
    # chunks of draws and a two-way split of the points: the same bytes
    a = host(A.sample_y(lik, dev(F[:1]), point0=point0, draw0=draw0, sweep=sweep, ctx=sctx))
    b = host(A.sample_y(lik, dev(F[1:]), point0=point0, draw0=draw0 + 1, sweep=sweep, ctx=sctx))
    assert np.concatenate([a, b]).tobytes() == got.tobytes()
    s1, s2 = A.Context(0, seed=SEED), A.Context(0, seed=SEED)
    s1.set_point_offset(point0)
    s2.set_point_offset(point0 + 50)
    left = host(A.sample_y(lik, dev(F[:, :, :50]), sweep=sweep, draw0=draw0, ctx=s1))
    right = host(A.sample_y(lik, dev(F[:, :, 50:]), sweep=sweep, draw0=draw0, ctx=s2))
    assert np.concatenate([left, right], axis=1).tobytes() == got.tobytes()


@pytest.mark.parametrize("tau", [0.01, 0.3, 0.9])
def test_the_share_of_draws_below_the_latent_is_tau(A, tau):
    T = 200000
    sctx = A.Context(0, seed=SEED + 1)
    F = torch.full((T, 1, 1), 0.4, dtype=torch.float32, device="cuda")
    y = host(A.sample_y(A.AsymmetricLaplaceLikelihood(tau, 1.3), F, sweep=3, ctx=sctx))
    share = float(np.mean(y < float(np.float32(0.4))))
    assert abs(share - tau) <= 5.0 * math.sqrt(tau * (1.0 - tau) / T), (tau, share)


# ------------------------------------------------------------------------------------------ 9. learning sigma
def test_learn_likelihood_learns_sigma_and_leaves_tau(A, ctx):
    """Data drawn at sigma = 0.7, tau = 0.8, started at sigma = 2: every outer step is the Adam step lr in the direction of the
    reference's gradient at the marginals it was taken at, the bound rises from step to step, and tau stays what it was."""
    tau, lr = 0.8, 0.05
    rng = np.random.default_rng(9)
    M = 24
    Phi = (rng.normal(size=(N, M)) / math.sqrt(M)).astype(np.float32)
    kd = rng.uniform(0.05, 0.3, size=N).astype(np.float32)
    y = R.inverse_cdf(0.7, tau, Phi.astype(np.float64) @ rng.normal(size=M), rng.uniform(size=N)).astype(np.float32)
    cavi = A.SparseCAVI(A.AsymmetricLaplaceLikelihood(tau, 2.0), dev(Phi), dev(kd), dev(y), ctx=ctx)
    bounds, sig = [], [2.0]
    for step in range(6):
        tr = A.learn_likelihood(cavi, nouter=1, nsweeps=3, lr=lr)  # (one outer step a call: Adam's first step is lr sign(g))
        mu, var = (host(t)[0].astype(np.float64) for t in cavi.marginals())
        _, dref = R.expected_loglik(sig[-1], tau, y.astype(np.float64), mu, var)
        d = float(tr["lik"][1, 0] - tr["lik"][0, 0])
        assert np.sign(d) == np.sign(dref.sum()) and abs(abs(d) - lr) <= 1e-6 * lr
        assert tr["lik"].shape == (2, 1) and cavi.lik.tau == tau
        sig.append(cavi.lik.sigma)
        cavi.sweep()
        bounds.append(cavi.bound())
    print(f"ASYMLAPLACE learn_likelihood: sigma {sig}, bound {bounds}")
    assert sig[-1] < sig[0] and abs(math.log(sig[-1]) - math.log(0.7)) < abs(math.log(2.0) - math.log(0.7))
    assert all(b >= a for a, b in zip(bounds, bounds[1:])), bounds
