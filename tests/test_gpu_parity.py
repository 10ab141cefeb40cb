"""GPU parity tests (run with -m gpu on an MI355X): every entry point of the C ABI is driven through the
Python host mirror and compared with the CPU oracle on the same seeded inputs.

Bars (BASELINE.json north_star): integer / index bookkeeping bit-exact (y copies, one-hot rows, Poisson and
negative-multinomial counts, uniforms consumed per draw, series index at acceptance); float64 operators
within 1e-12 relative (libm vs OCML last-ulp differences only); float32 operators within 2e-6; posterior
natural parameters (G, g, and Lambda_v = I + G) within 1e-5 relative to max|ref| after 10 sweeps.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

SEED = 20240807
NAT_TOL = 1e-5  # north_star: posterior natural parameters within 1e-5 relative


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


def lik_pairs(A, O):
    return {
        "bernoulli": (A.BernoulliLikelihood(), O.bernoulli()),
        "negbin": (A.NegativeBinomialLikelihood(15.0), O.negbinomial(15.0)),
        "negbin_real": (A.NegativeBinomialLikelihood(5.5), O.negbinomial(5.5)),
        "studentt": (A.StudentTLikelihood(3.5, 2.0), O.studentt(3.5, 2.0)),
        "poisson": (A.PoissonLikelihood(10.0), O.poisson(10.0)),
        "laplace": (A.LaplaceLikelihood(1.3), O.laplace(1.3)),
        "cat": (A.CategoricalLikelihood(np.array([0.1, -0.2, 0.3, 0.0])), O.categorical([0.1, -0.2, 0.3, 0.0])),
        "catbij": (A.CategoricalLikelihood(np.array([0.1, -0.2, 0.3, 0.0]), bijective=True),
                   O.categorical([0.1, -0.2, 0.3, 0.0], bijective=True)),
        "hetero": (A.HeteroscedasticGaussianLikelihood(5.0), O.heterogauss(5.0)),
    }


def gen_y(O, olik, n, rng):
    L = olik.nlatent
    if olik.kind == O.BERNOULLI:
        return (rng.uniform(size=n) < 0.5).astype(np.uint8)
    if olik.kind in (O.NEGBINOMIAL, O.POISSON):
        return rng.poisson(4.0, size=n).astype(np.int32)
    if olik.kind in (O.CATEGORICAL, O.CATEGORICAL_BIJ):
        K = L + (1 if olik.kind == O.CATEGORICAL_BIJ else 0)
        lab = rng.integers(0, K, size=n)
        return (lab[:, None] == np.arange(L)[None, :]).astype(np.uint8)
    return rng.normal(size=n)


ALL = ["bernoulli", "negbin", "negbin_real", "studentt", "poisson", "laplace", "cat", "catbij", "hetero"]


# ------------------------------------------------------------------------------------------ synthetic inputs
def test_synthetic_inputs_bit_exact(A, ctx, oracle):
    O = oracle
    for name in ("bernoulli", "negbin", "studentt", "cat", "catbij"):
        lik, olik = lik_pairs(A, O)[name]
        x, y = A.synth_xy(lik, SEED, 1000, 5000, ctx=ctx)
        assert np.array_equal(host(x), O.synth_x(SEED, 1000, 5000)) or relmax(host(x), O.synth_x(SEED, 1000, 5000)) < 1e-15
        yo = O.synth_y(olik, SEED, 1000, 5000)
        if name == "studentt":
            assert np.allclose(host(y), yo.astype(np.float32), rtol=1e-6)
        else:
            assert np.array_equal(host(y), yo), name  # integer outputs: bit-exact


# ------------------------------------------------------------------------------------------ PG sampler
@pytest.mark.parametrize("b,c", [(1, 0.0), (1, 2.0), (3, 0.0), (3, 2.5), (3, 3.2), (1.2, 3.2), (1, 9.0), (2, 60.0),
                                 (0, 1.0), (0.4, 0.7)])
def test_rand_polyagamma_matches_oracle_stream(A, ctx, oracle, b, c):
    n = 20000 if float(b).is_integer() else 2000
    out = torch.empty(n, dtype=torch.float64, device="cuda")
    _, nuni, nterms = A.rand_polyagamma(b, c, out, ctx=ctx, sweep=0, stats=True)
    ref, runi, rterms = oracle.rand_pg(b, c, n, seed=SEED, stats=True)
    # integer bookkeeping: uniforms consumed and summed series index, bit-exact
    assert np.array_equal(host(nuni).astype(np.uint32), runi)
    assert np.array_equal(host(nterms).astype(np.uint32), rterms)
    assert np.allclose(host(out), ref, rtol=1e-10, atol=0)
    if b > 0:
        # the reference's own sampler test (test/SpecialDistributions/polyagamma.jl:36) on the device draws
        assert abs(host(out)[:10000].mean() - oracle.pg_mean(b, c)) <= 1e-2 * max(1.0, b)


@pytest.mark.parametrize("name", ALL)
def test_aux_sample_matches_oracle(A, ctx, oracle, name):
    O = oracle
    lik, olik = lik_pairs(A, O)[name]
    rng = np.random.default_rng(5)
    n, L = 3000, olik.nlatent
    f = rng.normal(size=(n, L)) * 2.0
    if L == 1:
        f = f.ravel()
    y = gen_y(O, olik, n, rng)
    Om, nuni, nterms = A.aux_sample_(A.init_aux_variables(lik, n, ctx=ctx), lik, dev(y), dev(f), ctx=ctx, sweep=7,
                                     stats=True)
    ref = O.aux_sample(olik, y, f, seed=SEED, sweep=7, stats=True)
    assert np.array_equal(host(nuni).astype(np.uint32), ref["nuni"])
    assert np.array_equal(host(nterms).astype(np.uint32), ref["nterms"])
    if "n" in ref:
        assert np.array_equal(host(Om.n), ref["n"])  # Poisson / negative-multinomial counts: bit-exact
    assert np.allclose(host(Om.ω), ref["omega"], rtol=1e-10, atol=0)
    # sampled potentials / precisions (a10)
    fg = dev(f) if name == "hetero" else None
    beta, gamma = A.auglik_potential_and_precision(lik, Om, dev(y), fg, ctx=ctx)
    rb, rg = O.potential_precision(olik, y, ref["omega"], ref.get("n"), fg=f if name == "hetero" else None)
    assert len(beta) == len(gamma) == A.nlatent(lik)  # TestUtils.jl:83
    for k in range(L):
        assert np.allclose(host(beta[k]), rb[k], rtol=1e-10, atol=1e-300)
        assert np.allclose(host(gamma[k]), rg[k], rtol=1e-10, atol=1e-300)
        assert (host(gamma[k]) >= 0).all()  # TestUtils.jl:88
    if name not in ("hetero",):
        lt = A.logtilt(lik, Om, dev(y), dev(f), ctx=ctx)
        assert lt == pytest.approx(O.logtilt(olik, y, ref["omega"], f, ref.get("n")), rel=1e-11)
    if name in ("bernoulli", "negbin", "negbin_real", "studentt", "poisson", "laplace", "hetero"):
        # aug_loglik = logtilt + log-density of the aux prior at the draw (generic.jl:48-50; PG series polyagamma.jl:37-91;
        # priors poisson.jl:67-76 / polyagammapoisson.jl:29-33, laplace.jl:90-96); heteroscedasticgaussian.jl:106-128 its own
        fd, Omd, refd = f, Om, ref
        if name == "hetero":
            # The reference's 101-term series for logpdf(PG(b, 0), x) cancels catastrophically at large x (condition number 5e13 at
            # b = 106.5, x = 27 -- the draws (f - y)^2 ~ 50 above produce): there host and device libm differ in the third digit
            # and neither is right (docs/src/index.md:190-191 says to avoid it).  The density checks use residuals |f - y| ~ 0.8.
            fd = f.copy()
            fd[:, 0] = y + 0.8 * rng.normal(size=n)
            Omd = A.aux_sample_(A.init_aux_variables(lik, n, ctx=ctx), lik, dev(y), dev(fd), ctx=ctx, sweep=9)
            refd = O.aux_sample(olik, y, fd, seed=SEED, sweep=9)
            assert np.array_equal(host(Omd.n), refd["n"])
        al = A.aug_loglik(lik, Omd, dev(y), dev(fd), ctx=ctx)
        ral = O.aug_loglik(olik, y, refd["omega"], fd, refd.get("n"))
        assert np.isfinite(ral)
        assert al == pytest.approx(ral, rel=1e-9)  # (the 101-term PG density series through the device's libm)
        # the full-conditional-Omega identity of TestUtils.jl:107-116 with the DEVICE's aug_loglik on two of its own draws
        Om2 = A.aux_sample_(A.init_aux_variables(lik, n, ctx=ctx), lik, dev(y), dev(fd), ctx=ctx, sweep=8)
        hn = lambda o: host(o.n) if "n" in ref else None
        c1 = al - O.full_conditional_logpdf(olik, y, fd, host(Omd.ω), hn(Omd))
        c2 = A.aug_loglik(lik, Om2, dev(y), dev(fd), ctx=ctx) - O.full_conditional_logpdf(olik, y, fd, host(Om2.ω), hn(Om2))
        assert c1 == pytest.approx(c2, abs=1e-6)  # (1e-5 for n = 10 in the reference; measured ~1e-11 at n = 3000)
    if name in ("bernoulli", "negbin", "negbin_real", "studentt", "poisson", "laplace"):
        pl = A.aux_prior_logpdf(lik, Om, dev(y), ctx=ctx)
        assert pl == pytest.approx(O.aux_prior_logpdf(olik, y, ref["omega"], ref.get("n")), rel=1e-9)
    elif name == "hetero":
        with pytest.raises(A.AGPLError):  # no aux_prior for this likelihood in the reference
            A.aux_prior_logpdf(lik, Om, dev(y), ctx=ctx)
    else:
        with pytest.raises(A.AGPLError):  # categorical: the reference's logdensity_def is broken
            A.aug_loglik(lik, Om, dev(y), dev(f), ctx=ctx)


def test_sampler_is_reproducible_and_sweep_dependent(A, ctx):
    lik = A.BernoulliLikelihood()
    f = torch.linspace(-3, 3, 4096, dtype=torch.float64, device="cuda")
    a = A.aux_sample(lik, None, f, ctx=ctx, sweep=3).ω.clone()
    b = A.aux_sample(lik, None, f, ctx=ctx, sweep=3).ω
    c = A.aux_sample(lik, None, f, ctx=ctx, sweep=4).ω
    assert torch.equal(a, b)
    assert not torch.equal(a, c)


def test_aux_sample_edge_cases(A, ctx, oracle):
    lik = A.BernoulliLikelihood()
    # empty input
    e = A.aux_sample(lik, None, torch.empty(0, dtype=torch.float64, device="cuda"), ctx=ctx)
    assert e.ω.numel() == 0
    # f = 0 takes the hard-coded-r branch (polyagamma.jl:230-232); huge |f| takes the inverse-Gaussian branch
    f = np.array([0.0, -0.0, 1e-12, 40.0, -95.0, 200.0])
    got = A.aux_sample(lik, None, dev(f), ctx=ctx, sweep=1)
    ref = oracle.aux_sample(oracle.bernoulli(), np.zeros(6, np.uint8), f, seed=SEED, sweep=1)
    assert np.allclose(host(got.ω), ref["omega"], rtol=1e-10)
    assert (host(got.ω) > 0).all()
    # invalid negative-multinomial parameters raise ArgumentError (negativemultinomial.jl:17-22):
    # theta = (e^5, e^5, e^-30), f = 40 -> p_k = theta_k / sum(theta), sum p == 1.0 in float64
    cat = A.CategoricalLikelihood(np.array([5.0, 5.0, -30.0]), bijective=False)
    with pytest.raises(A.ArgumentError):
        A.aux_sample(cat, dev(np.zeros((4, 3), np.uint8)), dev(np.full((4, 3), 40.0)), ctx=ctx)
    # NaN / Inf latent values must not hang the accept loops: NaN in, NaN out
    fn = dev(np.array([np.nan, 1.0, np.inf, -np.inf]))
    got = host(A.aux_sample(lik, None, fn, ctx=ctx, sweep=2).ω)
    assert np.isnan(got[0]) and np.isfinite(got[1]) and np.isnan(got[2]) and np.isnan(got[3])
    with pytest.raises(ValueError):  # the oracle refuses the same input
        oracle.aux_sample(oracle.categorical([5.0, 5.0, -30.0]), np.zeros((4, 3), np.uint8), np.full((4, 3), 40.0), seed=1)
    # b = y + r >= 2^22 is outside the numbering of a point's draws (agpl_random.h kPgMaxB): reported (UNSUPPORTED), not a silent NaN
    nb = A.NegativeBinomialLikelihood(15.0)
    yb = dev(np.array([3, 65519, (1 << 22) - 15, 7], np.int32))  # b = 18, 65534, 2^22 (the first refused), 22
    fb = dev(np.array([0.3, 6.0, 6.0, -0.2]))
    ok = host(A.aux_sample(nb, yb[:2].contiguous(), fb[:2].contiguous(), ctx=ctx, sweep=3).ω)
    assert np.isfinite(ok).all() and ok[1] == pytest.approx(65534 / (2 * 6.0) * np.tanh(3.0), rel=0.05)
    with pytest.raises(A.AGPLError) as ei:
        A.aux_sample(nb, yb, fb, ctx=ctx, sweep=3)
    assert ei.value.code == -3 and "4194304" in str(ei.value)
    with pytest.raises(A.AGPLError):
        A.rand_polyagamma(4194304.0, 1.0, torch.empty(4, dtype=torch.float64, device="cuda"), ctx=ctx)


def test_polyagamma_beyond_the_sixteen_bit_draw_index(A, ctx, oracle):
    """polyagamma.jl:129-134 sums ANY integer b; rounds 2-5 stopped at b < 65535 (16 bits of the sub-stream id).  Round 6: draw
    j >= 65535 reuses id j mod 65535 and starts its block counter at (j div 65535) << 20 -- device and oracle agree on the stream
    (values, uniforms consumed, series indices), and the draws of b < 65535 are what they were (every golden fixture still passes).
    rand(PolyaGamma(200 000, c)), a negative-binomial and a Poisson point with y = 1e5 among ordinary ones."""
    O = oracle
    out = torch.empty(3, dtype=torch.float64, device="cuda")
    got, nuni, nterms = A.rand_polyagamma(200_000.0, 1.7, out, ctx=ctx, sweep=0, stats=True)
    ref, runi, rterms = O.rand_pg(200_000.0, 1.7, 3, seed=SEED, stats=True)
    assert np.array_equal(host(nuni).astype(np.uint32), runi) and np.array_equal(host(nterms).astype(np.uint32), rterms)
    assert np.allclose(host(got), ref, rtol=1e-10, atol=0)
    assert host(got)[0] == pytest.approx(200_000 / (2 * 1.7) * np.tanh(0.85), rel=5e-3)  # mean(PG(b, c)), polyagamma.jl:25-31
    # non-integer b: floor(b) draws + the residual series on its own id (0xFFFF is never a draw's id)
    got2 = A.rand_polyagamma(70_000.4, 0.9, torch.empty(2, dtype=torch.float64, device="cuda"), ctx=ctx, sweep=0)
    ref2 = O.rand_pg(70_000.4, 0.9, 2, seed=SEED)
    assert np.allclose(host(got2), ref2, rtol=1e-10, atol=0)
    # the vector entry point: the workgroup engine deals the 100 015 draws of one point across its wave
    nb, onb = A.NegativeBinomialLikelihood(15.0), O.negbinomial(15.0)
    y = np.array([3, 100_000, 0, 7, 65_520, 65_521, 11], np.int32)  # b = 18, 100015, 15, 22, 65535, 65536, 26
    f = np.array([0.3, 2.0, -1.0, -0.2, 0.7, -3.3, 0.0])
    Om, nu, nt = A.aux_sample_(A.init_aux_variables(nb, y.size, ctx=ctx), nb, dev(y), dev(f), ctx=ctx, sweep=5, stats=True)
    r = O.aux_sample(onb, y, f, seed=SEED, sweep=5, stats=True)
    assert np.array_equal(host(nu).astype(np.uint32), r["nuni"]) and np.array_equal(host(nt).astype(np.uint32), r["nterms"])
    assert np.allclose(host(Om.ω), r["omega"], rtol=1e-10, atol=0)
    po, opo = A.PoissonLikelihood(10.0), O.poisson(10.0)
    yp = np.array([4, 100_000, 9], np.int32)
    fp = np.array([0.2, 1.5, -0.4])
    Op = A.aux_sample(po, dev(yp), dev(fp), ctx=ctx, sweep=6)
    rp = O.aux_sample(opo, yp, fp, seed=SEED, sweep=6)
    assert np.array_equal(host(Op.n), rp["n"]) and np.allclose(host(Op.ω), rp["omega"], rtol=1e-10, atol=0)


@pytest.mark.parametrize("name", ["bernoulli", "negbin"])
def test_aux_sample_without_a_fitted_branch_mass(A, ctx, oracle, name):
    """|f| >= 16 (z >= 8) has no Chebyshev fit of the branch mass: every such draw is decided by the exact formula in the sequential
    sampler -- for Bernoulli on the retry list of the PG(1) kernel pair (here the list is FULL: every point is on it, at a ragged
    point count and with a second launch straight behind on the same list), for the one-latent engine in its phase C.  Values,
    uniforms consumed and series indices must be the oracle's (polyagamma.jl:223-257)."""
    O = oracle
    lik, olik = lik_pairs(A, O)[name]
    rng = np.random.default_rng(31)
    n = 5003
    f = rng.uniform(16.0, 30.0, size=n) * rng.choice([-1.0, 1.0], size=n)
    f[::7] = rng.normal(size=f[::7].shape)  # (and some ordinary points between them)
    y = gen_y(O, olik, n, rng)
    for sweep in (2, 3):
        Om, nuni, nterms = A.aux_sample_(A.init_aux_variables(lik, n, ctx=ctx), lik, dev(y), dev(f), ctx=ctx, sweep=sweep, stats=True)
        ref = O.aux_sample(olik, y, f, seed=SEED, sweep=sweep, stats=True)
        assert np.array_equal(host(nuni).astype(np.uint32), ref["nuni"])
        assert np.array_equal(host(nterms).astype(np.uint32), ref["nterms"])
        assert np.allclose(host(Om.ω), ref["omega"], rtol=1e-10, atol=0)


# ------------------------------------------------------------------------------------------ CAVI operators
@pytest.mark.parametrize("name", ALL)
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_aux_posterior_and_expectations(A, ctx, oracle, name, dtype):
    O = oracle
    lik, olik = lik_pairs(A, O)[name]
    rng = np.random.default_rng(6)
    n, L = 2500, olik.nlatent
    mu = rng.normal(size=(n, L)) * 1.5
    var = rng.uniform(0.05, 2.0, size=(n, L))
    if L == 1:
        mu, var = mu.ravel(), var.ravel()
    y = gen_y(O, olik, n, rng)
    tdt = torch.float64 if dtype == "f64" else torch.float32
    rtol = 1e-12 if dtype == "f64" else 3e-6
    yd = dev(y, tdt) if lik.ykind == "real" else dev(y)
    q = A.aux_posterior(lik, yd, (dev(mu, tdt), dev(var, tdt)), ctx=ctx)
    assert len(q) == n  # TestUtils.jl:155,160
    r1, r2, r3 = O.aux_posterior(olik, y, mu, var)
    phi = q.inds[0]
    names = [k for k in phi.keys() if k != "y"]
    for nm, ref in zip(names, (r1, r2, r3)):
        assert np.allclose(host(phi[nm]).astype(np.float64), ref, rtol=rtol, atol=1e-30), (name, nm)
    if "y" in phi.keys():
        assert np.array_equal(host(phi["y"]), y)  # integer copies: bit-exact
    beta, gamma = A.expected_auglik_potential_and_precision(lik, q, yd, (dev(mu, tdt), dev(var, tdt)), ctx=ctx)
    rb, rg = O.expected_potential_precision(olik, y, r1, r2, mu_g=mu[:, 1] if name == "hetero" else None)
    assert len(beta) == len(gamma) == A.nlatent(lik)
    for k in range(L):
        assert np.allclose(host(beta[k]).astype(np.float64), rb[k], rtol=10 * rtol, atol=1e-6 if dtype == "f32" else 1e-14)
        assert np.allclose(host(gamma[k]).astype(np.float64), rg[k], rtol=10 * rtol, atol=0)
        assert (host(gamma[k]) >= 0).all()  # TestUtils.jl:171
    b1 = A.expected_auglik_potential(lik, q, yd, (dev(mu, tdt), dev(var, tdt)), ctx=ctx)
    assert all(torch.equal(u, v) for u, v in zip(b1, beta))  # TestUtils.jl:168
    if dtype == "f64" and name != "hetero":
        el = A.expected_logtilt(lik, q, yd, (dev(mu), dev(var)), ctx=ctx)
        assert el == pytest.approx(O.expected_logtilt(olik, y, r1, r2, mu, var), rel=1e-11)
        if name == "cat":
            with pytest.raises(A.AGPLError):  # error() categorical.jl:165-170
                A.aux_kldivergence(lik, q, yd, ctx=ctx)
        else:
            kl = A.aux_kldivergence(lik, q, yd, ctx=ctx)
            assert kl == pytest.approx(O.aux_kl(olik, y, r1, r2), rel=1e-10)
            # expected_aug_loglik generic.jl:52-54 (the reference ADDS the KL)
            eal = A.expected_aug_loglik(lik, q, yd, (dev(mu), dev(var)), ctx=ctx)
            assert eal == pytest.approx(O.expected_aug_loglik(olik, y, r1, r2, mu, var), rel=1e-10)
            assert eal == pytest.approx(el + kl, rel=1e-12)
    if dtype == "f64" and name == "hetero":
        # the heteroscedastic likelihood defines expected_aug_loglik only (heteroscedasticgaussian.jl:130-145)
        eal = A.expected_aug_loglik(lik, q, yd, (dev(mu), dev(var)), ctx=ctx)
        assert eal == pytest.approx(O.expected_aug_loglik(olik, y, r1, r2, mu, var), rel=1e-10)
        with pytest.raises(A.AGPLError):
            A.expected_logtilt(lik, q, yd, (dev(mu), dev(var)), ctx=ctx)


def test_closed_form_means_on_device(A, ctx):
    # test/SpecialDistributions/polyagamma.jl:27-28 through expected_auglik_precision
    lik = A.BernoulliLikelihood()
    mu = torch.tensor([0.0, 2.0], dtype=torch.float64, device="cuda")
    q = A.aux_posterior(lik, torch.zeros(2, dtype=torch.uint8, device="cuda"), (mu, torch.zeros_like(mu)), ctx=ctx)
    g = host(A.expected_auglik_precision(lik, q, torch.zeros(2, dtype=torch.uint8, device="cuda"), ctx=ctx)[0])
    assert g[0] == 0.25
    assert g[1] == pytest.approx(np.tanh(1.0) / 4, rel=1e-15)


# ------------------------------------------------------------------------------------------ MFMA passes
def _features(rng, N, M, scale=0.3):
    return (rng.normal(size=(N, M)) * scale).astype(np.float32)


@pytest.mark.parametrize("N,M,L", [(1000, 128, 1), (4099, 256, 1), (257, 384, 2), (20000, 128, 3), (1, 128, 1),
                                   (127, 128, 1), (129, 256, 1)])
def test_marginals_against_float64(A, ctx, N, M, L):
    """agpl_marginals (float32-input MFMA) with the packed -S and alpha = m that agpl_gaussian_update writes, against float64."""
    import ctypes as C

    rng = np.random.default_rng(N + M)
    Phi = _features(rng, N, M)
    B = rng.normal(size=(L, M, 2 * M)) / np.sqrt(2 * M)
    G, g = np.einsum("lik,ljk->lij", B, B) * 3.0, rng.normal(size=(L, M))
    kd = rng.uniform(1, 2, size=N)
    mu0 = rng.normal(size=(L, N))
    S = torch.empty((L, M, M), dtype=torch.float64, device="cuda")
    m = torch.empty((L, M), dtype=torch.float64, device="cuda")
    Wp = torch.empty((L, M, M), dtype=torch.float32, device="cuda")
    dal = torch.empty((L, M), dtype=torch.float32, device="cuda")
    dG, dg = dev(G), dev(g)  # keep every device tensor referenced until the stream has consumed it
    pp = lambda t: C.c_void_p(t.data_ptr())
    ctx.call("agpl_gaussian_update", C.c_int32(M), C.c_int32(L), pp(dG), pp(dg), C.c_void_p(0), pp(S), pp(m), pp(Wp), pp(dal),
             C.c_void_p(0))
    W = -host(S)
    # packed layout: Wp[b][a] = 2 W[a][b] (b > a), W[a][a] (b == a), 0 (b < a)
    Wph = host(Wp)[0]
    assert np.allclose(np.tril(Wph, -1), 2 * np.tril(W[0], -1), rtol=1e-6, atol=1e-8)
    assert np.allclose(np.diag(Wph), np.diag(W[0]), rtol=1e-6) and np.all(np.triu(Wph, 1) == 0)
    mu = torch.empty((L, N), dtype=torch.float32, device="cuda")
    var = torch.empty_like(mu)
    dPhi, dkd, dmu0 = dev(Phi), dev(kd, torch.float32), dev(mu0, torch.float32)
    ctx.call("agpl_marginals", C.c_int64(N), C.c_int32(M), C.c_int32(L), pp(dPhi), pp(dkd), pp(dmu0), pp(Wp), pp(dal), pp(mu),
             pp(var))
    torch.cuda.synchronize()
    P = Phi.astype(np.float64)
    Wf = host(Wp).astype(np.float64)
    Wsym = np.stack([np.tril(w, -1) / 2 + np.tril(w, -1).T / 2 + np.diag(np.diag(w)) for w in Wf])
    af = host(dal).astype(np.float64)
    for l in range(L):
        ref_mu = mu0.astype(np.float32)[l] + P @ af[l]
        ref_var = kd.astype(np.float32) - np.einsum("ia,ab,ib->i", P, Wsym[l], P)
        assert np.abs(host(mu)[l] - ref_mu).max() < 2e-6 * np.abs(P).sum(1).max() * np.abs(af[l]).max() + 1e-6
        assert np.abs(host(var)[l] - ref_var).max() < 3e-6 * max(1.0, np.abs(ref_var).max())


@pytest.mark.parametrize("N,M,L", [(1000, 128, 1), (4099, 256, 1), (70001, 128, 2), (31, 128, 1), (5000, 384, 1),
                                   (300000, 128, 1)])
def test_accumulate_against_oracle(A, ctx, oracle, N, M, L):
    rng = np.random.default_rng(N + 3 * M)
    Phi = _features(rng, N, M)
    gamma = rng.uniform(0.0, 0.25, size=(L, N)).astype(np.float32)
    beta = rng.choice([-0.5, 0.5], size=(L, N)).astype(np.float32)
    G = torch.empty((L, M, M), dtype=torch.float64, device="cuda")
    g = torch.empty((L, M), dtype=torch.float64, device="cuda")
    import ctypes as C

    dPhi, dbeta, dgamma = dev(Phi), dev(beta), dev(gamma)
    args = (C.c_int64(N), C.c_int32(M), C.c_int32(L), C.c_void_p(dPhi.data_ptr()),
            C.c_void_p(dbeta.data_ptr()), C.c_void_p(dgamma.data_ptr()), C.c_void_p(G.data_ptr()),
            C.c_void_p(g.data_ptr()))
    ctx.call("agpl_accumulate", *args)
    G1 = host(G).copy()
    Gr, gr = oracle.accumulate(Phi, beta, gamma)
    # one f32 accumulation run covers <= 4096 points: eps * sqrt(4096) / 3 ~ 1.3e-6 relative per slab
    assert relmax(G1, Gr) < 5e-6
    assert relmax(host(g), gr) < 5e-6
    assert np.array_equal(G1, G1.transpose(0, 2, 1))  # exactly symmetric
    ctx.call("agpl_accumulate", *args)  # bitwise reproducible: fixed reduction order, no atomics
    assert np.array_equal(host(G), G1)


def test_accumulate_linearity_at_scale(A, ctx):
    """Size-independent property at a size the oracle cannot reach in seconds: G is linear in gamma."""
    N, M = 2_000_000, 256
    gen = torch.Generator(device="cuda").manual_seed(1)
    Phi = torch.randn((N, M), device="cuda", generator=gen) * 0.2
    g1 = torch.rand((1, N), device="cuda", generator=gen) * 0.25
    g2 = torch.rand((1, N), device="cuda", generator=gen) * 0.25
    b = torch.zeros((1, N), device="cuda")
    import ctypes as C

    def acc(gm):
        G = torch.empty((1, M, M), dtype=torch.float64, device="cuda")
        gg = torch.empty((1, M), dtype=torch.float64, device="cuda")
        ctx.call("agpl_accumulate", C.c_int64(N), C.c_int32(M), C.c_int32(1), C.c_void_p(Phi.data_ptr()),
                 C.c_void_p(b.data_ptr()), C.c_void_p(gm.data_ptr()), C.c_void_p(G.data_ptr()),
                 C.c_void_p(gg.data_ptr()))
        return G

    Ga, Gb, Gab = acc(g1), acc(g2), acc(g1 + g2)
    assert relmax(host(Ga + Gb), host(Gab)) < 1e-6
    # trace identity: tr G = sum_i gamma_i |phi_i|^2 (float64 torch reduction as the independent check)
    tr = (g1[0].double() * (Phi.double() ** 2).sum(1)).sum().item()
    assert host(torch.diagonal(Ga[0]).sum()) == pytest.approx(tr, rel=1e-6)


@pytest.mark.parametrize("L,M", [(2, 256), (1, 512), (2, 768), (1, 1024), (1, 1152), (2, 1536), (1, 2048), (1, 1100), (1, 2176)])
def test_gaussian_update_against_lapack(A, ctx, oracle, L, M):
    """S, m against LAPACK on every route: factor kernel (M <= 512), factor pipeline (M <= 1024, M % 128 == 0), two block rows of it
    (round 6: 1024 < M <= 2048, M % 128 == 0: 1152, 1536, 2048), rocSOLVER (1100: not a multiple of 128; 2176: beyond 2048)."""
    rng = np.random.default_rng(11 + M)
    B = rng.normal(size=(L, M, 3 * M)) / np.sqrt(M / 256.0)
    G = B @ B.transpose(0, 2, 1)
    g = rng.normal(size=(L, M))
    S = torch.empty((L, M, M), dtype=torch.float64, device="cuda")
    m = torch.empty((L, M), dtype=torch.float64, device="cuda")
    Wp = torch.empty((L, M, M), dtype=torch.float32, device="cuda")
    al = torch.empty((L, M), dtype=torch.float32, device="cuda")
    kl = torch.zeros(1, dtype=torch.float64, device="cuda")
    import ctypes as C

    dG, dg = dev(G), dev(g)
    ctx.call("agpl_gaussian_update", C.c_int32(M), C.c_int32(L), C.c_void_p(dG.data_ptr()),
             C.c_void_p(dg.data_ptr()), C.c_void_p(0), C.c_void_p(S.data_ptr()), C.c_void_p(m.data_ptr()),
             C.c_void_p(Wp.data_ptr()), C.c_void_p(al.data_ptr()), C.c_void_p(kl.data_ptr()))
    Sr, mr = oracle.gaussian_update(G, g)
    # kl_out: sum_l KL(N(m_l, S_l) || N(0, I)) = (tr S + m'm - M + logdet(I + G)) / 2  (aug_elbo's Gaussian term, script.jl:65-70)
    klr = sum(0.5 * (np.trace(Sr[l]) + mr[l] @ mr[l] - M + np.linalg.slogdet(np.eye(M) + G[l])[1]) for l in range(L))
    assert kl.item() == pytest.approx(klr, rel=1e-9)
    assert relmax(host(S), Sr) < 1e-9
    assert relmax(host(m), mr) < 1e-9
    assert np.array_equal(host(S), host(S).transpose(0, 2, 1))
    assert np.allclose(host(al), mr, rtol=1e-6, atol=1e-9)
    # not positive definite -> PosDefException analogue
    dbad, dg1 = dev(-2.0 * np.eye(M)[None]), dev(g[:1])
    with pytest.raises(A.PosDefException):
        ctx.call("agpl_gaussian_update", C.c_int32(M), C.c_int32(1), C.c_void_p(dbad.data_ptr()),
                 C.c_void_p(dg1.data_ptr()), C.c_void_p(0), C.c_void_p(S.data_ptr()),
                 C.c_void_p(m.data_ptr()), C.c_void_p(0), C.c_void_p(0), C.c_void_p(0))


def _setup_svgp(A, ctx, O, lik, olik, N, M, ell_factor=1.5, pad=128):
    x, y = A.synth_xy(lik, SEED, 0, N, ctx=ctx)
    z = np.linspace(-10, 10, M)
    ell = ell_factor * (z[1] - z[0])
    Kzz = np.exp(-0.5 * ((z[:, None] - z[None, :]) / ell) ** 2)
    _, Linv = A.sparse.whitening_matrix(Kzz, 1e-8)
    Kzx = A.se_features(x, dev(z), ell, ctx=ctx)
    # features against the oracle's float64 kernel rounded to float32
    ref_K = O.se_kernel_f32(host(x), z, ell)
    assert np.abs(host(Kzx)[:, :M] - ref_K).max() <= 1.2e-7
    assert (host(Kzx)[:, M:] == 0).all()
    Phi = A.whiten_features(Kzx, Linv, ctx=ctx)
    ref_Phi = ref_K.astype(np.float64) @ Linv.T
    assert np.abs(host(Phi)[:, :M] - ref_Phi).max() < 5e-5  # f32 GEMM with |L^-1| up to ~1e2
    kd = A.sparse.nystrom_residual(Phi, torch.ones(N, device="cuda"), ctx=ctx)
    if Phi.shape[1] % pad:  # zero feature columns change nothing (M is padded, never truncated)
        Phi = torch.nn.functional.pad(Phi, (0, pad - Phi.shape[1] % pad)).contiguous()
    return x, y, Phi, kd


@pytest.mark.parametrize("name,N,M", [("bernoulli", 10_000, 64), ("negbin", 6_000, 128), ("studentt", 5_000, 64),
                                      ("cat", 4_000, 64), ("catbij", 3_000, 64), ("poisson", 4_000, 64),
                                      ("laplace", 4_000, 64), ("hetero", 3_000, 64)])
def test_cavi_natural_parameters_match_oracle(A, ctx, oracle, name, N, M):
    """BASELINE config C1 (Bernoulli, N = 10 000, M = 64, 10 CAVI sweeps) and its siblings: after 10 sweeps the
    posterior natural parameters agree with the float64 oracle to 1e-5 (relative to max|ref| per array)."""
    O = oracle
    lik, olik = lik_pairs(A, O)[name]
    if name in ("poisson", "laplace", "hetero"):  # no synthetic generator for these: seeded numpy data
        _, _, Phi, kd = _setup_svgp(A, ctx, O, A.BernoulliLikelihood(), O.bernoulli(), N, M)
        rng = np.random.default_rng(41)
        xs = host(A.synth_xy(A.BernoulliLikelihood(), SEED, 0, N, ctx=ctx)[0])
        fs = 2 * np.sin(0.7 * xs) + np.cos(0.23 * xs)
        yh = rng.poisson(10.0 / (1 + np.exp(-fs))).astype(np.int32) if name == "poisson" else (
            fs + rng.laplace(scale=1.3, size=N) if name == "laplace" else fs + rng.normal(size=N) * 0.5)
        y = dev(yh) if name == "poisson" else dev(yh, torch.float32)
    else:
        x, y, Phi, kd = _setup_svgp(A, ctx, O, lik, olik, N, M)
    cavi = A.SparseCAVI(lik, Phi, kd, y, ctx=ctx, keep_points=True, marginal_precision="f32", accumulate_precision="f32")  # the float32-MFMA kernels
    Phi_h, kd_h, y_h = host(Phi), host(kd).astype(np.float64), host(y)
    Mp, L = Phi_h.shape[1], olik.nlatent
    S, m = np.tile(np.eye(Mp), (L, 1, 1)), np.zeros((L, Mp))
    for it in range(10):
        cavi.sweep()
        G, g, pts = O.cavi_pass(olik, Phi_h, kd_h, y_h.astype(np.float64) if lik.ykind == "real" else y_h, -S, m,
                                want_points=True)
        S, m = O.gaussian_update(G, g)
        if it in (0, 9):
            assert relmax(host(cavi.G), G) < NAT_TOL, (it, relmax(host(cavi.G), G))
            assert relmax(host(cavi.g), g) < NAT_TOL
            # per-point float32 expectations (not a natural parameter): looser, informational bound
            assert relmax(host(cavi.gamma), pts["gamma"]) < 1e-4
            assert relmax(host(cavi.beta), pts["beta"]) < 1e-4
    Lam, eta = cavi.natural_parameters()
    assert relmax(host(Lam), np.eye(Mp) + G) < NAT_TOL
    assert relmax(host(eta), g) < NAT_TOL
    # moments: the M x M solve amplifies the natural-parameter difference by cond(I + G) (why the bar is
    # stated on natural parameters); bound = bar x condition number
    kappa = max(np.linalg.cond(np.eye(Mp) + G[l]) for l in range(L))
    assert relmax(host(cavi.m), m) < max(1e-4, NAT_TOL * kappa)
    assert relmax(host(cavi.S), S) < max(1e-4, NAT_TOL * kappa)
    mu, var = cavi.marginals()
    assert (host(var) > 0).all()


@pytest.mark.parametrize("name", ALL)
def test_cavi_pass_is_its_operators_chained(A, ctx, oracle, name):
    """The sweep's fused per-point step and the stand-alone float32 operators state aux_posterior! and the expected potential /
    precision through the same rules (agpl_lik_rules.h) and are compiled without contraction: on the same float32 marginals
    agpl_cavi_pass's c, gamma, beta equal agpl_aux_posterior -> agpl_expected_potential_precision bit for bit, for every
    likelihood.  N = 777: several workgroups and a ragged last one; mu spans a few units either side of 0, var ~ 0.05 .. 3."""
    import ctypes as C

    lik, olik = lik_pairs(A, oracle)[name]
    rng = np.random.default_rng(29)
    N, M = 777, 128
    L = olik.nlatent
    La = 1 if name == "hetero" else L
    B = rng.normal(size=(L, M, 2 * M)) * 0.3
    dG, dg = dev(B @ B.transpose(0, 2, 1)), dev(rng.normal(size=(L, M)))
    dPhi = dev(_features(rng, N, M, 0.15))
    dkd = dev(rng.uniform(0.05, 3.0, size=N).astype(np.float32))
    dmu0 = dev((rng.normal(size=(L, N)) * 1.5).astype(np.float32))
    yh = gen_y(oracle, olik, N, rng)
    dy = dev(yh, torch.float32) if lik.ykind == "real" else dev(yh)
    p = lambda t: C.c_void_p(t.data_ptr())
    f32 = lambda *shape: torch.empty(shape, dtype=torch.float32, device="cuda")
    Wp, al = f32(L, M, M), f32(L, M)
    ctx.call("agpl_gaussian_update", C.c_int32(M), C.c_int32(L), p(dG), p(dg), C.c_void_p(0), C.c_void_p(0), C.c_void_p(0),
             p(Wp), p(al), C.c_void_p(0))
    G = torch.empty((L, M, M), dtype=torch.float64, device="cuda")
    g = torch.empty((L, M), dtype=torch.float64, device="cuda")
    c, gamma, beta = f32(N, La), f32(L, N), f32(L, N)
    d = lik.desc()
    ctx.call("agpl_cavi_pass", C.byref(d), C.c_int64(N), C.c_int32(M), p(dPhi), p(dkd), p(dmu0), p(dy), p(Wp), p(al), p(G), p(g),
             p(c), p(gamma), p(beta))
    mu, var = f32(L, N), f32(L, N)
    ctx.call("agpl_marginals", C.c_int64(N), C.c_int32(M), C.c_int32(L), p(dPhi), p(dkd), p(dmu0), p(Wp), p(al), p(mu), p(var))
    assert -2.0 > float(mu.min()) and float(mu.max()) > 2.0 and 0.05 <= float(var.min()) and float(var.max()) < 8.0
    mu_pm, var_pm = mu.t().contiguous(), var.t().contiguous()  # the operators take [N][L]
    q1, q2, q3 = f32(N, La), f32(N, La), f32(N)
    ctx.call("agpl_aux_posterior", C.byref(d), C.c_int32(A._ffi.F32), C.c_int64(N), p(dy), p(mu_pm), p(var_pm), p(q1), p(q2), p(q3))
    mu_g = mu[1].contiguous() if name == "hetero" else None
    beta2, gamma2 = f32(L, N), f32(L, N)
    ctx.call("agpl_expected_potential_precision", C.byref(d), C.c_int32(A._ffi.F32), C.c_int64(N), p(dy), p(q1), p(q2),
             p(mu_g) if mu_g is not None else C.c_void_p(0), p(beta2), p(gamma2))
    assert torch.equal(c, q1)
    assert torch.equal(gamma, gamma2)
    assert torch.equal(beta, beta2)


def test_cavi_reference_example_lengthscale_whitened(A, ctx, oracle):
    """The examples' own kernel (lengthscale 2.0, examples/bernoulli/script.jl:15) on the C1 grid is
    numerically singular: parity is asserted in the whitened parameterisation."""
    O = oracle
    lik, olik = A.BernoulliLikelihood(), O.bernoulli()
    N, M = 10_000, 64
    x, y = A.synth_xy(lik, SEED, 0, N, ctx=ctx)
    z = np.linspace(-10, 10, M)
    Kzz = np.exp(-0.5 * ((z[:, None] - z[None, :]) / 2.0) ** 2)
    _, Linv = A.sparse.whitening_matrix(Kzz, 1e-8)  # gp(x, 1e-8) script.jl:44
    # whitening in float64 on the host for this ill-conditioned case, then rounded to the device element type
    K64 = np.exp(-0.5 * ((host(x)[:, None] - z[None, :]) / 2.0) ** 2)
    Phi_h = np.zeros((N, 128), dtype=np.float32)
    Phi_h[:, :M] = K64 @ Linv.T
    kd_h = np.maximum(1.0 - (Phi_h.astype(np.float64) ** 2).sum(1), 0.0)
    cavi = A.SparseCAVI(lik, dev(Phi_h), dev(kd_h, torch.float32), y, ctx=ctx, marginal_precision="f32", accumulate_precision="f32")
    S, m = np.eye(128)[None], np.zeros((1, 128))
    for _ in range(10):
        cavi.sweep()
        G, g = O.cavi_pass(olik, Phi_h, kd_h.astype(np.float32).astype(np.float64), host(y), -S, m)
        S, m = O.gaussian_update(G, g)
    assert relmax(host(cavi.G), G) < NAT_TOL
    assert relmax(host(cavi.g), g) < NAT_TOL


def test_error_codes(A, ctx):
    import ctypes as C

    lik = A.BernoulliLikelihood()
    f = torch.zeros(8, dtype=torch.float64, device="cuda")
    with pytest.raises(A.ArgumentError):  # M not a multiple of 128
        ctx.call("agpl_accumulate", C.c_int64(8), C.c_int32(100), C.c_int32(1), C.c_void_p(f.data_ptr()),
                 C.c_void_p(f.data_ptr()), C.c_void_p(f.data_ptr()), C.c_void_p(f.data_ptr()), C.c_void_p(f.data_ptr()))
    with pytest.raises(TypeError):  # host tensors are rejected: no CPU fallback
        A.aux_sample(lik, None, torch.zeros(8, dtype=torch.float64), ctx=ctx)
    bad = A.NegativeBinomialLikelihood(-1.0)
    with pytest.raises(A.ArgumentError):
        A.aux_sample(bad, torch.zeros(8, dtype=torch.int32, device="cuda"), f, ctx=ctx)
    with pytest.raises(A.ArgumentError):  # Poisson needs n_out
        d = A.PoissonLikelihood(3.0).desc()
        ctx.call("agpl_aux_sample", C.byref(d), C.c_int64(8), C.c_void_p(f.data_ptr()), C.c_void_p(f.data_ptr()),
                 C.c_void_p(f.data_ptr()), C.c_void_p(0), C.c_uint32(0), C.c_void_p(0), C.c_void_p(0))


# ------------------------------------------------------------------------------------------ sparse Gibbs sweep
@pytest.mark.parametrize("name", ["bernoulli", "negbin", "studentt", "poisson", "cat", "hetero"])
def test_gibbs_pass_matches_oracle(A, ctx, oracle, name):
    """Per-point half of a Gibbs sweep: projection in the contractual float64 order, noise, aux_sample! on the
    same stream, sampled potentials, accumulation."""
    import ctypes as C

    O = oracle
    lik, olik = lik_pairs(A, O)[name]
    rng = np.random.default_rng(17)
    N, M = 3001, 256
    L = olik.nlatent
    Lo = 1 if name == "hetero" else L
    Phi = _features(rng, N, M, 0.15)
    kd = rng.uniform(0.0, 0.3, size=N).astype(np.float32)
    v = rng.normal(size=(L, M))
    y = gen_y(O, olik, N, rng)
    dPhi, dkd, dv = dev(Phi), dev(kd), dev(v)
    dy = dev(y)
    G = torch.empty((L, M, M), dtype=torch.float64, device="cuda")
    g = torch.empty((L, M), dtype=torch.float64, device="cuda")
    f = torch.empty((N, L), dtype=torch.float64, device="cuda")
    om = torch.empty((N, Lo), dtype=torch.float64, device="cuda")
    nn = torch.zeros((N, Lo), dtype=torch.int64, device="cuda")
    nuni = torch.zeros(N, dtype=torch.int32, device="cuda")
    d = lik.desc()
    ctx.call("agpl_gibbs_pass", C.byref(d), C.c_int64(N), C.c_int32(M), C.c_void_p(dPhi.data_ptr()),
             C.c_void_p(dkd.data_ptr()), C.c_void_p(0), C.c_void_p(dy.data_ptr()), C.c_void_p(dv.data_ptr()),
             C.c_uint32(9), C.c_void_p(G.data_ptr()), C.c_void_p(g.data_ptr()), C.c_void_p(f.data_ptr()),
             C.c_void_p(om.data_ptr()), C.c_void_p(nn.data_ptr()), C.c_void_p(nuni.data_ptr()))
    Gr, gr, pts = O.gibbs_pass(olik, Phi, kd.astype(np.float64), y, v, seed=SEED, sweep=9)
    assert np.array_equal(host(nuni).astype(np.uint32), pts["nuni"])  # uniforms consumed: bit-exact
    assert np.allclose(host(f), pts["f"], rtol=1e-13, atol=1e-15)  # same summation order; libm vs OCML in the noise
    assert np.allclose(host(om), pts["omega"], rtol=1e-9, atol=0)
    if name in ("poisson", "cat", "hetero"):
        assert np.array_equal(host(nn), pts["n"])  # counts: bit-exact
    assert relmax(host(G), Gr) < 5e-6
    assert relmax(host(g), gr) < 5e-6


@pytest.mark.parametrize("name", ALL)
def test_gibbs_pass_is_its_operators_chained(A, ctx, oracle, name):
    """The Gibbs point pass and the stand-alone operator state auglik_potential / auglik_precision through ONE rule
    (agpl_lik_rules.h), so agpl_potential_precision on the pass's own f, omega, n, narrowed to float32 and accumulated on the
    same features by the same float32-input kernel, gives the pass's G and g bit for bit -- for every likelihood."""
    import ctypes as C

    lik, olik = lik_pairs(A, oracle)[name]
    rng = np.random.default_rng(19)
    N, M = 3001, 256
    L = olik.nlatent
    Lo = 1 if name == "hetero" else L
    dPhi = dev(_features(rng, N, M, 0.15))
    dkd = dev(rng.uniform(0.0, 0.3, size=N).astype(np.float32))
    dv = dev(rng.normal(size=(L, M)))
    dy = dev(gen_y(oracle, olik, N, rng))
    p = lambda t: C.c_void_p(t.data_ptr())
    G, G2 = (torch.empty((L, M, M), dtype=torch.float64, device="cuda") for _ in range(2))
    g, g2 = (torch.empty((L, M), dtype=torch.float64, device="cuda") for _ in range(2))
    f = torch.empty((N, L), dtype=torch.float64, device="cuda")
    om = torch.empty((N, Lo), dtype=torch.float64, device="cuda")
    nn = torch.zeros((N, Lo), dtype=torch.int64, device="cuda")
    d = lik.desc()
    ctx.call("agpl_gibbs_pass", C.byref(d), C.c_int64(N), C.c_int32(M), p(dPhi), p(dkd), C.c_void_p(0), p(dy), p(dv),
             C.c_uint32(9), p(G), p(g), p(f), p(om), p(nn), C.c_void_p(0))
    beta, gamma = (torch.empty((L, N), dtype=torch.float64, device="cuda") for _ in range(2))
    ctx.call("agpl_potential_precision", C.byref(d), C.c_int64(N), p(dy), p(om), p(nn), p(f), p(beta), p(gamma))
    b32, g32 = beta.to(torch.float32), gamma.to(torch.float32)  # (round to nearest even, as the pass's own narrowing)
    ctx.call("agpl_accumulate", C.c_int64(N), C.c_int32(M), C.c_int32(L), p(dPhi), p(b32), p(g32), p(G2), p(g2))
    assert np.array_equal(host(G2), host(G))
    assert np.array_equal(host(g2), host(g))


@pytest.mark.parametrize("L,M", [(2, 256), (1, 512), (2, 640), (1, 1024), (1, 1280), (2, 200), (1, 37), (1, 600), (10, 1024), (1, 1300),
                                 (2, 2048), (1, 2100)])
def test_gibbs_draw_v_matches_oracle(A, ctx, oracle, L, M):
    """Every route of the conditional draw: the one-launch factor kernel (M <= 512), the factor pipeline (M <= 1024; ten latents in
    two launches), two block rows of it (1024 < M <= 2048: 1280, 2048, and 1300 padded to 1408), rocSOLVER (2100), and -- round 6 --
    feature counts the kernels do not take as they are (200, 37, 600, 1300), which agpl_gibbs_draw_v zero-pads to the next one they do;
    the draw z stays M-sized (the oracle's stream indices)."""
    import ctypes as C

    rng = np.random.default_rng(23 + M)
    B = rng.normal(size=(L, M, 2 * M)) * 0.3
    G = B @ B.transpose(0, 2, 1)
    g = rng.normal(size=(L, M))
    dG, dg = dev(G), dev(g)
    v = torch.empty((L, M), dtype=torch.float64, device="cuda")
    m = torch.empty((L, M), dtype=torch.float64, device="cuda")
    ctx.call("agpl_gibbs_draw_v", C.c_int32(M), C.c_int32(L), C.c_void_p(dG.data_ptr()), C.c_void_p(dg.data_ptr()),
             C.c_void_p(0), C.c_uint32(4), C.c_void_p(v.data_ptr()), C.c_void_p(m.data_ptr()))
    vr, mr = oracle.gibbs_draw_v(G, g, seed=SEED, sweep=4)
    assert relmax(host(m), mr) < 1e-9
    assert relmax(host(v), vr) < 1e-9


def test_sparse_gibbs_chain_matches_oracle_and_mixes(A, ctx, oracle):
    """Three full sweeps of the device chain against the oracle chain (same seeds), then a longer device-only run
    whose average of v must agree with the CAVI mean to Monte-Carlo accuracy (both target the same posterior
    region for a PG-augmented Bernoulli model)."""
    O = oracle
    lik, olik = A.BernoulliLikelihood(), O.bernoulli()
    N, M = 4000, 32
    x, y, Phi, kd = _setup_svgp(A, ctx, O, lik, olik, N, M)
    gctx = A.Context(0, seed=777)
    gib = A.SparseGibbs(lik, Phi, kd, y, ctx=gctx, keep_points=True)
    Phi_h, kd_h, y_h = host(Phi), host(kd).astype(np.float64), host(y)
    Mp = Phi_h.shape[1]
    v, _ = O.gibbs_draw_v(np.zeros((1, Mp, Mp)), np.zeros((1, Mp)), seed=777, sweep=0)
    assert np.allclose(host(gib.v), v, rtol=1e-12, atol=1e-14)
    sweep = 1
    for _ in range(3):
        gib.sweep()
        G, g, pts = O.gibbs_pass(olik, Phi_h, kd_h, y_h, v, seed=777, sweep=sweep)
        v, _ = O.gibbs_draw_v(G, g, seed=777, sweep=sweep)  # the draw uses stream (sweep | 2^31)
        sweep += 1
        assert relmax(host(gib.G), G) < 1e-5
        assert relmax(host(gib.v), v) < 1e-5 * np.linalg.cond(np.eye(Mp) + G[0])
    chain = host(gib.run(200))[40:, 0, :M]
    cavi = A.SparseCAVI(lik, Phi, kd, y, ctx=ctx)
    cavi.run(15)
    m = host(cavi.m)[0, :M]
    sd = chain.std(0) / np.sqrt(20)  # generous effective-sample-size allowance
    assert np.all(np.abs(chain.mean(0) - m) < 6 * sd + 0.05)


# ------------------------------------------------------------------------------------------ full-rank Gibbs (C5)
@pytest.mark.parametrize("name", ["studentt", "bernoulli", "negbin"])
def test_dense_gibbs_step_matches_oracle(A, ctx, oracle, name):
    """BASELINE config C5 at a size the oracle solves in seconds: StudentT (and the PG families) full-rank Gibbs,
    3 steps of the device chain against the numpy chain on the same Philox streams."""
    O = oracle
    lik, olik = lik_pairs(A, O)[name]
    N = 700
    rng = np.random.default_rng(31)
    x = np.sort(rng.uniform(-10, 10, size=N))
    K = np.exp(-0.5 * ((x[:, None] - x[None, :]) / 2.0) ** 2) + 1e-6 * np.eye(N)  # script.jl:15, lf 1e-6 :18
    y = gen_y(O, olik, N, rng)
    dctx = A.Context(0, seed=4242)
    dg = A.DenseGibbs(lik, dev(K), dev(y), ctx=dctx)
    Lk = np.linalg.cholesky(K)
    # the factor sits in the LAPACK-lower triangle of the column-major view = upper triangle of the torch tensor
    assert np.allclose(np.triu(host(dg.Lk)).T, Lk, rtol=1e-6, atol=1e-9)  # cond(K) ~ 1e6 with the 1e-6 jitter
    f = np.zeros(N)
    for sweep in range(3):
        dg.sweep()
        f, d = O.dense_gibbs_step(olik, K, Lk, y, f, seed=4242, sweep=sweep)
        assert np.allclose(host(dg.omega), d["omega"], rtol=1e-6)
        # f passes through a solve with cond(B) ~ 1e3..1e5
        assert np.abs(host(dg.f) - f).max() < 1e-6 * max(1.0, np.abs(f).max())


@pytest.mark.timeout(600)
def test_dense_gibbs_step_blocked_routes_match_oracle(A, ctx, oracle):
    """The same step above the blocking threshold (N >= 8192, not a multiple of the 2048 block): blocked Cholesky and
    blocked triangular solves on the device against the numpy chain."""
    O = oracle
    lik, olik = lik_pairs(A, O)["studentt"]
    N = 8192 + 300
    rng = np.random.default_rng(37)
    x = np.sort(rng.uniform(-400, 400, size=N))
    K = np.exp(-0.5 * ((x[:, None] - x[None, :]) / 2.0) ** 2) + 1e-3 * np.eye(N)
    y = gen_y(O, olik, N, rng)
    dctx = A.Context(0, seed=99)
    dg = A.DenseGibbs(lik, dev(K), dev(y), ctx=dctx)
    Lk = np.linalg.cholesky(K)
    f = np.zeros(N)
    for sweep in range(2):
        dg.sweep()
        f, d = O.dense_gibbs_step(olik, K, Lk, y, f, seed=99, sweep=sweep)
        assert np.allclose(host(dg.omega), d["omega"], rtol=1e-6)
        assert np.abs(host(dg.f) - f).max() < 1e-6 * max(1.0, np.abs(f).max())


@pytest.mark.timeout(900)
@pytest.mark.parametrize("N", [8192, 9216])
def test_dense_gibbs_step_inverse_block_route_matches_oracle(A, ctx, oracle, N):
    """Round 6: for N a multiple of 1024 (C5's 65 536) the step's solve runs block by block on the sparse sweep's one-launch
    factorisation -- U_k = chol(D_k)^-1, panel <- panel U_k' on the tile routine, trailing update, all in stream order; the
    triangular solves use the kept U_k.  Two sweeps against the numpy chain (np.linalg.cholesky of the same B), Student-t and --
    with gamma_i = 0 rows -- Poisson; a matrix that is not positive definite reports AGPL_ERR_NOT_POSDEF."""
    O = oracle
    rng = np.random.default_rng(41 + N)
    x = np.sort(rng.uniform(-400, 400, size=N))
    K = np.exp(-0.5 * ((x[:, None] - x[None, :]) / 2.0) ** 2) + 1e-3 * np.eye(N)
    Lk = np.linalg.cholesky(K)
    for name in ("studentt", "poisson") if N == 8192 else ("studentt",):
        lik, olik = lik_pairs(A, O)[name]
        y = gen_y(O, olik, N, rng)
        dctx = A.Context(0, seed=123)
        dg = A.DenseGibbs(lik, dev(K), dev(y), ctx=dctx)
        f = np.zeros(N)
        for sweep in range(2):
            dg.sweep()
            f, d = O.dense_gibbs_step(olik, K, Lk, y, f, seed=123, sweep=sweep)
            assert np.allclose(host(dg.omega), d["omega"], rtol=1e-6), name
            assert np.abs(host(dg.f) - f).max() < 1e-6 * max(1.0, np.abs(f).max()), name
        f1 = host(dg.f).copy()
        del dg
    # not positive definite: K with a negative eigenvalue and a large gamma (Student-t precision is positive)
    Kbad = K.copy()
    Kbad[N // 2, N // 2] = -50.0
    lik, olik = lik_pairs(A, O)["studentt"]
    y = gen_y(O, olik, N, rng)
    dctx = A.Context(0, seed=5)
    dg = A.DenseGibbs(lik, dev(K), dev(y), ctx=dctx)
    dg.K = dev(Kbad)
    with pytest.raises(Exception) as ei:
        dg.sweep()
    assert "positive definite" in str(ei.value)


def test_elbo_matches_oracle_and_increases(A, ctx, oracle):
    """aug_elbo (examples/bernoulli/script.jl:65-70) on the device against the float64 oracle evaluation, and the
    CAVI property the reference's commented-out test was after: the ELBO does not decrease across sweeps."""
    O = oracle
    lik, olik = A.BernoulliLikelihood(), O.bernoulli()
    N, M = 6000, 64
    x, y, Phi, kd = _setup_svgp(A, ctx, O, lik, olik, N, M)
    cavi = A.SparseCAVI(lik, Phi, kd, y, ctx=ctx, marginal_precision="f32", accumulate_precision="f32")
    Phi_h, kd_h, y_h = host(Phi), host(kd).astype(np.float64), host(y)
    Mp = Phi_h.shape[1]
    vals = []
    for it in range(6):
        cavi.sweep()
        vals.append(cavi.elbo())
    assert all(b >= a - 1e-6 * abs(a) for a, b in zip(vals, vals[1:])), vals
    # oracle ELBO for the device's current q(v)
    S, m, G = host(cavi.S), host(cavi.m), host(cavi.G)
    _, _, pts = O.cavi_pass(olik, Phi_h, kd_h, y_h, -S, m, want_points=True)
    mu, var = pts["mu"][:, 0], pts["var"][:, 0]
    c, _, _ = O.aux_posterior(olik, y_h, mu, var)
    kl_v = 0.5 * (np.trace(S[0]) + m[0] @ m[0] - Mp + np.linalg.slogdet(np.eye(Mp) + G[0])[1])
    ref = O.expected_logtilt(olik, y_h, c, None, mu, var) - O.aux_kl(olik, y_h, c) - kl_v
    assert vals[-1] == pytest.approx(ref, rel=2e-6)


# ------------------------------------------------------------------------------------------ the plan path (factor form)
def test_plan_path_takes_an_unpadded_feature_count(A, ctx):
    """Rounds 3-5 refused a feature count that is not a multiple of 256 on the plan path; round 6 pads inside the plan."""
    x = torch.zeros((64, 128), dtype=torch.float32, device="cuda")
    c = A.SparseCAVI(A.BernoulliLikelihood(), x, torch.ones(64, device="cuda"),
                     torch.zeros(64, dtype=torch.uint8, device="cuda"), ctx=ctx, marginal_precision="f16x2-factor")
    assert c.plan is not None and c.plan.Mp == 256 and tuple(c.G.shape) == (1, 128, 128)
    c.sweep()
    c.check()
    with pytest.raises(A.ArgumentError):  # the two arithmetics do not mix
        A.SparseCAVI(A.BernoulliLikelihood(), x, torch.ones(64, device="cuda"),
                     torch.zeros(64, dtype=torch.uint8, device="cuda"), ctx=ctx, marginal_precision="f16x2-factor",
                     accumulate_precision="f32")


@pytest.mark.parametrize("name,N,M", [("bernoulli", 10_000, 200), ("negbin", 6_000, 256), ("cat", 4_000, 250),
                                      ("studentt", 5_000, 256)])
def test_cavi_factor_form_matches_oracle(A, ctx, oracle, name, N, M):
    """10-sweep natural-parameter bar with the one-pass factor marginals and the split-float16 accumulation
    (bench.py's default path); S and m are materialised from (U, v) and compared too."""
    O = oracle
    lik, olik = lik_pairs(A, O)[name]
    x, y, Phi, kd = _setup_svgp(A, ctx, O, lik, olik, N, M, pad=256)
    cavi = A.SparseCAVI(lik, Phi, kd, y, ctx=ctx, marginal_precision="f16x2-factor", accumulate_precision="f16x2")
    Phi_h, kd_h, y_h = host(Phi), host(kd).astype(np.float64), host(y)
    Mp, L = Phi_h.shape[1], olik.nlatent
    S, m = np.tile(np.eye(Mp), (L, 1, 1)), np.zeros((L, Mp))
    try:
        for it in range(10):
            cavi.sweep()
            G, g = O.cavi_pass(olik, Phi_h, kd_h, y_h, -S, m)
            S, m = O.gaussian_update(G, g)
    finally:
        pass
    assert relmax(host(cavi.G), G) < NAT_TOL, relmax(host(cavi.G), G)
    assert relmax(host(cavi.g), g) < NAT_TOL
    # moments from (U, v): the M x M solve amplifies the natural-parameter difference by cond(I + G)
    kappa = max(np.linalg.cond(np.eye(Mp) + G[l]) for l in range(L))
    assert relmax(host(cavi.S), S) < max(1e-4, NAT_TOL * kappa)
    assert relmax(host(cavi.m), m) < max(1e-4, NAT_TOL * kappa)


@pytest.mark.parametrize("M,L", [(32, 1), (64, 2), (96, 1), (128, 1), (256, 1), (352, 1), (384, 3), (512, 2), (544, 1), (640, 3),
                                 (768, 1), (896, 2), (1024, 1), (1024, 2), (1024, 8), (1024, 9), (1536, 1), (256, 30), (512, 9), (256, 20), (512, 40),
                                 (1152, 1), (1280, 3), (1920, 1), (2048, 2), (2176, 1)])
def test_gaussian_factor_with_prior_term_and_all_routes(A, ctx, M, L):
    """agpl_gaussian_factor with eta0: v = U (g + eta0); the one-launch kernels (M <= 1024: every block count, both
    latent-per-XCD packings, nine latents at M = 1024 in two launches of the pipeline), two block rows of them (round 6: 1024 < M <=
    2048, M % 128 == 0 -- 1152, 1280 with three latents, 1536, 1920, 2048 with two) and the rocSOLVER route (M = 2176, and 544: not a
    multiple of 128 beyond 512) satisfy the same identities: U'U = (I+G)^-1,
    U'v = (I+G)^-1 (g + eta0), log det."""
    import ctypes as C

    rng = np.random.default_rng(M + L)
    B = rng.normal(size=(L, M, M + 7)) / np.sqrt(M)
    G = np.einsum("lik,ljk->lij", B, B) * 5.0
    g, eta0 = rng.normal(size=(L, M)), rng.normal(size=(L, M))
    dG, dg, de = dev(G), dev(g), dev(eta0)
    Aw = torch.empty((L, M, M), dtype=torch.float64, device="cuda")
    v = torch.empty((L, M), dtype=torch.float64, device="cuda")
    ld = torch.empty(L, dtype=torch.float64, device="cuda")
    ctx.call("agpl_gaussian_factor", C.c_int32(M), C.c_int32(L), C.c_void_p(dG.data_ptr()), C.c_void_p(dg.data_ptr()),
             C.c_void_p(de.data_ptr()), C.c_void_p(Aw.data_ptr()), C.c_void_p(v.data_ptr()), C.c_void_p(ld.data_ptr()))
    ctx.synchronize()  # (asynchronous: the outcome is reported here)
    for l in range(L):
        S = np.linalg.inv(np.eye(M) + G[l])
        Ut = np.triu(host(Aw)[l])
        assert relmax(Ut @ Ut.T, S) < 1e-10
        assert relmax(Ut @ host(v)[l], S @ (g[l] + eta0[l])) < 1e-10
        assert host(ld)[l] == pytest.approx(np.linalg.slogdet(np.eye(M) + G[l])[1], rel=1e-12)


@pytest.mark.parametrize("M,L", [(512, 1), (256, 3), (1024, 2)])
def test_gaussian_factor_rescue_launch_reproduces_the_cooperative_result(A, M, L):
    """The one-launch factorisation runs as cooperating workgroups that assume each other resident; when other work holds their
    CUs the launch reports info = -1 and a second launch queued behind it redoes the latent in one workgroup.  On an idle device
    that path never runs: agpl_debug_force_factor_rescue makes every cooperative launch take it.  U, v, log det and
    the float16 images of a plan's update must be the cooperative launch's -- bitwise: both run the same elimination order."""
    import ctypes as C

    rctx = A.Context(0, seed=3)
    rng = np.random.default_rng(M + L)
    B = rng.normal(size=(L, M, 2 * M)) / np.sqrt(2 * M)
    G, g = dev(np.einsum("lik,ljk->lij", B, B) * 2.0), dev(rng.normal(size=(L, M)))
    Phi = dev(_features(rng, 300, M))
    plan = A.sparse.Plan(Phi, torch.ones(300, device="cuda"), L, rctx)
    outs = []
    for force in (0, 1):
        rctx.call("agpl_debug_force_factor_rescue", C.c_int32(force))
        plan.U_colmajor.zero_()
        plan.call("agpl_plan_update", C.c_void_p(G.data_ptr()), C.c_void_p(g.data_ptr()), C.c_void_p(0), C.c_void_p(0))
        if force and M > 512:
            # beyond 512 rows one workgroup cannot hold a block column: a lost partner is REPORTED (the clean-up launch still
            # zeroes the hand-off flags, so the context stays usable)
            with pytest.raises(A.AGPLError, match="never arrived"):
                rctx.synchronize()
            rctx.call("agpl_debug_force_factor_rescue", C.c_int32(0))
            plan.call("agpl_plan_update", C.c_void_p(G.data_ptr()), C.c_void_p(g.data_ptr()), C.c_void_p(0), C.c_void_p(0))
            rctx.synchronize()
            assert torch.equal(torch.triu(plan.U_colmajor), outs[0][0]) and torch.equal(plan.v, outs[0][1])
            outs.append(outs[0])
            continue
        rctx.synchronize()
        outs.append((torch.triu(plan.U_colmajor).clone(), plan.v.clone(), plan.logdet.clone(), plan.U_hi.clone(),
                     plan.U_lo.clone(), plan.v32.clone()))
        # ... and the stand-alone entry point
        Aw = torch.zeros((L, M, M), dtype=torch.float64, device="cuda")
        v = torch.empty((L, M), dtype=torch.float64, device="cuda")
        ld = torch.empty(L, dtype=torch.float64, device="cuda")
        rctx.call("agpl_gaussian_factor", C.c_int32(M), C.c_int32(L), C.c_void_p(G.data_ptr()), C.c_void_p(g.data_ptr()),
                  C.c_void_p(0), C.c_void_p(Aw.data_ptr()), C.c_void_p(v.data_ptr()), C.c_void_p(ld.data_ptr()))
        rctx.synchronize()
        assert torch.equal(torch.triu(Aw), outs[-1][0]) and torch.equal(v, outs[-1][1]) and torch.equal(ld, outs[-1][2])
    rctx.call("agpl_debug_force_factor_rescue", C.c_int32(0))
    for a, b in zip(*outs):
        assert torch.equal(a, b)
    for l in range(L):  # and it is the factor: U'U = (I + G)^-1
        Ut = host(outs[1][0])[l]
        assert relmax(Ut @ Ut.T, np.linalg.inv(np.eye(M) + host(G)[l])) < 1e-10
    del plan


def test_small_workspace_regions_keep_apart_on_one_context(A):
    """Every user of the context's small workspace (csrc/agpl_ws2.h) on ONE context, interleaved: plan sweeps with update (item queues,
    bad-gamma word, hand-off flags, the factor tail), an ELBO reduction over 262 144 points (all 1016 partials, to the last byte
    below the queues), a second agpl_plan_create (range-check words, residual word), agpl_gaussian_update at M = 768, L = 2 (the
    workspace grows: the head moves), agpl_gibbs_draw_v at M = 37 (the padded tail), then two more sweeps.  G, g, U, v and log det
    must be bit for bit those of a fresh context that ran the four sweeps and nothing else, and the reduction's value that of a fresh
    context: a region that overlaps another, a zero-between-launches word left dirty or a head that does not travel with the
    reallocation changes one of them or fails the next sweep's outcome report."""
    import ctypes as C

    rng = np.random.default_rng(909)
    lik = A.BernoulliLikelihood()
    N, M = 2000, 256
    Phi, kd = dev(_features(rng, N, M)), torch.ones(N, device="cuda")
    y = dev((rng.uniform(size=N) < 0.5).astype(np.uint8))
    n = 262144
    mu, var = dev(rng.normal(size=n) * 1.5), dev(rng.uniform(0.05, 2.0, size=n))
    yn = dev((rng.uniform(size=n) < 0.5).astype(np.uint8))

    def logtilt(c):
        return A.expected_logtilt(lik, A.aux_posterior(lik, yn, (mu, var), ctx=c), yn, (mu, var), ctx=c)

    def sweeps(cavi, k):
        for _ in range(k):
            cavi.sweep()
            cavi.check()

    def state(cavi):
        return [t.clone() for t in (cavi.G, cavi.g, torch.triu(cavi.plan.U_colmajor), cavi.plan.v, cavi.plan.logdet)]

    one, ref = A.Context(0, seed=5), A.Context(0, seed=5)
    el_ref = logtilt(ref)  # (on the still fresh context)
    cavi_ref = A.SparseCAVI(lik, Phi, kd, y, ctx=ref, marginal_precision="f16x2-factor", accumulate_precision="f16x2")
    sweeps(cavi_ref, 4)
    want = state(cavi_ref)

    cavi = A.SparseCAVI(lik, Phi, kd, y, ctx=one, marginal_precision="f16x2-factor", accumulate_precision="f16x2")
    sweeps(cavi, 2)                                                       # 1
    el = logtilt(one)                                                     # 2
    other = A.sparse.Plan(Phi, kd, 1, one)                                # 3
    Mu, Lu = 768, 2                                                       # 4
    B = rng.normal(size=(Lu, Mu, 2 * Mu)) / np.sqrt(Mu)
    Gu, gu = B @ B.transpose(0, 2, 1), rng.normal(size=(Lu, Mu))
    S = torch.empty((Lu, Mu, Mu), dtype=torch.float64, device="cuda")
    m = torch.empty((Lu, Mu), dtype=torch.float64, device="cuda")
    dGu, dgu = dev(Gu), dev(gu)
    one.call("agpl_gaussian_update", C.c_int32(Mu), C.c_int32(Lu), C.c_void_p(dGu.data_ptr()), C.c_void_p(dgu.data_ptr()),
             C.c_void_p(0), C.c_void_p(S.data_ptr()), C.c_void_p(m.data_ptr()), C.c_void_p(0), C.c_void_p(0), C.c_void_p(0))
    assert relmax(host(S), np.linalg.inv(np.eye(Mu) + Gu)) < 1e-9
    Md = 37                                                               # 5
    Bd = rng.normal(size=(1, Md, 2 * Md)) * 0.3
    Gd, gd = dev(Bd @ Bd.transpose(0, 2, 1)), dev(rng.normal(size=(1, Md)))
    vd = torch.empty((1, Md), dtype=torch.float64, device="cuda")
    one.call("agpl_gibbs_draw_v", C.c_int32(Md), C.c_int32(1), C.c_void_p(Gd.data_ptr()), C.c_void_p(gd.data_ptr()), C.c_void_p(0),
             C.c_uint32(4), C.c_void_p(vd.data_ptr()), C.c_void_p(0))
    assert bool(torch.isfinite(vd).all())
    sweeps(cavi, 2)                                                       # 6
    assert el == el_ref
    for name, a, b in zip(("G", "g", "U", "v", "logdet"), state(cavi), want):
        assert torch.equal(a, b), name
    del other, cavi, cavi_ref


@pytest.mark.parametrize("M,first_bad", [(256, 0), (1024, 0), (1024, 700)])
def test_gaussian_factor_reports_indefinite_matrix(A, ctx, M, first_bad):
    import ctypes as C

    d = np.zeros(M)
    d[first_bad:] = -2.0  # I + G = diag(1, ..., 1, -1, ..., -1): whichever block step meets the first bad pivot must report it
    G = np.diag(d)[None]
    dG, dg = dev(G), dev(np.zeros((1, M)))
    Aw = torch.empty((1, M, M), dtype=torch.float64, device="cuda")
    with pytest.raises(A.PosDefException):
        ctx.call("agpl_gaussian_factor", C.c_int32(M), C.c_int32(1), C.c_void_p(dG.data_ptr()),
                 C.c_void_p(dg.data_ptr()), C.c_void_p(0), C.c_void_p(Aw.data_ptr()), C.c_void_p(0), C.c_void_p(0))
        ctx.synchronize()


def test_gaussian_factor_defers_the_report(A, ctx):
    """agpl_gaussian_factor returns before the outcome is known; a failed factorisation is reported by the next
    synchronisation point of the context (here agpl_ctx_synchronize), once, and the context is usable afterwards."""
    import ctypes as C

    M = 256
    d = np.zeros(M)
    d[100:] = -2.0
    dG, dg = dev(np.diag(d)[None]), dev(np.zeros((1, M)))
    Aw = torch.empty((1, M, M), dtype=torch.float64, device="cuda")
    args = (C.c_int32(M), C.c_int32(1), C.c_void_p(dG.data_ptr()), C.c_void_p(dg.data_ptr()), C.c_void_p(0),
            C.c_void_p(Aw.data_ptr()), C.c_void_p(0), C.c_void_p(0))
    ctx.call("agpl_gaussian_factor", *args)  # no exception yet
    with pytest.raises(A.PosDefException, match=r"row 100\)"):
        ctx.synchronize()
    ctx.synchronize()  # reported once
    good = dev(np.zeros((1, M, M)))
    gargs = (C.c_int32(M), C.c_int32(1), C.c_void_p(good.data_ptr()), C.c_void_p(dg.data_ptr()), C.c_void_p(0),
             C.c_void_p(Aw.data_ptr()), C.c_void_p(0), C.c_void_p(0))
    ctx.call("agpl_gaussian_factor", *gargs)
    ctx.synchronize()
    assert np.allclose(np.triu(host(Aw)[0]), np.eye(M))
    # a pending failure is also reported by the next factorisation on the context, before it starts
    ctx.call("agpl_gaussian_factor", *args)
    with pytest.raises(A.PosDefException):
        ctx.call("agpl_gaussian_factor", *gargs)
    ctx.synchronize()


def test_cavi_factor_form_reports_a_failed_update(A, ctx):
    """SparseCAVI in the factor form defers the outcome of its M x M update to the next pass: a state that makes
    I + G indefinite (planted directly in G) must still raise -- at the next sweep or at check()."""
    N, M = 2000, 256
    rng = np.random.default_rng(3)
    Phi = dev(_features(rng, N, M))
    kd = torch.ones(N, device="cuda")
    y = dev((rng.random(N) < 0.5).astype(np.uint8))
    cavi = A.SparseCAVI(A.BernoulliLikelihood(), Phi, kd, y, ctx=ctx, marginal_precision="f16x2-factor",
                        accumulate_precision="f16x2")
    cavi.sweep()
    cavi.check()
    cavi.G.copy_(-3.0 * torch.eye(M, dtype=torch.float64, device="cuda")[None])
    cavi.update()  # enqueued, not yet reported
    with pytest.raises(A.PosDefException):
        cavi.check()


def test_pg_logpdf_series_both_branches(A, ctx, oracle):
    """The aux-prior log-density at omega on both sides of the reference's x < 1e-2 switch to the log-domain series
    (polyagamma.jl:49-54), Bernoulli prior PG(1, 0), against the oracle's restatement point by point."""
    om = np.concatenate([10.0 ** np.linspace(-3.5, -2.001, 40), 10.0 ** np.linspace(-1.999, 0.7, 60)])
    lik = A.BernoulliLikelihood()
    y = np.zeros(om.size, dtype=np.uint8)
    for i in range(om.size):
        Om = A.TupleVector(ω=dev(om[i:i + 1]))
        got = A.aux_prior_logpdf(lik, Om, dev(y[i:i + 1]), ctx=ctx)
        ref = oracle.pg_logpdf(1.0, 0.0, om[i])
        # device libm vs glibc on arguments of magnitude 1e2..1e4 (R_n^2 / 8x): a few 1e-11 relative
        assert got == pytest.approx(ref, rel=5e-10, abs=1e-10), (om[i], got, ref)


def test_dense_cholesky_blocked_route(A, ctx):
    """agpl_dense_cholesky above its blocking threshold (N >= 8192; N not a multiple of the 2048 block) against
    torch.linalg.cholesky in float64, and the potrf-style failure report for an indefinite input."""
    import ctypes as C

    N = 8192 + 1000
    gen = torch.Generator(device="cuda").manual_seed(3)
    x = torch.sort(torch.rand(N, dtype=torch.float64, device="cuda", generator=gen) * 40 - 20).values
    K = torch.exp(-0.5 * ((x[:, None] - x[None, :]) / 0.05) ** 2)
    K.diagonal().add_(1e-3)
    Lk = torch.empty_like(K)
    ctx.call("agpl_dense_cholesky", C.c_int64(N), C.c_void_p(K.data_ptr()), C.c_void_p(Lk.data_ptr()))
    ref = torch.linalg.cholesky(K)
    got = torch.triu(Lk).T  # column-major lower triangle = row-major upper
    assert (got - ref).abs().max().item() < 1e-11
    Kbad = K.clone()
    Kbad[5000, 5000] = -1.0
    with pytest.raises(A.PosDefException):
        ctx.call("agpl_dense_cholesky", C.c_int64(N), C.c_void_p(Kbad.data_ptr()), C.c_void_p(Lk.data_ptr()))


@pytest.mark.timeout(600)
def test_c2_full_size_properties_of_the_shipped_path(A, ctx):
    """BASELINE config C2 at its full size (Bernoulli, N = 1e7, M = 512) on the path bench.py ships (split-float16
    contractions, factor-form marginals) -- sizes the oracle cannot reach, so size-independent properties:
      * G exactly symmetric, the sweep bitwise reproducible from the same state;
      * tr G = sum_n gamma_n |phi_n|^2, g = Phi beta and v'Gv = sum_n gamma_n (phi_n . v)^2 (4 random v: every tile of G enters)
        against float64 torch reductions over the same gamma, beta;
      * additivity over N: G(all) = G(first half) + G(second half) (the sharding identity of the multi-GPU sweep);
      * first-sweep marginals in closed form (S = I, m = 0: mu = 0, var = d + |phi|^2 = 1 for a unit-variance kernel);
      * gamma = tanh(c/2)/(2c) in (0, 1/4] and finite everywhere."""
    import ctypes as C

    N, M = 10_000_000, 512
    lik = A.BernoulliLikelihood()
    x, y = A.synth_xy(lik, SEED, 0, N, ctx=ctx)
    z = np.linspace(-10, 10, M)
    ell = 1.5 * (z[1] - z[0])
    Kzz = np.exp(-0.5 * ((z[:, None] - z[None, :]) / ell) ** 2)
    _, Linv = A.sparse.whitening_matrix(Kzz, 1e-8)
    Kzx = A.se_features(x, dev(z), ell, ctx=ctx)
    Phi = A.whiten_features(Kzx, Linv, ctx=ctx)
    del Kzx
    kd = A.sparse.nystrom_residual(Phi, torch.ones(N, device="cuda"), ctx=ctx)

    def make(sl=slice(None)):
        return A.SparseCAVI(lik, Phi[sl], kd[sl], y[sl], ctx=ctx, keep_points=True,
                            marginal_precision="f16x2-factor", accumulate_precision="f16x2")

    try:
        cavi = make()
        mu, var = cavi.marginals()  # S = I, m = 0
        assert mu.abs().max().item() == 0.0
        assert (var - 1.0).abs().max().item() < 2e-5  # k_nn = 1: d + |phi|^2 recombined in float32
        cavi.accumulate()
        G1, g1 = cavi.G.clone(), cavi.g.clone()
        assert torch.equal(G1, G1.transpose(1, 2))
        gam, bet = cavi.gamma[0], cavi.beta[0]
        assert torch.isfinite(gam).all() and (gam > 0).all() and (gam <= 0.25).all()
        # trace and g against float64 reductions, in chunks (no N x M float64 temporary)
        tr = 0.0
        gref = torch.zeros(M, dtype=torch.float64, device="cuda")
        for i0 in range(0, N, 1_000_000):
            P = Phi[i0:i0 + 1_000_000].double()
            tr += (gam[i0:i0 + 1_000_000].double() * (P * P).sum(1)).sum().item()
            gref += P.T @ bet[i0:i0 + 1_000_000].double()
        assert torch.diagonal(G1[0]).sum().item() == pytest.approx(tr, rel=2e-6)
        assert relmax(host(g1[0]), host(gref)) < 2e-6
        # quadratic forms v'Gv = sum_n gamma_n (phi_n . v)^2 for random v: unlike the trace they see every off-diagonal tile
        import bench

        chk = bench.full_size_quadratic_check(Phi, cavi.gamma, cavi.beta, G1, g1)
        assert chk["max_rel_d_vGv"] < 2e-6 and chk["rel_d_trace_G"] < 2e-6 and chk["max_rel_dg"] < 2e-6, chk
        cavi.accumulate()  # same state: bitwise identical
        assert torch.equal(cavi.G, G1) and torch.equal(cavi.g, g1)
        # the marginal kernel at this size with a REAL factor: two sweeps, then U, v from agpl_plan_state and
        # a sampled float64 evaluation over every per-XCD queue and the last tile; then gamma, beta from those marginals
        cavi.sweep()
        cavi.sweep()
        mchk = bench.full_size_marginal_check(cavi, Phi)
        assert mchk["sampled_points"] >= 10_000 and mchk["tile_residues_mod_8"] == list(range(8)), mchk
        assert mchk["max_abs_offdiag_U"] > 1e-3 and mchk["max_rel_d_mu"] < 2e-5 and mchk["max_rel_d_var"] < 2e-5, mchk
        idx, _ = bench.marginal_sample_indices(N)
        Ps = Phi[idx].double()
        T = Ps @ torch.triu(cavi.plan.U_colmajor[0])
        mu64 = T @ cavi.plan.v[0]
        c64 = torch.sqrt(mu64 * mu64 + kd[idx].double().clamp_min(0.0) + (T * T).sum(1))
        cavi.accumulate()
        gref = torch.tanh(c64 / 2) / (2 * c64)  # bernoulli.jl:41-45
        assert ((cavi.gamma[0][idx].double() - gref).abs().max() / gref.max()).item() < 2e-5
        assert torch.equal(cavi.beta[0][idx].double(), y[idx].double() - 0.5)
        del cavi, Ps, T
        h = N // 2
        parts = []
        for sl in (slice(0, h), slice(h, N)):
            c = make(sl)
            c.accumulate()
            parts.append((c.G.clone(), c.g.clone()))
            del c
        assert relmax(host(parts[0][0] + parts[1][0]), host(G1)) < 2e-6
        assert relmax(host(parts[0][1] + parts[1][1]), host(g1)) < 2e-6
    finally:
        pass


@pytest.mark.timeout(120)
def test_allreduce_nat_on_a_one_rank_rccl_communicator(A, ctx):
    """agpl_allreduce_nat with a communicator the caller owns (ncclCommInitRank through the process's librccl, one
    rank): the in-place float64 sum over one rank is the identity and the call returns AGPL_OK; a null communicator
    is an ArgumentError.  (The multi-rank sum is RCCL's; the two-rank sweep is covered through torch.distributed.)"""
    import ctypes as C

    try:
        rccl = C.CDLL("librccl.so.1")
    except OSError:
        pytest.skip("librccl not loadable in this process")

    class UniqueId(C.Structure):
        _fields_ = [("internal", C.c_char * 128)]

    uid = UniqueId()
    assert rccl.ncclGetUniqueId(C.byref(uid)) == 0
    comm = C.c_void_p()
    rccl.ncclCommInitRank.argtypes = [C.POINTER(C.c_void_p), C.c_int, UniqueId, C.c_int]
    assert rccl.ncclCommInitRank(C.byref(comm), 1, uid, 0) == 0
    try:
        M = 256
        flat, G, g = A.sparse.natural_parameter_buffers(1, M, "cuda")
        flat.copy_(torch.arange(flat.numel(), dtype=torch.float64, device="cuda") * 0.5 - 3.0)
        ref = flat.clone()
        ctx.call("agpl_allreduce_nat", comm, C.c_void_p(flat.data_ptr()), C.c_int64(flat.numel()))
        torch.cuda.synchronize()
        assert torch.equal(flat, ref)
        with pytest.raises(A.ArgumentError):
            ctx.call("agpl_allreduce_nat", C.c_void_p(0), C.c_void_p(flat.data_ptr()), C.c_int64(flat.numel()))
    finally:
        rccl.ncclCommDestroy.argtypes = [C.c_void_p]
        rccl.ncclCommDestroy(comm)


# ------------------------------------------------------------------------------------------ kernel variants (A/B forms)
