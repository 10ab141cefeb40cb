"""The periodic kernel (include/agpl_kernels.h: AGPL_KERNEL_PERIODIC, ``kernel=("periodic", p)``) on the device against the float64
reference of tests/periodic_reference.py, every bar read from the existing test of the same entry point:

* features: err <= max(1e-5, 2 err_two), residual within 1e-5 s2 (tests/test_gpu_kernels.py::test_features_match_float64);
* predict: 2e-5 of the max (test_gpu_kernels.py::test_predict_at_new_inputs); predict_cov: 2e-5 of max |Cov| (the float64 tier of
  tests/test_gpu_predict_cov.py); predict_grad: 2e-5 of each row's max (tests/test_gpu_predict_grad.py);
* predict_chain: the element-wise bars of tests/chain_reference.py with the plan's own features (test_gpu_kernels.py's chain test);
* hyper_grad / inducing_grad: |device - reference| / scale, scale the reference's sum of |terms|, within HYPER_BAR_FULL
  (tests/hyper_reference.py) and ZGRAD_BAR_FULL (tests/zgrad_reference.py);
* sample_paths: the element-wise bars of tests/pathwise_reference.py with the plan's own features (tests/test_gpu_pathwise.py);
* greedy selection: the reference's pivots (tests/test_gpu_greedy.py), on inputs whose pivot margins
  tests/test_periodic_reference_cpu.py has shown to be clear."""
import ctypes as C

import numpy as np
import pytest

import periodic_reference as P

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

S2 = 1.0
GRID = [(D, M, ell, p) for (D, M, ell) in P.CASES for p in P.PERIODS]
IDS = [f"D{D}-M{M}-p{p}" for D, M, ell, p in GRID]


@pytest.fixture(scope="module")
def A():
    import agpl_amd

    return agpl_amd


def host(t):
    return t.detach().cpu().numpy()


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@pytest.fixture(scope="module")
def ctx(A):
    return A.Context(0, seed=17)


@pytest.mark.parametrize("N", P.NS)
@pytest.mark.parametrize("D,M,ell,p", GRID, ids=IDS)
def test_plan_features_match_float64(A, ctx, D, M, ell, p, N):
    """Fails without the feature: the kind is refused."""
    x, z, ells = P.workload(N, M, D, ell, p)
    plan = A.Plan.from_inputs(dev(x), dev(z), ells, variance=S2, jitter=P.JITTER, ctx=ctx, kernel=("periodic", p))
    assert plan.kernel == "periodic" and plan.kernel_param == p
    F, d = host(plan.features()), host(plan.resid)
    Phi, res, Linv = P.phi_f64(x, z, ells, S2, p)
    Mp = (M + 127) // 128 * 128
    K32 = np.zeros((N, Mp), np.float32)
    K32[:, :M] = P.kernel(x, z, ells, S2, p)
    two = host(A.whiten_features(torch.from_numpy(K32).cuda(), Linv, ctx=ctx))[:, :M]
    err_two, err = np.abs(two - Phi).max(), np.abs(F - Phi).max()
    print(f"FEATURES D={D} M={M} p={p} N={N}: err {err:.3e} err_two {err_two:.3e} bar {max(1e-5, 2 * err_two):.3e} "
          f"residual err {np.abs(d - res).max():.3e}")
    assert F.shape == (N, M) and np.abs(Phi).max() > 1e-6
    assert err <= max(1e-5, 2 * err_two), (err, err_two)
    assert np.abs(d - res).max() <= 1e-5 * S2 and (d >= 0).all()


def _fit(A, ctx, lik_name, D, M, ell, p, N=777, **kw):
    if lik_name == "poisson" and D == 1:
        N = 255  # (lambda = 4 and 777 points in D = 1, M = 16 leave max var = 0.019 s2: below the condition asserted in the test)
    x, z, ells = P.workload(N, M, D, ell, p)
    rng = np.random.default_rng(31)
    f = np.sin(2 * np.pi * x[:, 0] / p)
    if lik_name == "bernoulli":
        lik, y = A.BernoulliLikelihood(), dev((rng.uniform(size=N) < 1 / (1 + np.exp(-2 * f))).astype(np.uint8))
    else:
        lik, y = A.PoissonLikelihood(4.0), dev(rng.poisson(4.0 / (1 + np.exp(-f))).astype(np.int32))
    cavi = A.SparseCAVI.from_inputs(lik, dev(x), y, dev(z), ells, variance=S2, jitter=P.JITTER, ctx=ctx, kernel=("periodic", p), **kw)
    cavi.run(10)
    cavi.check()
    U = np.tril(host(cavi.plan.U_colmajor)[0].T[:M, :M])
    v = host(cavi.plan.v)[0, :M]
    return cavi, z, ells, U, v


@pytest.mark.parametrize("lik_name", ["bernoulli", "poisson"])
@pytest.mark.parametrize("D,M,ell,p", [GRID[1], GRID[2], GRID[5]], ids=[IDS[1], IDS[2], IDS[5]])
def test_predict_cov_and_grad_after_ten_sweeps(A, ctx, lik_name, D, M, ell, p):
    cavi, z, ells, U, v = _fit(A, ctx, lik_name, D, M, ell, p)
    xs = np.random.default_rng(23).uniform(-1.5 * p, 2.5 * p, size=(255, D))
    xs[0] = z[0] + p / 2  # delta = p / 2 exactly in every dimension against z[0]: u at its maximum, u' = 0
    m = U.T @ v
    phis = P.phi_f64(xs, z, ells, S2, p)[0].T  # [M, Ns]
    mu_ref = m @ phis
    T = U @ phis
    var_ref = S2 - (phis * phis).sum(0) + (T * T).sum(0)
    mu, var = cavi.predict(dev(xs))
    e_mu, e_var = np.abs(host(mu)[0] - mu_ref).max(), np.abs(host(var)[0] - var_ref).max()
    print(f"PREDICT {lik_name} D={D} M={M} p={p}: mu {e_mu / (2e-5 * np.abs(mu_ref).max()):.3f} var "
          f"{e_var / (2e-5 * np.abs(var_ref).max()):.3f} of the bar")
    # conditions on the inputs.  The variance is formed in float32 from s2: about 8 ulp of s2, 4.8e-7 s2, is its own round-off, and
    # the bar, relative to max var, is above that only where max var >= 0.024 s2 (lambda = 4 on 777 points in D = 1 gave 0.019 s2
    # and an error of 6.4e-7 s2: that case runs on 255 points)
    assert np.abs(mu_ref).max() > 1e-2 and var_ref.max() >= 0.025 * S2, var_ref.max()
    assert e_mu <= 2e-5 * np.abs(mu_ref).max() and e_var <= 2e-5 * np.abs(var_ref).max()
    # one period further: the same posterior within the same bar (not bit for bit: sinpi(t) and sinpi(t + 1) round differently)
    mu2, var2 = cavi.predict(dev(xs + p))
    assert np.abs(host(mu2)[0] - mu_ref).max() <= 2e-5 * np.abs(mu_ref).max()
    assert np.abs(host(var2)[0] - var_ref).max() <= 2e-5 * np.abs(var_ref).max()
    # the joint covariance
    cov = host(cavi.predict_cov(dev(xs)))[0]
    cov_ref = P.kernel(xs, xs, ells, S2, p) + phis.T @ (U.T @ U - np.eye(M)) @ phis
    e_cov = np.abs(cov - cov_ref).max()
    print(f"COV {e_cov / (2e-5 * np.abs(cov_ref).max()):.3f} of the bar")
    assert e_cov <= 2e-5 * np.abs(cov_ref).max()
    # the gradient of f: mean m' d phi / d x_d, variance d^2 k / dx dx' at 0 - |d phi|^2 + |U d phi|^2
    dphi = P.dphi_dx(xs, z, ells, S2, p)  # [D, Ns, M]
    rmu = np.einsum("a,dna->dn", m, dphi)
    Td = np.einsum("ab,dnb->dna", U, dphi)
    prior = S2 * (np.pi / (p * ells)) ** 2
    rvar = prior[:, None] - (dphi * dphi).sum(-1) + (Td * Td).sum(-1)
    dmu, dvar = cavi.predict_grad(dev(xs))
    g_mu = np.abs(host(dmu)[0] - rmu).max(-1) / np.abs(rmu).max(-1)
    g_var = np.abs(host(dvar)[0] - rvar).max(-1) / np.abs(rvar).max(-1)
    print(f"GRAD mean {g_mu.max() / 2e-5:.3f} var {g_var.max() / 2e-5:.3f} of the bar")
    assert (g_mu <= 2e-5).all() and (g_var <= 2e-5).all(), (g_mu, g_var)


@pytest.mark.parametrize("D,M,ell,p", [GRID[1], GRID[2], GRID[5]], ids=[IDS[1], IDS[2], IDS[5]])
def test_hyper_and_inducing_gradients(A, ctx, D, M, ell, p):
    """The whole gradient (points' part and K_ZZ part) for log ell, log variance and z against the reference's analytic ones.  One
    inducing input sits at delta = p / 2 exactly from the first point in every dimension (u' = 0, u at its maximum)."""
    import hyper_reference as HR
    import zgrad_reference as ZR

    N = 777
    x, z, ells = P.workload(N, M, D, ell, p)
    z = z.copy()
    z[1] = x[0] + p / 2
    rng = np.random.default_rng(41)
    y = dev((rng.uniform(size=N) < 1 / (1 + np.exp(-2 * np.sin(2 * np.pi * x[:, 0] / p)))).astype(np.uint8))
    jitter = 1e-6  # (the gradient tests' jitter)
    cavi = A.SparseCAVI.from_inputs(A.BernoulliLikelihood(), dev(x), y, dev(z), ells, variance=S2, jitter=jitter, ctx=ctx,
                                    kernel=("periodic", p), keep_points=True, keep_inputs=True)
    cavi.run(3)
    cavi.accumulate()
    cavi.check()
    plan = cavi.plan
    theta, gz = plan.inducing_grad(cavi.x, cavi.beta, cavi.gamma, None, cavi.G, cavi.g, with_theta=True)
    th2 = plan.hyper_grad(cavi.x, cavi.beta, cavi.gamma, None, cavi.G, cavi.g)
    ref = P.bound_gradients(x, z, ells, S2, p, jitter, host(cavi.m), host(cavi.S), host(cavi.beta).astype(np.float64),
                            host(cavi.gamma).astype(np.float64))
    e_th = np.abs(host(th2) - ref["theta"]) / ref["scale_theta"]
    e_z = np.abs(host(gz) - ref["z"]) / ref["scale_z"]
    print(f"HYPER D={D} M={M} p={p}: theta {e_th.max() / HR.HYPER_BAR_FULL:.3f} z {e_z.max() / ZR.ZGRAD_BAR_FULL:.3f} of the bars; "
          f"grad {np.array2string(ref['theta'], precision=3)} max |dz| {np.abs(ref['z']).max():.3e}")
    assert torch.equal(theta, th2)
    assert np.abs(ref["theta"]).max() > 1e-3 * ref["scale_theta"].max() and np.abs(ref["z"]).max() > 0
    assert e_th.max() <= HR.HYPER_BAR_FULL, e_th
    assert e_z.max() <= ZR.ZGRAD_BAR_FULL, e_z.max()


def test_learn_hyperparameters_runs(A, ctx):
    D, M, ell, p = GRID[1]
    x, z, ells = P.workload(255, M, D, ell, p)
    y = dev((x[:, 0] % p > p / 2).astype(np.uint8))
    out = A.learn_hyperparameters(A.BernoulliLikelihood(), dev(x), y, dev(z), ells, kernel=("periodic", p), nouter=2, nsweeps=2, ctx=ctx,
                                  learn_inducing=True)
    assert out is not None


def test_chain_prediction(A, ctx):
    """agpl_plan_predict_chain on a plan of Gibbs sweeps (no marginal image), judged as tests/test_gpu_kernels.py judges the
    Matern-5/2 plan: float64 with the plan's own features (test_plan_features_match_float64 judges those), element-wise bars."""
    import chain_reference as R
    from agpl_amd import _ffi

    D, M, ell, p = GRID[2]
    N, T, L = 255, 3, 1
    x, z, ells = P.workload(N, M, D, ell, p)
    rng = np.random.default_rng(31)
    y = dev((rng.uniform(size=N) < 0.5).astype(np.uint8))
    gib = A.SparseGibbs.from_inputs(A.BernoulliLikelihood(), dev(x), y, dev(z), ells, variance=S2, jitter=P.JITTER, ctx=ctx,
                                    kernel=("periodic", p))
    pl = gib.plan
    assert pl.flags == A.Plan.NO_MARGINALS and pl.kernel == "periodic"
    Phi = host(pl.features()).astype(np.float64)
    assert np.abs(Phi - P.phi_f64(x, z, ells, S2, p)[0]).max() <= 1e-5
    V = rng.standard_normal((T, L, M))
    mu0 = (0.5 * rng.standard_normal((L, N))).astype(np.float32)
    Vd, xd, m0d = dev(V), dev(x), dev(mu0)
    mean = torch.full((L, N), -7.0, dtype=torch.float32, device="cuda")
    spread, resid = torch.full_like(mean, -7.0), torch.full((N,), -7.0, dtype=torch.float32, device="cuda")
    F = torch.full((T, L, N), -7.0, dtype=torch.float32, device="cuda")
    ptr = lambda t: C.c_void_p(t.data_ptr())
    pl.call("agpl_plan_predict_chain", C.c_int32(T), ptr(Vd), C.c_int64(N), ptr(xd), ptr(m0d), ptr(mean), ptr(spread), ptr(resid), ptr(F),
            lib=_ffi.chain_lib())
    ctx.synchronize()
    r = R.reference(Phi, V, mu0.astype(np.float64))
    bars = R.bars(Phi, r, A.sparse.plan_padded(M), absolute=False)
    for name, got, want, bar in (("F", F, r.F, bars.F), ("mean", mean, r.mean, bars.mean), ("spread", spread, r.spread, bars.spread)):
        err = np.abs(host(got).astype(np.float64) - want)
        print(f"CHAIN {name}: max err / bar {np.max(err / bar):.3f}")
        assert (err <= bar).all(), (name, np.max(err / bar))
    assert torch.equal(resid, pl.resid)
    mean2, var2, resid2, F2 = gib.predict(xd, Vd, m0d, samples=True)
    assert torch.equal(mean2, mean) and torch.equal(F2, F) and torch.equal(var2, spread + resid)


@pytest.mark.parametrize("D,M,ell,p", [GRID[0], GRID[3]], ids=[IDS[0], IDS[3]])
def test_sample_paths_against_the_reference(A, ctx, D, M, ell, p):
    """agpl_plan_sample_paths with given (omega, phase) against tests/pathwise_reference.py's float64 formula and element-wise bars,
    with the plan's own features; the frequencies are spectral_frequencies' (integer multiples of 2 pi ell_d / p)."""
    import pathwise_reference as PR
    from test_gpu_pathwise import raw_paths

    N, T, L, Fn = 255, 3, 1, 64
    x, z, ells = P.workload(N, M, D, ell, p)
    plan = A.Plan.from_inputs(dev(x), dev(z), ells, variance=S2, jitter=P.JITTER, L=L, ctx=ctx, kernel=("periodic", p))
    gen = torch.Generator(device="cuda").manual_seed(5)
    om, ph = A.spectral_frequencies(("periodic", p), Fn, D, generator=gen, lengthscale=ells)
    omega, phase = host(om), host(ph)
    k = omega * p / (2 * np.pi * ells)
    assert np.abs(k - np.round(k)).max() < 1e-9 and np.abs(k).max() >= 1
    rng = np.random.default_rng(9)
    V, W, Xi = rng.standard_normal((T, L, M)), rng.standard_normal((T, L, Fn)), rng.standard_normal((T, L, M))
    Phi = host(plan.features()).astype(np.float64)
    s = np.sqrt(S2) * np.sqrt(2.0 / Fn)
    Linv = P.factor(z, ells, S2, p)[1]
    cc = PR.coefficients(V, W, Xi, PR.psi_f64(z, ells, omega, phase), Linv, s, P.JITTER)
    Psi = PR.psi_f64(x, ells, omega, phase)
    ref = PR.reference(Phi, Psi, cc, W, s, None)
    mag = np.abs(phase).max() + (np.abs(x / ells) @ np.abs(omega).T).max()
    bars = PR.bars(Phi, Psi, cc, W, s, ref, plan.scale_exp, mag, D)
    F = raw_paths(plan, dev(V), om, ph, dev(W), dev(Xi), dev(x), None)
    ctx.synchronize()
    err = np.abs(host(F).astype(np.float64) - ref)
    print(f"PATHS D={D} M={M} p={p}: max |F| {np.abs(ref).max():.3e} max err / bar {np.max(err / bars.F):.3f}")
    assert (err <= bars.F).all(), np.max(err / bars.F)
    # the Python surface draws its own frequencies for the kind
    paths = plan.sample_paths(2, nfeatures=32, generator=gen)
    kk = host(paths.omega) * p / (2 * np.pi * ells)
    assert np.abs(kk - np.round(kk)).max() < 1e-9 and torch.isfinite(paths(dev(x))).all()


@pytest.mark.parametrize("D,p", [(1, 1.0), (3, 2.5)])
def test_greedy_selection_returns_the_reference_pivots(A, ctx, D, p):
    x, ells = P.greedy_inputs(D, p)
    piv, margins = P.greedy_pivots(x, P.GREEDY_M, ells, S2, p)  # (margins: tests/test_periodic_reference_cpu.py)
    z, info = A.select_inducing_greedy(dev(x), P.GREEDY_M, ells, variance=S2, kernel=("periodic", p), threshold=1e-12, ctx=ctx,
                                       return_info=True)
    got = np.asarray(info["indices"])
    print(f"GREEDY D={D} p={p}: smallest margin {margins.min():.3e}")
    assert np.array_equal(got, piv), (got, piv)
    assert np.array_equal(host(z), x[piv])


def test_refusals(A, ctx):
    from agpl_amd import _ffi

    import test_gpu_kernels as TK

    x, z, ells = P.workload(255, 16, 1, 0.3, 1.0)
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(A.ArgumentError, match="period"):
            A.Plan.from_inputs(dev(x), dev(z), ells, ctx=ctx, kernel=("periodic", bad))
    for bad in (0.0, -2.0, float("nan"), float("inf")):  # the C entry point itself names p too
        rc, pl, msg = TK.raw_plan(A, ctx, "stationary", P.KIND, bad, x, z, ells)
        assert rc == _ffi.ERR_INVALID_ARGUMENT and pl is None and "period p" in msg, (bad, rc, msg)
    with pytest.raises(A.AGPLError, match="select_inducing_greedy") as e:
        A.select_inducing(dev(x), 4, ells, ctx=ctx, kernel=("periodic", 1.0))
    assert e.value.code == _ffi.ERR_UNSUPPORTED
    with pytest.raises(A.ArgumentError, match="lengthscale"):
        A.spectral_frequencies(("periodic", 1.0), 16, 1)
