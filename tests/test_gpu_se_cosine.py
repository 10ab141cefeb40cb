"""The squared exponential x cosine kernel (include/agpl_kernels.h: AGPL_KERNEL_SE_COSINE, ``kernel=("se_cosine", p)``) on the device
against the float64 reference of tests/se_cosine_reference.py.  Every bar is the one tests/test_gpu_se_periodic.py uses for the same
quantity:

* features: err <= max(1e-5, 2 err_two), residual within 1e-5 s2; predict, predict_cov, predict_grad: 2e-5 of the max (of each
  row's max for the gradient); predict_chain and sample_paths: the element-wise bars of tests/chain_reference.py and
  tests/pathwise_reference.py with the plan's own features;
* hyper_grad / inducing_grad: |device - reference| / scale, scale the reference's sum of |terms|, within HYPER_BAR_FULL
  (tests/hyper_reference.py) and ZGRAD_BAR_FULL (tests/zgrad_reference.py);
* greedy selection: the reference's pivots, on inputs whose pivot margins tests/test_se_cosine_reference_cpu.py has shown to be
  clear.

k crosses zero, so every comparison here is of scale (against the max of the reference), as they already were for kind 8."""
import ctypes as C

import numpy as np
import pytest

import kernels_reference as K
import se_cosine_reference as SC

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

S2 = 1.0
GRID = [(D, M, r) for (D, M) in SC.CASES for r in SC.RATIOS]
IDS = [f"D{D}-M{M}-r{r}" for D, M, r in GRID]
FIT = SC.FIT
FIT_IDS = [f"D{D}-M{M}-r{r}" for D, M, r in FIT]
assert all(c in GRID for c in FIT)


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


def _check_features(A, ctx, x, z, ells, p, label, kernel=None, reference=None):
    N, M = len(x), len(z)
    plan = A.Plan.from_inputs(dev(x), dev(z), ells, variance=S2, jitter=SC.JITTER, ctx=ctx, kernel=kernel or ("se_cosine", p))
    F, d = host(plan.features()), host(plan.resid)
    # (K_XZ, Phi, residual, L^-1) of the reference the features are judged against
    Kxz, Phi, res, Linv = reference if reference is not None else (SC.kernel(x, z, ells, S2, p),) + SC.phi_f64(x, z, ells, S2, p)
    Mp = (M + 127) // 128 * 128
    K32 = np.zeros((N, Mp), np.float32)
    K32[:, :M] = Kxz
    two = host(A.whiten_features(torch.from_numpy(K32).cuda(), Linv, ctx=ctx))[:, :M]
    err_two, err = np.abs(two - Phi).max(), np.abs(F - Phi).max()
    print(f"FEATURES {label} N={N}: err {err:.3e} err_two {err_two:.3e} bar {max(1e-5, 2 * err_two):.3e} "
          f"residual err {np.abs(d - res).max():.3e}")
    assert F.shape == (N, M) and np.abs(Phi).max() > 1e-6
    assert err <= max(1e-5, 2 * err_two), (err, err_two)
    assert np.abs(d - res).max() <= 1e-5 * S2 and (d >= 0).all()
    return plan, F, max(1e-5, 2 * err_two)


@pytest.mark.parametrize("N", SC.NS)
@pytest.mark.parametrize("D,M,ratio", GRID, ids=IDS)
def test_plan_features_match_float64(A, ctx, D, M, ratio, N):
    """Fails without the feature: the kind is refused ("unknown kernel kind").  Both regimes of ell / p at every N; the features at
    the placed pairs (x[0] half a period from z[1], a quarter period from z[2]) carry the reference's sign."""
    x, z, ells, p = SC.workload(N, M, D, ratio)
    plan, F, bar = _check_features(A, ctx, x, z, ells, p, f"D={D} M={M} ell/p={ratio}")
    assert plan.kernel == "se_cosine" and plan.kernel_param == p
    Phi = SC.phi_f64(x, z, ells, S2, p)[0]
    print(f"PAIRS half a period: {F[0, 1]:+.6f} (reference {Phi[0, 1]:+.6f}); a quarter: {F[0, 2]:+.6f} (reference {Phi[0, 2]:+.6f})")
    for a in (1, 2):
        assert abs(Phi[0, a]) <= bar or np.sign(F[0, a]) == np.sign(Phi[0, a]), (a, F[0, a], Phi[0, a])
    assert (Phi < -bar).any() and (np.sign(F[np.abs(Phi) > bar]) == np.sign(Phi[np.abs(Phi) > bar])).all()


@pytest.mark.parametrize("D,M", [(1, 16), (3, 64)])
def test_a_very_long_period_is_the_squared_exponential(A, ctx, D, M):
    """p = 1e12: the factor is 1 to 1e-23 over these inputs, and the plan's features agree with an ``"se"`` plan's within the
    features' bar against the squared exponential reference."""
    x, z, ells, _ = SC.workload(777, M, D, 0.3)
    Kzz = K.kernel(K.SE, z, z, ells, S2) + SC.JITTER * np.eye(M)
    Linv = np.linalg.solve(np.linalg.cholesky(Kzz), np.eye(M))
    Phi = (Linv @ K.kernel(K.SE, z, x, ells, S2)).T
    ref = (K.kernel(K.SE, x, z, ells, S2), Phi, np.maximum(S2 - (Phi * Phi).sum(1), 0.0), Linv)
    _, F10, bar10 = _check_features(A, ctx, x, z, ells, 1e12, f"D={D} kind 10 p=1e12", reference=ref)
    _, F0, bar0 = _check_features(A, ctx, x, z, ells, 1e12, f"D={D} kind 0", kernel="se", reference=ref)
    assert bar0 == bar10
    print(f"D={D}: kinds 0 and 10 (p = 1e12) bit-identical: {np.array_equal(F0, F10)}; max |diff| {np.abs(F0 - F10).max():.3e} bar {bar10:.3e}")
    assert np.abs(F0 - F10).max() <= bar10, (np.abs(F0 - F10).max(), bar10)


def _latent(x, p):
    f = np.cos(2 * np.pi * x[:, -1] / p)
    return f + (2.0 * x[:, 0] - 1.0 if x.shape[1] > 1 else 0.0)


def _fit(A, ctx, lik_name, D, M, ratio, **kw):
    N = 255 if lik_name == "poisson" else 777
    x, z, ells, p = SC.workload(N, M, D, ratio)
    rng = np.random.default_rng(31)
    f = _latent(x, p)
    if lik_name == "bernoulli":
        lik, y = A.BernoulliLikelihood(), dev((rng.uniform(size=N) < 1 / (1 + np.exp(-2 * f))).astype(np.uint8))
    else:
        lik, y = A.PoissonLikelihood(4.0), dev(rng.poisson(4.0 / (1 + np.exp(-f))).astype(np.int32))
    cavi = A.SparseCAVI.from_inputs(lik, dev(x), y, dev(z), ells, variance=S2, jitter=SC.JITTER, ctx=ctx, kernel=("se_cosine", p), **kw)
    cavi.run(10)
    cavi.check()
    U = np.tril(host(cavi.plan.U_colmajor)[0].T[:M, :M])
    v = host(cavi.plan.v)[0, :M]
    return cavi, z, ells, p, U, v


@pytest.mark.parametrize("lik_name", ["bernoulli", "poisson"])
@pytest.mark.parametrize("D,M,ratio", FIT, ids=FIT_IDS)
def test_predict_cov_and_grad_after_ten_sweeps(A, ctx, lik_name, D, M, ratio):
    cavi, z, ells, p, U, v = _fit(A, ctx, lik_name, D, M, ratio)
    xs = SC.predict_inputs(z, ells, p, ratio)  # (xs[0], xs[1]: half and a quarter period from z[1], the other differences 0)
    m = U.T @ v
    phis = SC.phi_f64(xs, z, ells, S2, p)[0].T  # [M, Ns]
    mu_ref = m @ phis
    T = U @ phis
    var_ref = S2 - (phis * phis).sum(0) + (T * T).sum(0)
    mu, var = cavi.predict(dev(xs))
    e_mu, e_var = np.abs(host(mu)[0] - mu_ref).max(), np.abs(host(var)[0] - var_ref).max()
    print(f"PREDICT {lik_name} D={D} M={M} ell/p={ratio}: mu {e_mu / (2e-5 * np.abs(mu_ref).max()):.3f} var "
          f"{e_var / (2e-5 * np.abs(var_ref).max()):.3f} of the bar; max var {var_ref.max():.3f}")
    # conditions on the inputs (tests/test_gpu_periodic.py: the float32 variance bar has no margin below max var = 0.025 s2);
    # tests/test_se_cosine_reference_cpu.py shows the second from the reference alone for every case
    assert np.abs(mu_ref).max() > 1e-2 and var_ref.max() >= 0.025 * S2, var_ref.max()
    assert e_mu <= 2e-5 * np.abs(mu_ref).max() and e_var <= 2e-5 * np.abs(var_ref).max()
    # the joint covariance: negative entries half a period apart; the symmetric form is its own transpose bit for bit
    cov = host(cavi.predict_cov(dev(xs)))[0]
    cov_ref = SC.kernel(xs, xs, ells, S2, p) + phis.T @ (U.T @ U - np.eye(M)) @ phis
    e_cov = np.abs(cov - cov_ref).max()
    print(f"COV {e_cov / (2e-5 * np.abs(cov_ref).max()):.3f} of the bar; min cov {cov_ref.min():.3f}")
    assert e_cov <= 2e-5 * np.abs(cov_ref).max() and cov_ref.min() < -1e-2
    assert np.array_equal(cov, cov.T)
    cross = host(cavi.predict_cov(dev(xs[:100]), dev(xs[100:])))[0]  # the general form, against the same reference
    assert np.abs(cross - cov_ref[:100, 100:]).max() <= 2e-5 * np.abs(cov_ref).max()
    # the gradient of f, every dimension: mean m' d phi / d x_d, variance -d^2 k / d tau_d^2 at 0 - |d phi|^2 + |U d phi|^2
    dphi = SC.dphi_dx(xs, z, ells, S2, p)  # [D, Ns, M]
    rmu = np.einsum("a,dna->dn", m, dphi)
    Td = np.einsum("ab,dnb->dna", U, dphi)
    rvar = SC.prior_grad_variance(ells, S2, p)[:, None] - (dphi * dphi).sum(-1) + (Td * Td).sum(-1)
    dmu, dvar = cavi.predict_grad(dev(xs))
    assert host(dmu)[0].shape == (D, 255)
    g_mu = np.abs(host(dmu)[0] - rmu).max(-1) / np.abs(rmu).max(-1)
    g_var = np.abs(host(dvar)[0] - rvar).max(-1) / np.abs(rvar).max(-1)
    print(f"GRAD mean {np.array2string(g_mu / 2e-5, precision=3)} var {np.array2string(g_var / 2e-5, precision=3)} of the bar, per dimension")
    assert (g_mu <= 2e-5).all() and (g_var <= 2e-5).all(), (g_mu, g_var)
    # far from every inducing input the variance of d f / d x_d is the prior's: s2 / ell_d^2, the last s2 (1 / ell_L^2 + (2 pi / p)^2)
    far = xs[:1].copy()
    far[0, -1] = z[:, -1].max() + 40.0 * ells[-1]
    _, dv = cavi.predict_grad(dev(far))
    prior = SC.prior_grad_variance(ells, S2, p)
    assert np.abs(host(dv)[0, :, 0] - prior).max() <= 2e-5 * prior.max()


@pytest.mark.parametrize("D,M,ratio", FIT, ids=FIT_IDS)
def test_hyper_and_inducing_gradients(A, ctx, D, M, ratio):
    """The whole gradient (points' part and K_ZZ part) for log ell, log variance and z against the reference's analytic ones.  The
    workload's placed pairs are in: an inducing input half a period and one a quarter period from the first point."""
    import hyper_reference as HR
    import zgrad_reference as ZR

    N = 777
    x, z, ells, p = SC.workload(N, M, D, ratio)
    rng = np.random.default_rng(41)
    y = dev((rng.uniform(size=N) < 1 / (1 + np.exp(-2 * _latent(x, p)))).astype(np.uint8))
    jitter = 1e-6  # (the gradient tests' jitter)
    cavi = A.SparseCAVI.from_inputs(A.BernoulliLikelihood(), dev(x), y, dev(z), ells, variance=S2, jitter=jitter, ctx=ctx,
                                    kernel=("se_cosine", p), keep_points=True, keep_inputs=True)
    cavi.run(3)
    cavi.accumulate()
    cavi.check()
    plan = cavi.plan
    theta, gz = plan.inducing_grad(cavi.x, cavi.beta, cavi.gamma, None, cavi.G, cavi.g, with_theta=True)
    th2 = plan.hyper_grad(cavi.x, cavi.beta, cavi.gamma, None, cavi.G, cavi.g)
    ref = SC.bound_gradients(x, z, ells, S2, p, jitter, host(cavi.m), host(cavi.S), host(cavi.beta).astype(np.float64),
                             host(cavi.gamma).astype(np.float64))
    e_th = np.abs(host(th2) - ref["theta"]) / ref["scale_theta"]
    e_z = np.abs(host(gz) - ref["z"]) / ref["scale_z"]
    print(f"HYPER D={D} M={M} ell/p={ratio}: theta {e_th.max() / HR.HYPER_BAR_FULL:.3f} z {e_z.max() / ZR.ZGRAD_BAR_FULL:.3f} of the bars; "
          f"grad {np.array2string(ref['theta'], precision=3)} max |dz| {np.abs(ref['z']).max():.3e}")
    assert torch.equal(theta, th2)
    assert np.abs(ref["theta"]).max() > 1e-3 * ref["scale_theta"].max() and np.abs(ref["z"]).max() > 0
    assert e_th.max() <= HR.HYPER_BAR_FULL, e_th
    assert e_z.max() <= ZR.ZGRAD_BAR_FULL, e_z.max()


@pytest.mark.parametrize("learn_inducing", [False, True])
def test_learn_hyperparameters_runs(A, ctx, learn_inducing):
    D, M, ratio = GRID[4]
    x, z, ells, p = SC.workload(255, M, D, ratio)
    y = dev((np.cos(2 * np.pi * x[:, -1] / p) > 0).astype(np.uint8))
    out = A.learn_hyperparameters(A.BernoulliLikelihood(), dev(x), y, dev(z), ells, kernel=("se_cosine", p), nouter=2, nsweeps=2,
                                  ctx=ctx, learn_inducing=learn_inducing)
    cavi, trace = out
    assert cavi.plan.kernel == "se_cosine" and cavi.plan.kernel_param == p  # the period is not learned
    assert torch.isfinite(trace["log_lengthscale"]).all() and np.isfinite(trace["log_variance"]).all() and np.isfinite(trace["elbo"]).all()
    assert trace["log_lengthscale"].shape == (3, D) and (trace["log_lengthscale"][2] != trace["log_lengthscale"][0]).all()
    if learn_inducing:
        assert trace["z"].shape == (3, M, D) and torch.isfinite(trace["z"]).all() and (trace["z"][2] != trace["z"][0]).any()


def test_chain_prediction(A, ctx):
    """agpl_plan_predict_chain on a plan of Gibbs sweeps (no marginal image), as tests/test_gpu_se_periodic.py judges it: float64 with
    the plan's own features (test_plan_features_match_float64 judges those), element-wise bars."""
    import chain_reference as R
    from agpl_amd import _ffi

    D, M, ratio = GRID[5]
    N, T, L = 255, 3, 1
    x, z, ells, p = SC.workload(N, M, D, ratio)
    rng = np.random.default_rng(31)
    y = dev((rng.uniform(size=N) < 0.5).astype(np.uint8))
    gib = A.SparseGibbs.from_inputs(A.BernoulliLikelihood(), dev(x), y, dev(z), ells, variance=S2, jitter=SC.JITTER, ctx=ctx,
                                    kernel=("se_cosine", p))
    chain = gib.run(T)  # a short chain of this sampler: [T, L, M]
    pl = gib.plan
    assert pl.flags == A.Plan.NO_MARGINALS and pl.kernel == "se_cosine"
    Phi = host(pl.features()).astype(np.float64)
    assert np.abs(Phi - SC.phi_f64(x, z, ells, S2, p)[0]).max() <= 1e-5
    V = host(chain)
    assert V.shape == (T, L, M) and np.isfinite(V).all()
    mu0 = (0.5 * rng.standard_normal((L, N))).astype(np.float32)
    Vd, xd, m0d = chain.contiguous(), dev(x), dev(mu0)
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


@pytest.mark.parametrize("D,M,ratio", [GRID[3], GRID[4]], ids=[IDS[3], IDS[4]])
def test_sample_paths_against_the_reference(A, ctx, D, M, ratio):
    """agpl_plan_sample_paths with given (omega, phase) against tests/pathwise_reference.py's float64 formula and element-wise bars,
    with the plan's own features; the frequencies are spectral_frequencies' (the last column n +- 2 pi ell / p)."""
    import pathwise_reference as PR
    from test_gpu_pathwise import raw_paths

    N, T, L, Fn = 255, 3, 1, 64
    x, z, ells, p = SC.workload(N, M, D, ratio)
    plan = A.Plan.from_inputs(dev(x), dev(z), ells, variance=S2, jitter=SC.JITTER, L=L, ctx=ctx, kernel=("se_cosine", p))
    gen = torch.Generator(device="cuda").manual_seed(5)
    om, ph = A.spectral_frequencies(("se_cosine", p), Fn, D, generator=gen, lengthscale=ells)
    omega, phase = host(om), host(ph)
    shift = 2 * np.pi * ells[-1] / p
    assert omega.shape == (Fn, D) and abs(np.abs(omega[:, -1]).mean() - shift) < 0.2 * shift + 1.0
    rng = np.random.default_rng(9)
    V, W, Xi = rng.standard_normal((T, L, M)), rng.standard_normal((T, L, Fn)), rng.standard_normal((T, L, M))
    Phi = host(plan.features()).astype(np.float64)
    s = np.sqrt(S2) * np.sqrt(2.0 / Fn)
    Linv = SC.factor(z, ells, S2, p)[1]
    cc = PR.coefficients(V, W, Xi, PR.psi_f64(z, ells, omega, phase), Linv, s, SC.JITTER)
    Psi = PR.psi_f64(x, ells, omega, phase)
    ref = PR.reference(Phi, Psi, cc, W, s, None)
    mag = np.abs(phase).max() + (np.abs(x / ells) @ np.abs(omega).T).max()
    bars = PR.bars(Phi, Psi, cc, W, s, ref, plan.scale_exp, mag, D)
    F = raw_paths(plan, dev(V), om, ph, dev(W), dev(Xi), dev(x), None)
    ctx.synchronize()
    err = np.abs(host(F).astype(np.float64) - ref)
    print(f"PATHS D={D} M={M} ell/p={ratio}: max |F| {np.abs(ref).max():.3e} max err / bar {np.max(err / bars.F):.3f}")
    assert (err <= bars.F).all(), np.max(err / bars.F)
    # the Python surface draws its own frequencies for the kind (the plan passes its lengthscales on)
    paths = plan.sample_paths(2, nfeatures=32, generator=gen)
    assert host(paths.omega).shape == (32, D) and torch.isfinite(paths(dev(x))).all()


@pytest.mark.parametrize("D,ratio,periods", SC.GREEDY_CASES)
def test_greedy_selection_returns_the_reference_pivots(A, ctx, D, ratio, periods):
    x, ells, p = SC.greedy_inputs(D, ratio, periods)
    piv, margins = SC.greedy_pivots(x, SC.GREEDY_M, ells, S2, p)  # (margins: tests/test_se_cosine_reference_cpu.py)
    z, info = A.select_inducing_greedy(dev(x), SC.GREEDY_M, ells, variance=S2, kernel=("se_cosine", p), threshold=1e-12, ctx=ctx,
                                       return_info=True)
    got = np.asarray(info["indices"])
    print(f"GREEDY D={D} ell/p={ratio}: smallest margin {margins.min():.3e}")
    assert np.array_equal(got, piv), (got, piv)
    assert np.array_equal(host(z), x[piv])


def test_refusals(A, ctx):
    from agpl_amd import _ffi

    import test_gpu_kernels as TK

    x, z, ells, p = SC.workload(255, 16, 2, 0.3)
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(A.ArgumentError, match="period"):
            A.Plan.from_inputs(dev(x), dev(z), ells, ctx=ctx, kernel=("se_cosine", bad))
    for bad in (0.0, -2.0, float("nan"), float("inf")):  # the C entry point itself names p too
        rc, pl, msg = TK.raw_plan(A, ctx, "stationary", SC.KIND, bad, x, z, ells)
        assert rc == _ffi.ERR_INVALID_ARGUMENT and pl is None and "the period p of the squared exponential x cosine kernel" in msg, (bad, rc, msg)
    for kind in (5, 7, 9, 11, 12):  # no kinds
        rc, pl, msg = TK.raw_plan(A, ctx, "stationary", kind, 1.0, x, z, ells)
        assert rc == _ffi.ERR_INVALID_ARGUMENT and pl is None and "unknown kernel kind" in msg, (kind, rc, msg)
    with pytest.raises(A.AGPLError, match="select_inducing_greedy") as e:
        A.select_inducing(dev(x), 4, ells, ctx=ctx, kernel=("se_cosine", 1.0))
    assert e.value.code == _ffi.ERR_UNSUPPORTED
    with pytest.raises(A.ArgumentError, match="lengthscale"):
        A.spectral_frequencies(("se_cosine", 1.0), 16, 2)
