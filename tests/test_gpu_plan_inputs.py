"""GPU tests of plans built from raw squared-exponential inputs (include/agpl.h: agpl_plan_create_se, agpl_plan_predict,
agpl_plan_features; csrc/agpl_features.hip):

* the features a plan holds against float64 numpy (K, np.linalg.cholesky), with the two-step path's own error as the yardstick;
* ten CAVI sweeps from SparseCAVI.from_inputs against the float64 oracle fed the plan's own features, and against the two-step plan;
* prediction at new inputs against float64 numpy with the plan's own (U, v); predict(x_train) is marginals() bit for bit;
* per-point determinism (rebuilds, shards at offsets that are not multiples of 128);
* argument, domain and positive-definiteness errors, after which the context still works.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

SEED = 20240807
NAT_TOL = 1e-5


@pytest.fixture(scope="module")
def A():
    import agpl_amd

    return agpl_amd


@pytest.fixture(scope="module")
def oracle():
    from oracle import oracle as O

    return O


def host(t):
    return t.detach().cpu().numpy()


def relmax(a, b):
    return np.abs(np.asarray(a, np.float64) - b).max() / max(np.abs(b).max(), 1e-300)


def se_kernel(a, b, ell, s2):
    d = (a[:, None, :] - b[None, :, :]) / ell
    return s2 * np.exp(-0.5 * (d * d).sum(-1))


def phi_f64(x, z, ell, s2, jitter):
    """Phi [N, M] = (L^-1 K_ZX)' and the residual s2 - |phi|^2 in float64 (numpy), and L^-1."""
    Kzz = se_kernel(z, z, ell, s2) + jitter * np.eye(len(z))
    Lc = np.linalg.cholesky(Kzz)
    Linv = np.linalg.solve(Lc, np.eye(len(z)))
    Phi = (Linv @ se_kernel(z, x, ell, s2)).T
    return Phi, np.maximum(s2 - (Phi * Phi).sum(1), 0.0), Linv


def workload(N, M, D, seed=3):
    rng = np.random.default_rng(seed)
    x = rng.uniform(-10, 10, size=(N, D))
    if D == 1:
        z = np.linspace(-10, 10, M)[:, None]
        ell = np.array([1.5 * 20 / (M - 1)])
    else:
        z = rng.uniform(-10, 10, size=(M, D))
        ell = np.array([1.0, 1.4, 1.8][:D]) if D <= 3 else np.full(D, 12.0)
    return x, z, ell


@pytest.mark.parametrize("M,D,s2", [(37, 1, 1.0), (200, 3, 2.5), (256, 1, 2.5), (512, 3, 1.0), (1000, 1, 1.0), (1024, 3, 2.5),
                                      (64, 16, 1.0)])  # D = 16: the most the generator takes
def test_features_match_float64(A, M, D, s2):
    N, jitter = 5003, 1e-8
    x, z, ell = workload(N, M, D)
    ctx = A.Context(0, seed=1)
    plan = A.Plan.from_inputs(torch.from_numpy(x).cuda(), torch.from_numpy(z).cuda(), ell, variance=s2, jitter=jitter, ctx=ctx)
    F = host(plan.features())
    d = host(plan.resid)
    ctx.synchronize()
    Phi, res, Linv = phi_f64(x, z, ell, s2, jitter)
    assert len(ell) == D and np.abs(Phi).max() > 1e-6  # features of a size the bar below can judge
    # the two-step path's own error on the same points: float32 K_ZX, float32 L^-1 on the f32 MFMA (agpl_transform_features)
    Mp = (M + 127) // 128 * 128
    K32 = np.zeros((N, Mp), np.float32)
    K32[:, :M] = se_kernel(x, z, ell, s2)
    two = host(A.whiten_features(torch.from_numpy(K32).cuda(), Linv, ctx=ctx))[:, :M]
    err_two = np.abs(two - Phi).max()
    err = np.abs(F - Phi).max()
    assert F.shape == (N, M)
    assert err <= max(1e-5, 2 * err_two), (err, err_two)
    assert np.abs(d - res).max() <= 1e-5 * s2, np.abs(d - res).max()
    assert (d >= 0).all()


def _two_step(A, ctx, x, z, ell):
    """Phi and the residual of the existing four-step build (tests/test_gpu_plan.py::_svgp), D = 1, variance 1."""
    _, Linv = A.sparse.whitening_matrix(se_kernel(z[:, None], z[:, None], np.array([ell]), 1.0), 1e-8)
    Kzx = A.se_features(x, torch.from_numpy(z).cuda(), ell, ctx=ctx)
    Phi = A.whiten_features(Kzx, Linv, ctx=ctx)[:, : len(z)].contiguous()
    return Phi, A.sparse.nystrom_residual(Phi, torch.ones(len(x), device="cuda"), ctx=ctx)


def _liks(A, O):
    return {"bernoulli": (A.BernoulliLikelihood(), O.bernoulli()),
            "negbin": (A.NegativeBinomialLikelihood(15.0), O.negbinomial(15.0)),
            "categorical": (A.CategoricalLikelihood(np.array([0.1, -0.2, 0.3, 0.0])), O.categorical([0.1, -0.2, 0.3, 0.0])),
            "heterogauss": (A.HeteroscedasticGaussianLikelihood(2.0), O.heterogauss(2.0))}


@pytest.mark.parametrize("name,N,M", [("bernoulli", 10_000, 64), ("bernoulli", 6_000, 200), ("negbin", 6_000, 256),
                                      ("categorical", 4_000, 64), ("heterogauss", 4_000, 64)])
def test_ten_sweeps_from_inputs(A, oracle, name, N, M):
    O = oracle
    lik, olik = _liks(A, O)[name]
    L = olik.nlatent
    ctx = A.Context(0, seed=5)
    if name == "heterogauss":
        rng = np.random.default_rng(11)
        xh = rng.uniform(-10, 10, N)
        x = torch.from_numpy(xh).cuda()
        y = torch.from_numpy((np.sin(xh) + 0.3 * rng.standard_normal(N)).astype(np.float32)).cuda()
    else:
        x, y = A.synth_xy(lik, SEED, 0, N, ctx=ctx)
    z = np.linspace(-10, 10, M)
    ell = 1.5 * (z[1] - z[0])
    cavi = A.SparseCAVI.from_inputs(lik, x, y, torch.from_numpy(z).cuda(), ell, ctx=ctx)
    assert cavi.Phi is None
    F, kd = host(cavi.plan.features()), host(cavi.plan.resid).astype(np.float64)
    Phi2, kd2 = _two_step(A, ctx, x, z, ell)
    ref = A.SparseCAVI(lik, Phi2, kd2, y, ctx=ctx)
    y_h = host(y)
    S, m = np.tile(np.eye(M), (L, 1, 1)), np.zeros((L, M))
    for _ in range(10):
        cavi.sweep()
        ref.sweep()
        G, g = O.cavi_pass(olik, F, kd, y_h, -S, m)
        S, m = O.gaussian_update(G, g)
    cavi.check()
    ref.check()
    assert relmax(host(cavi.G), G) < NAT_TOL and relmax(host(cavi.g), g) < NAT_TOL, (relmax(host(cavi.G), G), relmax(host(cavi.g), g))
    # against the two-step plan: the features differ by the float32 round-off of either build; the M x M solve amplifies that by
    # cond(I + G) (the bar of test_gpu_plan.py::test_plan_path_at_any_feature_count_ten_sweeps)
    kappa = max(np.linalg.cond(np.eye(M) + G[l]) for l in range(L))
    assert relmax(host(cavi.m), host(ref.m)) < max(NAT_TOL, NAT_TOL * kappa)
    assert relmax(host(cavi.S), host(ref.S)) < max(NAT_TOL, NAT_TOL * kappa)


def test_predict(A, oracle):
    lik = A.BernoulliLikelihood()
    ctx = A.Context(0, seed=7)
    N, M = 10_000, 64
    x, y = A.synth_xy(lik, SEED, 0, N, ctx=ctx)
    z = np.linspace(-10, 10, M)
    ell = 1.5 * (z[1] - z[0])
    cavi = A.SparseCAVI.from_inputs(lik, x, y, torch.from_numpy(z).cuda(), ell, ctx=ctx)
    cavi.run(10)
    cavi.check()
    xs = np.linspace(-12, 12, 2001)
    mu, var = cavi.predict(torch.from_numpy(xs).cuda())
    U = host(cavi.plan.U_colmajor)[0].T[:M, :M]  # row-major view of the column-major lower triangle: U[a][b], b <= a
    U = np.tril(U)
    v = host(cavi.plan.v)[0, :M]
    _, _, Linv = phi_f64(xs[:, None], z[:, None], np.array([ell]), 1.0, 1e-8)
    phis = (Linv @ se_kernel(z[:, None], xs[:, None], np.array([ell]), 1.0))  # [M, Ns]
    mu_ref = (U.T @ v) @ phis
    T = U @ phis
    var_ref = 1.0 - (phis * phis).sum(0) + (T * T).sum(0)
    assert np.abs(host(mu)[0] - mu_ref).max() <= 2e-5 * np.abs(mu_ref).max()
    assert np.abs(host(var)[0] - var_ref).max() <= 2e-5 * np.abs(var_ref).max()
    # at the training inputs: the plan's own marginals, bit for bit
    mu_t, var_t = cavi.predict(x)
    mu_m, var_m = cavi.marginals()
    assert torch.equal(mu_t, mu_m) and torch.equal(var_t, var_m)


def test_per_point_determinism(A):
    lik = A.BernoulliLikelihood()
    ctx = A.Context(0, seed=9)
    N, M = 5003, 200
    x, y = A.synth_xy(lik, SEED, 0, N, ctx=ctx)
    zt = torch.from_numpy(np.linspace(-10, 10, M)).cuda()
    ell = 1.5 * 20 / (M - 1)
    a = A.SparseCAVI.from_inputs(lik, x, y, zt, ell, ctx=ctx)
    b = A.SparseCAVI.from_inputs(lik, x, y, zt, ell, ctx=ctx)
    assert torch.equal(a.plan.features(), b.plan.features()) and torch.equal(a.plan.resid, b.plan.resid)
    a.accumulate()
    b.accumulate()
    assert torch.equal(a.G, b.G) and torch.equal(a.g, b.g)
    full = a.plan.features()
    i0, i1 = 1237, 4001  # (not multiples of 128)
    part = A.Plan.from_inputs(x[i0:i1], zt, ell, ctx=ctx)
    assert torch.equal(part.features(), full[i0:i1])
    assert torch.equal(part.resid, a.plan.resid[i0:i1])
    assert torch.equal(part.features(100, 50), full[i0 + 100:i0 + 150])


def test_errors_leave_the_context_usable(A):
    ctx = A.Context(0, seed=3)
    N, M = 1000, 64
    x = torch.linspace(-10, 10, N, dtype=torch.float64, device="cuda")
    z = torch.linspace(-10, 10, M, dtype=torch.float64, device="cuda")
    ell = 0.5
    for kw in ({"lengthscale": 0.0}, {"lengthscale": -1.0}, {"variance": 0.0}, {"jitter": -1e-3}):
        args = {"lengthscale": ell, **kw}
        with pytest.raises(A.ArgumentError):
            A.Plan.from_inputs(x, z, ctx=ctx, **args)
    with pytest.raises(A.ArgumentError):
        A.Plan.from_inputs(torch.zeros((N, 17), dtype=torch.float64, device="cuda"),
                           torch.zeros((M, 17), dtype=torch.float64, device="cuda"), 1.0, ctx=ctx)
    xb = x.clone()
    xb[417] = float("nan")
    with pytest.raises(A.DomainError, match="417"):
        A.Plan.from_inputs(xb, z, ell, ctx=ctx)
    zb = z.clone()
    zb[33] = float("inf")
    with pytest.raises(A.DomainError, match="33"):
        A.Plan.from_inputs(x, zb, ell, ctx=ctx)
    zd = z.clone()
    zd[11] = zd[10]
    with pytest.raises(A.PosDefException):
        A.Plan.from_inputs(x, zd, ell, jitter=0.0, ctx=ctx)
    # predict on plans that cannot: one from agpl_plan_create, one without the marginal image
    lik = A.BernoulliLikelihood()
    xs, y = A.synth_xy(lik, SEED, 0, N, ctx=ctx)
    Phi, kd = _two_step(A, ctx, xs, host(z), 0.5)
    with pytest.raises(A.ArgumentError):
        A.SparseCAVI(lik, Phi, kd, y, ctx=ctx).predict(x)
    gib = A.SparseGibbs.from_inputs(lik, xs, y, z, 0.5, ctx=ctx)
    assert gib.Phi is None and gib.plan.flags == A.Plan.NO_MARGINALS
    gib.run(2)
    with pytest.raises(A.ArgumentError):
        gib.plan.predict(x)
    import ctypes as C

    from agpl_amd import _ffi
    for p in (A.Plan(Phi, kd, 1, ctx), gib.plan):  # the C entry point itself refuses too
        rc = _ffi.se_lib().agpl_plan_predict(p._h, C.c_int64(4), C.c_void_p(x.data_ptr()), None, C.c_void_p(Phi.data_ptr()),
                                          C.c_void_p(Phi.data_ptr()))
        assert rc == _ffi.ERR_INVALID_ARGUMENT
    # the context still runs a fresh build and sweep
    cavi = A.SparseCAVI.from_inputs(lik, xs, y, z, 0.5, ctx=ctx)
    cavi.run(2)
    cavi.check()
    assert torch.isfinite(cavi.G).all()
