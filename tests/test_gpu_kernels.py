"""GPU tests of plans built from raw inputs for the stationary kernels of include/agpl_kernels.h (agpl_plan_create_stationary;
csrc/agpl_kernel_rules.h, agpl_se_build.h, agpl_se_create.h; ``kernel=`` of the ``from_inputs`` constructors):

* the features of every kind against float64 numpy, with the two-step path's own error as the yardstick;
* kind = squared exponential through the new entry point gives agpl_plan_create_se's plan bit for bit;
* the kinds' features differ (a dispatch that falls through to the squared exponential does not pass);
* prediction: predict(x_train) is marginals() bit for bit (L = 1 and 2), new inputs against float64 numpy with the plan's own (U, v);
* chain prediction of a Matern-5/2 plan against tests/chain_reference.py;
* per-point determinism (rebuilds, a shard that starts and ends inside a tile);
* ten CAVI sweeps against the float64 oracle fed the plan's own features;
* argument errors through the C entry point, after which the context still works.

Shapes (tests/kernels_reference.py): N = 300 (three 128-point tiles, the last holding 44 points), M = 37 (one k-slice short of a
multiple of 16, padded to 256) and M = 300 (padded to 512: four row blocks, the triangular skip crossing the 256 pad), D = 1 with z
on a grid and D = 3 with three lengthscales, variance 1 and 2.5; the rational quadratic at alpha = 2.
"""
import ctypes as C
import itertools

import numpy as np
import pytest

import chain_reference as R
import kernels_reference as K

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

N, JITTER = K.N, K.JITTER
NAT_TOL = 1e-5  # DESIGN 7 (tests/test_gpu_plan_inputs.py)
KIND_TOL = 1e-4  # "these are this kind's features": ten times below what separates two kinds (1e-3, test_kinds_differ)
KIND_IDS = [K.NAMES[k] for k in K.KINDS]


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


def dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    return t if dtype is None else t.to(dtype)


def relmax(a, b):
    return np.abs(np.asarray(a, np.float64) - b).max() / max(np.abs(b).max(), 1e-300)


@pytest.fixture(scope="module")
def world(A):
    """One context; the plans by (kind, M, D, s2, L, flags) and the float64 references by (kind, M, D, s2), each made once."""
    ctx = A.Context(0, seed=13)
    plans, refs = {}, {}

    def plan(kind, M, D, s2, L=1, flags=0):
        key = (kind, M, D, s2, L, flags)
        if key not in plans:
            x, z, ell = K.workload(N, M, D)
            plans[key] = A.Plan.from_inputs(dev(x), dev(z), ell, variance=s2, jitter=JITTER, L=L, ctx=ctx, flags=flags,
                                            kernel=K.python_kernel(kind))
        return plans[key]

    def ref(kind, M, D, s2):
        key = (kind, M, D, s2)
        if key not in refs:
            x, z, ell = K.workload(N, M, D)
            refs[key] = K.phi_f64(kind, x, z, ell, s2, JITTER, K.param_of(kind))
            for a in refs[key]:
                a.setflags(write=False)
        return refs[key]

    return ctx, plan, ref


def raw_plan(A, ctx, entry, kind, param, x, z, ell, s2=1.0, jitter=JITTER, L=1, flags=0):
    """A plan through the C entry point itself: ``entry`` = "stationary" (agpl_plan_create_stationary with kind, param) or "se"
    (agpl_plan_create_se).  Returns (status, plan or None, message)."""
    from agpl_amd import _ffi

    x, z, ell = dev(x), dev(z), dev(np.asarray(ell, np.float64))
    p = A.Plan.__new__(A.Plan)
    p.ctx = ctx
    p.N, p.M, p.L, p.D = int(x.shape[0]), int(z.shape[0]), L, int(x.shape[1])
    p.flags, p.Mp, p.se, p.variance = flags, A.sparse.plan_padded(int(z.shape[0])), True, float(s2)
    nbytes = _ffi.se_lib().agpl_plan_se_bytes(C.c_int64(p.N), C.c_int32(p.M), C.c_int32(L), C.c_int32(p.D), C.c_uint32(flags))
    assert nbytes > 0
    p.mem = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    p._h = C.c_void_p()
    ptr = lambda t: C.c_void_p(t.data_ptr())
    h = ctx.bind()
    head = (h, C.c_int64(p.N), C.c_int32(p.M), C.c_int32(L), C.c_int32(p.D))
    tail = (ptr(x), ptr(z), ptr(ell), C.c_double(s2), C.c_double(jitter), C.c_uint32(flags), ptr(p.mem), C.byref(p._h))
    if entry == "se":
        rc = _ffi.se_lib().agpl_plan_create_se(*head, *tail)
    else:
        rc = _ffi.kernels_lib().agpl_plan_create_stationary(*head, C.c_int32(kind), C.c_double(param), *tail)
    if rc != _ffi.AGPL_OK:
        assert not p._h.value  # nothing is handed out on an error
        return rc, None, (_ffi.lib().agpl_last_error(h) or b"").decode()
    p._bind(nbytes)
    return rc, p, ""


def test_workload_is_the_plan_input_tests_recipe():
    import test_gpu_plan_inputs as T

    for M, D, _ in K.SHAPES:
        for a, b in zip(K.workload(N, M, D), T.workload(N, M, D)):
            assert np.array_equal(a, b)


@pytest.mark.parametrize("M,D,s2", K.SHAPES)
@pytest.mark.parametrize("kind", K.KINDS, ids=KIND_IDS)
def test_features_match_float64(A, world, kind, M, D, s2):
    """err <= max(1e-5, 2 err_two), err_two the error of the two-step route (float32 K from numpy, float32 L^-1 on the f32 MFMA:
    A.whiten_features) on the same points; the residual within 1e-5 s2 of float64 and >= 0."""
    ctx, plan, ref = world
    p = plan(kind, M, D, s2)
    assert p.kernel == K.NAMES[kind] and p.kernel_param == K.param_of(kind)
    F, d = host(p.features()), host(p.resid)
    ctx.synchronize()
    Phi, res, Linv = ref(kind, M, D, s2)
    x, z, ell = K.workload(N, M, D)
    assert np.abs(Phi).max() > 1e-6
    Mp = (M + 127) // 128 * 128
    K32 = np.zeros((N, Mp), np.float32)
    K32[:, :M] = K.kernel(kind, x, z, ell, s2, K.param_of(kind))
    two = host(A.whiten_features(torch.from_numpy(K32).cuda(), Linv, ctx=ctx))[:, :M]
    err_two = np.abs(two - Phi).max()
    err = np.abs(F - Phi).max()
    print(f"{K.NAMES[kind]} M={M} D={D} s2={s2}: err {err:.3e}, err_two {err_two:.3e}, residual err {np.abs(d - res).max():.3e}")
    assert F.shape == (N, M)
    assert err <= max(1e-5, 2 * err_two), (err, err_two)
    assert np.abs(d - res).max() <= 1e-5 * s2, np.abs(d - res).max()
    assert (d >= 0).all()


def test_squared_exponential_through_the_new_entry_point_is_bit_for_bit(A, world):
    ctx, _, _ = world
    M, D, s2 = 300, 3, 2.5
    x, z, ell = K.workload(N, M, D)
    rc_a, a, msg_a = raw_plan(A, ctx, "stationary", K.SE, 0.0, x, z, ell, s2)
    rc_b, b, msg_b = raw_plan(A, ctx, "se", K.SE, 0.0, x, z, ell, s2)
    assert rc_a == 0 and rc_b == 0, (msg_a, msg_b)
    assert torch.equal(a.features(), b.features()) and torch.equal(a.resid, b.resid)
    assert a.scale_exp == b.scale_exp
    # param is ignored for every kind but the rational quadratic
    rc_c, c, msg_c = raw_plan(A, ctx, "stationary", K.SE, float("nan"), x, z, ell, s2)
    assert rc_c == 0, msg_c
    assert torch.equal(c.features(), b.features())


def test_kinds_differ(world):
    ctx, plan, _ = world
    F = {kind: host(plan(kind, 37, 1, 1.0).features()) for kind in K.KINDS}
    for a, b in itertools.combinations(K.KINDS, 2):
        diff = np.abs(F[a] - F[b]).max()
        print(K.NAMES[a], K.NAMES[b], f"{diff:.3e}")
        assert diff > 1e-3, (K.NAMES[a], K.NAMES[b], diff)


def _data(A, L, x, rng):
    f = np.sin(x[:, 0])
    if L == 1:
        return A.BernoulliLikelihood(), dev((rng.uniform(size=len(x)) < 1 / (1 + np.exp(-2 * f))).astype(np.uint8))
    return A.HeteroscedasticGaussianLikelihood(2.0), dev((f + 0.3 * rng.standard_normal(len(x))).astype(np.float32))


@pytest.mark.parametrize("M,D,s2,L", [(37, 1, 1.0, 1), (37, 1, 1.0, 2), (300, 3, 2.5, 2)])
@pytest.mark.parametrize("kind", [K.MATERN32, K.RQ], ids=["matern32", "rq"])
def test_predict_at_the_training_inputs_is_marginals(A, world, kind, M, D, s2, L):
    ctx, _, _ = world
    x, z, ell = K.workload(N, M, D)
    lik, y = _data(A, L, x, np.random.default_rng(21))
    cavi = A.SparseCAVI.from_inputs(lik, dev(x), y, dev(z), ell, variance=s2, jitter=JITTER, ctx=ctx, kernel=K.python_kernel(kind))
    assert cavi.plan.L == L
    cavi.run(3)
    cavi.check()
    mu_t, var_t = cavi.predict(dev(x))  # Ns = 300
    mu_m, var_m = cavi.marginals()
    assert mu_t.shape == (L, N) and torch.isfinite(mu_t).all() and torch.isfinite(var_t).all()
    assert torch.equal(mu_t, mu_m) and torch.equal(var_t, var_m)


@pytest.mark.parametrize("M,D,s2", [(37, 1, 1.0), (300, 3, 2.5)])
@pytest.mark.parametrize("kind", [K.MATERN32, K.RQ], ids=["matern32", "rq"])
def test_predict_at_new_inputs(A, world, kind, M, D, s2):
    """Within 2e-5 of the max (the bar of tests/test_gpu_plan_inputs.py::test_predict) of the float64 posterior from numpy features
    and the plan's own (U, v)."""
    ctx, _, _ = world
    x, z, ell = K.workload(N, M, D)
    lik, y = _data(A, 1, x, np.random.default_rng(22))
    cavi = A.SparseCAVI.from_inputs(lik, dev(x), y, dev(z), ell, variance=s2, jitter=JITTER, ctx=ctx, kernel=K.python_kernel(kind))
    cavi.run(5)
    cavi.check()
    xs = np.random.default_rng(23).uniform(-12, 12, size=(257, D))  # some outside the hull of z
    mu, var = cavi.predict(dev(xs))
    U = np.tril(host(cavi.plan.U_colmajor)[0].T[:M, :M])
    v = host(cavi.plan.v)[0, :M]
    phis = K.phi_f64(kind, xs, z, ell, s2, JITTER, K.param_of(kind))[0].T  # [M, Ns]
    mu_ref = (U.T @ v) @ phis
    T = U @ phis
    var_ref = s2 - (phis * phis).sum(0) + (T * T).sum(0)
    e_mu, e_var = np.abs(host(mu)[0] - mu_ref).max(), np.abs(host(var)[0] - var_ref).max()
    print(f"mu err {e_mu:.3e} (bar {2e-5 * np.abs(mu_ref).max():.3e}), var err {e_var:.3e} (bar {2e-5 * np.abs(var_ref).max():.3e})")
    assert np.abs(mu_ref).max() > 1e-2
    assert e_mu <= 2e-5 * np.abs(mu_ref).max()
    assert e_var <= 2e-5 * np.abs(var_ref).max()


def test_chain_prediction_of_a_matern52_plan(A, world):
    """agpl_plan_predict_chain on a plan of Gibbs sweeps (no marginal image) with another kernel, judged as
    tests/test_gpu_chain_predict.py judges the squared exponential: float64 with the plan's own (exact) features, element-wise bars."""
    from agpl_amd import _ffi

    ctx, _, ref = world
    kind, M, D, s2, T, L = K.MATERN52, 37, 1, 1.0, 3, 1
    x, z, ell = K.workload(N, M, D)
    rng = np.random.default_rng(31)
    lik, y = _data(A, 1, x, rng)
    gib = A.SparseGibbs.from_inputs(lik, dev(x), y, dev(z), ell, variance=s2, jitter=JITTER, ctx=ctx, kernel="matern52")
    p = gib.plan
    assert p.flags == A.Plan.NO_MARGINALS and p.kernel == "matern52"
    Phi = host(p.features()).astype(np.float64)
    # the plan holds THIS kernel's features: test_features_match_float64 judges their accuracy; here 1e-4 tells the kinds apart
    # (their features differ by more than 1e-3, test_kinds_differ)
    assert np.abs(Phi - ref(kind, M, D, s2)[0]).max() <= KIND_TOL
    V = rng.standard_normal((T, L, M))
    mu0 = (0.5 * rng.standard_normal((L, N))).astype(np.float32)
    Vd, xd, m0d = dev(V), dev(x), dev(mu0)
    f32 = torch.float32
    mean = torch.full((L, N), -7.0, dtype=f32, device="cuda")
    spread, resid = torch.full_like(mean, -7.0), torch.full((N,), -7.0, dtype=f32, device="cuda")
    F = torch.full((T, L, N), -7.0, dtype=f32, device="cuda")
    ptr = lambda t: C.c_void_p(t.data_ptr())
    p.call("agpl_plan_predict_chain", C.c_int32(T), ptr(Vd), C.c_int64(N), ptr(xd), ptr(m0d), ptr(mean), ptr(spread), ptr(resid), ptr(F),
           lib=_ffi.chain_lib())
    ctx.synchronize()
    r = R.reference(Phi, V, mu0.astype(np.float64))
    bars = R.bars(Phi, r, A.sparse.plan_padded(M), absolute=False)
    for name, got, want, bar in (("F", F, r.F, bars.F), ("mean", mean, r.mean, bars.mean), ("spread", spread, r.spread, bars.spread)):
        err = np.abs(host(got).astype(np.float64) - want)
        print(f"{name}: max err {err.max():.3e}, max err / bar {np.max(err / bar):.3f}")
        assert (err <= bar).all(), (name, np.max(err / bar))
    assert torch.equal(resid, p.resid)
    # the Python surface of the sampler
    mean2, var2, resid2, F2 = gib.predict(xd, Vd, m0d, samples=True)
    assert torch.equal(mean2, mean) and torch.equal(F2, F) and torch.equal(resid2, resid) and torch.equal(var2, spread + resid)


@pytest.mark.parametrize("M,D,s2", [(37, 1, 1.0), (300, 3, 2.5)])
def test_per_point_determinism_and_shards(A, world, M, D, s2):
    ctx, _, _ = world
    x, z, ell = K.workload(N, M, D)
    xd, zd = dev(x), dev(z)
    build = lambda xx: A.Plan.from_inputs(xx, zd, ell, variance=s2, jitter=JITTER, ctx=ctx, kernel="matern12")
    a, b = build(xd), build(xd)
    assert torch.equal(a.features(), b.features()) and torch.equal(a.resid, b.resid)
    part = build(xd[100:250].contiguous())  # starts and ends inside a tile
    assert torch.equal(part.features(), a.features()[100:250]) and torch.equal(part.resid, a.resid[100:250])


def test_ten_sweeps_matern52(A, oracle):
    """SparseCAVI.from_inputs(kernel="matern52").run(10) against the float64 oracle fed the plan's own decoded features, as
    tests/test_gpu_plan_inputs.py::test_ten_sweeps_from_inputs."""
    O = oracle
    lik, olik = A.BernoulliLikelihood(), O.bernoulli()
    Nn, M, D = 2000, 200, 3
    ctx = A.Context(0, seed=5)
    x, z, ell = K.workload(Nn, M, D)
    rng = np.random.default_rng(41)
    y_h = (rng.uniform(size=Nn) < 1 / (1 + np.exp(-2 * np.sin(x[:, 0]) * np.cos(0.5 * x[:, 1])))).astype(np.uint8)
    cavi = A.SparseCAVI.from_inputs(lik, dev(x), dev(y_h), dev(z), ell, ctx=ctx, kernel="matern52")
    assert cavi.Phi is None and cavi.plan.kernel == "matern52"
    F, kd = host(cavi.plan.features()), host(cavi.plan.resid).astype(np.float64)
    assert np.abs(F - K.phi_f64(K.MATERN52, x, z, ell, 1.0, 1e-8)[0]).max() <= KIND_TOL  # (Matern-5/2 features)
    cavi.run(10)
    cavi.check()
    S, m = np.eye(M)[None], np.zeros((1, M))
    for _ in range(10):
        G, g = O.cavi_pass(olik, F, kd, y_h, -S, m)
        S, m = O.gaussian_update(G, g)
    dG, dg = relmax(host(cavi.G), G), relmax(host(cavi.g), g)
    print(f"rel G {dG:.3e}, rel g {dg:.3e}")
    assert dG < NAT_TOL and dg < NAT_TOL, (dG, dg)


def test_errors_through_the_entry_point_leave_the_context_usable(A, world):
    from agpl_amd import _ffi

    ctx, _, _ = world
    x, z, ell = K.workload(N, 37, 1)
    for kind in (5, -1, 99):
        rc, p, msg = raw_plan(A, ctx, "stationary", kind, 0.0, x, z, ell)
        assert rc == _ffi.ERR_INVALID_ARGUMENT and p is None and "kind" in msg and str(kind) in msg, (kind, rc, msg)
    for alpha in (0.0, -1.0, float("nan"), float("inf")):
        rc, p, msg = raw_plan(A, ctx, "stationary", K.RQ, alpha, x, z, ell)
        assert rc == _ffi.ERR_INVALID_ARGUMENT and p is None and "param" in msg and "alpha" in msg, (alpha, rc, msg)
    # the contract of agpl_plan_create_se holds for every kind: a bad lengthscale is named too
    rc, p, msg = raw_plan(A, ctx, "stationary", K.MATERN32, 0.0, x, z, [0.0])
    assert rc == _ffi.ERR_INVALID_ARGUMENT and "lengthscale" in msg, (rc, msg)
    rc, p, msg = raw_plan(A, ctx, "stationary", K.RQ, 2.0, x, z, ell)
    assert rc == 0 and p is not None, msg
    assert np.abs(host(p.features()) - K.phi_f64(K.RQ, x, z, ell, 1.0, JITTER, 2.0)[0]).max() <= KIND_TOL
