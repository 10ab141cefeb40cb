"""GPU tests of the posterior of the gradient of f at new inputs (include/agpl_grad.h: agpl_plan_predict_grad; Plan.predict_grad,
SparseCAVI.predict_grad) against tests/predict_grad_reference.py (float64; proved against difference quotients of the posterior of f
in tests/test_predict_grad_reference_cpu.py), evaluated with the plan's own (U, v) read back.

The recipe is tests/test_gpu_kernels.py's: N = 300 training points, kernels_reference.workload, JITTER, a CAVI fit of 3 - 5 sweeps.
The bar is the project's own for prediction (tests/test_gpu_kernels.py::test_predict_at_new_inputs): 2e-5 x max |ref| per (l, d) row,
for the mean and for the variance -- dividing a row by its constant (sqrt c / ell_d, c / ell_d^2) shows it is the same computation
on psi_d that prediction runs on phi.

Measured on one MI355X (the largest err / max |ref| over the (l, d) rows of both shapes; the bar is 2e-5; the parity test prints
each row's figure before it asserts):
    kind        mean        variance
    se          9.5e-07     6.2e-07
    matern32    3.3e-07     1.9e-07
    matern52    3.8e-07     3.5e-07
    rq          6.5e-07     3.3e-07
"""
import ctypes as C

import numpy as np
import pytest

import kernels_reference as K
import predict_grad_reference as G

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

N, JITTER = K.N, K.JITTER
BAR = 2e-5
SHAPES = [(37, 1, 1.0), (300, 3, 2.5)]  # (M, D, s2)
IDS = [K.NAMES[k] for k in G.KINDS]
NS = 257  # two 128-point tiles and one point: the last tile is partial


@pytest.fixture(scope="module")
def A():
    import agpl_amd

    return agpl_amd


def host(t):
    return t.detach().cpu().numpy()


def dev(a, dtype=None):
    t = torch.from_numpy(np.array(a, copy=True)).cuda()  # (the shared inputs are read-only arrays)
    return t if dtype is None else t.to(dtype)


def data(A, L, x, rng):
    f = np.sin(x[:, 0])
    if L == 1:
        return A.BernoulliLikelihood(), dev((rng.uniform(size=len(x)) < 1 / (1 + np.exp(-2 * f))).astype(np.uint8))
    return A.HeteroscedasticGaussianLikelihood(2.0), dev((f + 0.3 * rng.standard_normal(len(x))).astype(np.float32))


def state(plan):
    """The plan's q(v) read back: U [L, M, M] lower triangular (S = U' U), v [L, M] (m = U' v)."""
    M = plan.M
    U = np.stack([np.tril(u.T[:M, :M]) for u in host(plan.U_colmajor)])
    return U, host(plan.v)[:, :M].copy()


@pytest.fixture(scope="module")
def world(A):
    """One context; the fits by (kind, M, D, s2, L) with their inputs and their (U, v), each made once and left unchanged."""
    ctx = A.Context(0, seed=13)
    fits = {}

    def fit(kind, M, D, s2, L=1, sweeps=5):
        key = (kind, M, D, s2, L)
        if key not in fits:
            x, z, ell = K.workload(N, M, D)
            lik, y = data(A, L, x, np.random.default_rng(22))
            cavi = A.SparseCAVI.from_inputs(lik, dev(x), y, dev(z), ell, variance=s2, jitter=JITTER, ctx=ctx,
                                            kernel=K.python_kernel(kind))
            cavi.run(sweeps)
            cavi.check()
            U, v = state(cavi.plan)
            for a in (x, z, ell, U, v):
                a.setflags(write=False)
            fits[key] = (cavi, x, z, ell, U, v)
        return fits[key]

    return ctx, fit


def reference(kind, xs, z, ell, s2, U, v, dims=None):
    return G.grad_moments(xs, z, ell, s2, JITTER, kind, K.param_of(kind), U, v, dims)


def row_errors(got, ref):
    """max |got - ref| / max |ref| per (l, d) row: [L, D]."""
    return np.abs(host(got).astype(np.float64) - ref).max(-1) / np.abs(ref).max(-1)


@pytest.mark.parametrize("M,D,s2", SHAPES)
@pytest.mark.parametrize("kind", G.KINDS, ids=IDS)
def test_parity_with_the_float64_reference(world, kind, M, D, s2):
    ctx, fit = world
    cavi, x, z, ell, U, v = fit(kind, M, D, s2)
    xs = np.random.default_rng(23).uniform(-12, 12, size=(NS, D))  # some outside the hull of z
    dmu, dvar = cavi.predict_grad(dev(xs))
    ctx.synchronize()
    assert dmu.shape == dvar.shape == (1, D, NS) and dmu.dtype == dvar.dtype == torch.float32
    rmu, rvar = reference(kind, xs, z, ell, s2, U, v)
    e_mu, e_var = row_errors(dmu, rmu), row_errors(dvar, rvar)
    print(f"PARITY {K.NAMES[kind]} M={M} D={D} s2={s2}: mean err / max|ref| per row {np.array2string(e_mu[0], precision=3)}, "
          f"var {np.array2string(e_var[0], precision=3)} (bar {BAR:.0e}); max |dmu_ref| {np.abs(rmu).max():.3e}")
    assert np.abs(rmu).max() > 1e-2
    assert torch.isfinite(dmu).all() and torch.isfinite(dvar).all() and (dvar >= 0).all()
    assert (e_mu <= BAR).all(), e_mu
    assert (e_var <= BAR).all(), e_var


def test_two_latents_and_the_output_pitch(world):
    """L = 2 (heteroscedastic), D = 3: every [l][d] row is that latent's and that dimension's alone -- the single-dimension,
    single-latent evaluation of the reference -- and the six rows are six different functions."""
    ctx, fit = world
    kind, (M, D, s2) = K.SE, SHAPES[1]
    cavi, x, z, ell, U, v = fit(kind, M, D, s2, L=2, sweeps=3)
    assert cavi.plan.L == 2 and U.shape == (2, M, M)
    xs = np.random.default_rng(24).uniform(-12, 12, size=(NS, D))
    dmu, dvar = cavi.predict_grad(dev(xs))
    ctx.synchronize()
    assert dmu.shape == dvar.shape == (2, D, NS)
    rows_mu, rows_var = [], []
    for l in range(2):
        for d in range(D):
            rmu, rvar = reference(kind, xs, z, ell, s2, U[l], v[l], dims=[d])
            e_mu = np.abs(host(dmu)[l, d] - rmu[0, 0]).max() / np.abs(rmu).max()
            e_var = np.abs(host(dvar)[l, d] - rvar[0, 0]).max() / np.abs(rvar).max()
            print(f"l={l} d={d}: mean {e_mu:.3e}, var {e_var:.3e}")
            assert e_mu <= BAR and e_var <= BAR, (l, d, e_mu, e_var)
            rows_mu.append(rmu[0, 0])
            rows_var.append(rvar[0, 0])
    for i in range(6):
        for j in range(i):  # distinct far beyond the bar: a row written to another row's place does not pass
            assert np.abs(rows_mu[i] - rows_mu[j]).max() > 100 * BAR * max(np.abs(rows_mu[i]).max(), np.abs(rows_mu[j]).max()), (i, j)
            assert np.abs(rows_var[i] - rows_var[j]).max() > 100 * BAR * max(rows_var[i].max(), rows_var[j].max()), (i, j)


def test_chunk_and_position_invariance_bit_for_bit(world):
    """Ns = 65536 + 129 is two chunks: a window across the seam and a window that starts off a 128-point tile boundary give, as calls
    of their own, the bytes they have inside the large call."""
    ctx, fit = world
    cavi, x, z, ell, U, v = fit(K.MATERN52, 37, 2, 1.0, sweeps=3)
    Ns = 65536 + 129
    xs = dev(np.random.default_rng(25).uniform(-12, 12, size=(Ns, 2)))
    dmu, dvar = cavi.predict_grad(xs)
    assert dmu.shape == (1, 2, Ns) and torch.isfinite(dmu).all() and torch.isfinite(dvar).all()
    assert dmu.abs().max() > 1e-2
    for a, b in ((65536 - 100, Ns), (77, 77 + 300), (65536, 65536 + 1)):
        pm, pv = cavi.predict_grad(xs[a:b].contiguous())
        assert torch.equal(pm, dmu[:, :, a:b]) and torch.equal(pv, dvar[:, :, a:b]), (a, b)


@pytest.mark.parametrize("kind", G.KINDS, ids=IDS)
def test_coincident_and_far_points(world, kind):
    """x_s = z_a exactly (u = 0, r = 0: the limit of kappa'(r) / r, no 0 / 0) is an ordinary point within the bar; at |x_s| = 1e3 ell
    the data say nothing: the mean tends to 0 and the variance to the prior's c s2 / ell_d^2."""
    ctx, fit = world
    for M, D, s2 in SHAPES:
        cavi, x, z, ell, U, v = fit(kind, M, D, s2)
        far = np.stack([1e3 * ell, -1e3 * ell])
        xs = np.concatenate([z[:31], far])
        dmu, dvar = cavi.predict_grad(dev(xs))
        ctx.synchronize()
        rmu, rvar = reference(kind, xs, z, ell, s2, U, v)
        assert torch.isfinite(dmu).all() and torch.isfinite(dvar).all() and (dvar >= 0).all()
        e_mu, e_var = row_errors(dmu, rmu), row_errors(dvar, rvar)
        print(f"{K.NAMES[kind]} M={M} D={D}: coincident + far rows, mean {e_mu.max():.3e}, var {e_var.max():.3e}")
        assert (e_mu <= BAR).all() and (e_var <= BAR).all(), (e_mu, e_var)
        prior = G.c_of(kind, K.param_of(kind)) * s2 / ell ** 2  # [D]
        m_far, v_far = host(dmu)[0, :, -2:].astype(np.float64), host(dvar)[0, :, -2:].astype(np.float64)
        assert (np.abs(m_far) <= BAR * np.sqrt(prior)[:, None]).all(), m_far
        assert (np.abs(v_far - prior[:, None]) <= BAR * prior[:, None]).all(), v_far / prior[:, None] - 1


def test_neighbours_are_unchanged(world):
    """The shared scratch and the shared generator: after a predict_grad call, predict at the training inputs is still marginals()
    bit for bit and the plan's features are what they were."""
    ctx, fit = world
    cavi, x, z, ell, U, v = fit(K.RQ, 300, 3, 2.5)
    before = cavi.plan.features().clone()
    mu_m, var_m = (t.clone() for t in cavi.marginals())
    cavi.predict_grad(dev(np.random.default_rng(26).uniform(-12, 12, size=(1000, 3))))  # (grows the scratch past predict's own)
    mu_t, var_t = cavi.predict(dev(x))
    assert torch.equal(mu_t, mu_m) and torch.equal(var_t, var_m)
    mu_m2, var_m2 = cavi.marginals()
    assert torch.equal(mu_m2, mu_m) and torch.equal(var_m2, var_m)
    assert torch.equal(cavi.plan.features(), before)
    U2, v2 = state(cavi.plan)
    assert np.array_equal(U2, U) and np.array_equal(v2, v)


def test_errors_and_edge_cases(A, world):
    from agpl_amd import _ffi

    ctx, fit = world
    ptr = lambda t: C.c_void_p(0 if t is None else t.data_ptr())
    raw = lambda plan, Ns, xs, dmu, dvar: plan.call("agpl_plan_predict_grad", C.c_int64(Ns), ptr(xs), ptr(dmu), ptr(dvar),
                                                    lib=_ffi.grad_lib())
    M, D, s2 = SHAPES[0]
    x, z, ell = K.workload(N, M, D)
    xs = dev(np.random.default_rng(27).uniform(-12, 12, size=(NS, D)))
    out = lambda: torch.full((1, D, NS), -7.0, dtype=torch.float32, device="cuda")
    # Matern-1/2 is not differentiable: refused by name, nothing written
    m12 = A.Plan.from_inputs(dev(x), dev(z), ell, variance=s2, jitter=JITTER, ctx=ctx, kernel="matern12")
    with pytest.raises(A.AGPLError) as ei:
        m12.predict_grad(xs)
    assert ei.value.code == _ffi.ERR_UNSUPPORTED and "Matern-1/2" in str(ei.value)
    # a plan without the marginal image; a plan of given features; both outputs NULL; a negative count; a null x_s
    nom = A.Plan.from_inputs(dev(x), dev(z), ell, variance=s2, jitter=JITTER, ctx=ctx, flags=A.Plan.NO_MARGINALS)
    with pytest.raises(A.ArgumentError) as ei:
        nom.predict_grad(xs)
    assert ei.value.code == _ffi.ERR_INVALID_ARGUMENT and "NO_MARGINALS" in str(ei.value)
    cavi, _, _, _, U, v = fit(K.SE, M, D, s2)
    given = A.Plan(cavi.plan.features(), cavi.plan.resid, 1, ctx)
    a, b = out(), out()
    with pytest.raises(A.ArgumentError) as ei:
        raw(given, NS, xs, a, b)
    assert ei.value.code == _ffi.ERR_INVALID_ARGUMENT and "raw inputs" in str(ei.value)
    with pytest.raises(A.ArgumentError):
        given.predict_grad(xs)
    for args in ((NS, xs, None, None), (-1, xs, a, b), (NS, None, a, b)):
        with pytest.raises(A.ArgumentError) as ei:
            raw(cavi.plan, *args)
        assert ei.value.code == _ffi.ERR_INVALID_ARGUMENT
    ctx.synchronize()
    assert (a == -7.0).all() and (b == -7.0).all()
    # Ns = 0 is fine and writes nothing; wrong input shapes are refused before the call
    raw(cavi.plan, 0, None, None, None)
    e_mu, e_var = cavi.predict_grad(xs[:0])
    assert e_mu.shape == e_var.shape == (1, D, 0)
    with pytest.raises(A.ArgumentError):
        cavi.predict_grad(torch.zeros((4, D + 1), dtype=torch.float64, device="cuda"))
    # the context serves a correct call afterwards; either output alone is the same bytes
    dmu, dvar = cavi.predict_grad(xs)
    rmu, rvar = reference(K.SE, host(xs), z, ell, s2, U, v)
    assert (row_errors(dmu, rmu) <= BAR).all() and (row_errors(dvar, rvar) <= BAR).all()
    raw(cavi.plan, NS, xs, a, None)
    raw(cavi.plan, NS, xs, None, b)
    assert torch.equal(a, dmu) and torch.equal(b, dvar)
    # a non-finite row: NaN for that point, the clean run's bytes for every other point
    bad = xs.clone()
    bad[130, 0] = float("nan")
    bad[5, D - 1] = float("inf")
    nmu, nvar = cavi.predict_grad(bad)
    keep = torch.ones(NS, dtype=torch.bool, device="cuda")
    keep[[5, 130]] = False
    assert torch.isnan(nmu[:, :, ~keep]).all() and torch.isnan(nvar[:, :, ~keep]).all()
    assert torch.equal(nmu[:, :, keep], dmu[:, :, keep]) and torch.equal(nvar[:, :, keep], dvar[:, :, keep])
    again = cavi.predict_grad(xs)
    assert torch.equal(again[0], dmu) and torch.equal(again[1], dvar)


def test_python_surface(A, world):
    ctx, fit = world
    cavi, x, z, ell, U, v = fit(K.MATERN32, 37, 1, 1.0)
    xs = dev(np.random.default_rng(28).uniform(-12, 12, size=NS))  # [Ns] for D = 1
    a = cavi.predict_grad(xs)
    b = cavi.plan.predict_grad(xs.unsqueeze(1))
    assert isinstance(a, tuple) and len(a) == 2
    for s, t in zip(a, b):
        assert s.shape == (1, 1, NS) and s.dtype == torch.float32 and s.is_cuda and torch.equal(s, t)
    lik, y = data(A, 1, x, np.random.default_rng(22))
    Phi = cavi.plan.features()
    with pytest.raises(A.ArgumentError):  # an object of given features has no inputs to differentiate
        A.SparseCAVI(lik, Phi, cavi.plan.resid, y, ctx=ctx).predict_grad(xs)
