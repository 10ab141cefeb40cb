"""GPU tests of prediction from a chain of inducing draws (include/agpl_chain.h: agpl_plan_predict_chain; csrc/agpl_chain.hip;
Plan.predict_chain, SparseGibbs.predict / predict_y / heldout_logp):

* the projection against float64 with the plan's own (exact) features, element-wise bars from the arithmetic of the kernel;
* the spread of a tight chain far from the origin (centred projections, not a difference of sums); T = 1 gives exactly 0;
* new inputs against a float64 restatement of L^-1 K_ZX;
* per-point determinism across chunks, positions and calls; a plan without the marginal image gives the same bits;
* the Rao-Blackwellised mixture of y against operators.predictive per draw combined in numpy;
* argument and domain errors, after which the context still works.

Shapes: D = 2, N = 300 (two full 128-point tiles and a ragged one), M = 64 and 200 (both pad to 256), T = 1, 37, 130 (the 128-draw
block), L = 1, 2.
"""
import ctypes as C

import numpy as np
import pytest

import chain_reference as R

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

N, D, MP = 300, 2, 256
JITTER = 1e-8


@pytest.fixture(scope="module")
def A():
    import agpl_amd

    return agpl_amd


def host(t):
    return t.detach().cpu().numpy()


def dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    return t if dtype is None else t.to(dtype)


def relmax(a, b):
    return np.abs(np.asarray(a, np.float64) - b).max() / max(np.abs(b).max(), 1e-300)


inputs = R.se_inputs  # x [N, 2] in the square, z on a grid over it, lengthscales of 0.9 grid steps


def se_kernel(a, b, ell, s2=1.0):
    d = (a[:, None, :] - b[None, :, :]) / ell
    return s2 * np.exp(-0.5 * (d * d).sum(-1))


def phi_f64(x, z, ell):
    """Phi [n, M] = (L^-1 K_ZX)' in float64 (the helper of tests/test_gpu_plan_inputs.py, restated)."""
    Lc = np.linalg.cholesky(se_kernel(z, z, ell) + JITTER * np.eye(len(z)))
    return np.linalg.solve(Lc, se_kernel(z, x, ell)).T


@pytest.fixture(scope="module")
def world(A):
    """One context, the plans by (M, L) built once, and their features in float64 (exact: hi + lo of the image)."""
    ctx = A.Context(0, seed=11)
    plans, feats = {}, {}

    def plan(M, L, flags=0):
        key = (M, L, flags)
        if key not in plans:
            x, z, ell = inputs(M)
            plans[key] = A.Plan.from_inputs(dev(x), dev(z), ell, jitter=JITTER, L=L, ctx=ctx, flags=flags)
        return plans[key]

    def features(M):
        if M not in feats:
            feats[M] = host(plan(M, 1).features()).astype(np.float64)
        return feats[M]

    return ctx, plan, features


def raw_chain(plan, V, x_s, mu0_s=None, samples=True):
    """The C entry point with its own outputs: (mean, spread, resid, F) -- Plan.predict_chain returns var = resid + spread."""
    from agpl_amd import _ffi

    T, Ns, L = V.shape[0], x_s.shape[0], plan.L
    f32 = torch.float32
    mean = torch.full((L, Ns), -7.0, dtype=f32, device="cuda")
    spread, resid = torch.full_like(mean, -7.0), torch.full((Ns,), -7.0, dtype=f32, device="cuda")
    F = torch.full((T, L, Ns), -7.0, dtype=f32, device="cuda") if samples else None
    ptr = lambda t: C.c_void_p(0 if t is None else t.data_ptr())
    plan.call("agpl_plan_predict_chain", C.c_int32(T), ptr(V), C.c_int64(Ns), ptr(x_s), ptr(mu0_s), ptr(mean), ptr(spread), ptr(resid),
              ptr(F), lib=_ffi.chain_lib())
    return mean, spread, resid, F


@pytest.mark.parametrize("M", [64, 200])
@pytest.mark.parametrize("L", [1, 2])
@pytest.mark.parametrize("T", [1, 37, 130])
def test_projection_against_float64_with_exact_features(world, M, L, T):
    ctx, plan, features = world
    p, Phi = plan(M, L), features(M)
    rng = np.random.default_rng(1000 * M + 10 * T + L)
    V = rng.standard_normal((T, L, M))  # independent rows per latent: a latent mix-up shows
    with_mu0 = (T + L) % 2 == 0  # both cases occur over the parametrisation, for every M
    mu0 = (0.5 * rng.standard_normal((L, N))).astype(np.float32) if with_mu0 else None
    x = dev(inputs(M)[0])
    mean, spread, resid, F = raw_chain(p, dev(V), x, None if mu0 is None else dev(mu0))
    ctx.synchronize()
    m0 = None if mu0 is None else mu0.astype(np.float64)
    ref = R.reference(Phi, V, m0)
    bars = R.bars(Phi, ref, MP, absolute=False)
    err, bar = np.abs(host(F).astype(np.float64) - ref.F), bars.F
    print(f"F: max err {err.max():.3e}, max err / bar {np.max(err / bar):.3f}")
    assert (err <= bar).all(), np.max(err / bar)
    err_m, bar_m = np.abs(host(mean).astype(np.float64) - ref.mean), bars.mean
    print(f"mean: max err {err_m.max():.3e}, max err / bar {np.max(err_m / bar_m):.3f}")
    assert (err_m <= bar_m).all(), np.max(err_m / bar_m)
    assert torch.equal(resid, p.resid)
    if T == 1:
        assert torch.equal(spread, torch.zeros_like(spread))
    # the Python surface: var = resid + spread, the same mean and samples
    mean2, var2, resid2, F2 = p.predict_chain(dev(V), x, None if mu0 is None else dev(mu0), samples=True)
    assert torch.equal(mean2, mean) and torch.equal(F2, F) and torch.equal(resid2, resid)
    assert torch.equal(var2, spread + resid)


@pytest.mark.parametrize("M", [64, 200])
@pytest.mark.parametrize("L", [1, 2])
def test_spread_of_a_tight_chain(world, M, L):
    ctx, plan, features = world
    p, Phi = plan(M, L), features(M)
    rng = np.random.default_rng(77 + M + L)
    T = 37
    V = R.tight(rng, T, L, M)
    x = dev(inputs(M)[0])
    _, spread, _, _ = raw_chain(p, dev(V), x, samples=False)
    ref = R.reference(Phi, V)
    spread_ref = ref.spread  # = the population variance of F_ref over t
    assert np.allclose(spread_ref, ref.F.var(0), rtol=1e-6, atol=0)
    bar = R.bars(Phi, ref, MP, absolute=False).spread
    err = np.abs(host(spread).astype(np.float64) - spread_ref)
    print(f"spread: ref max {spread_ref.max():.3e}, max err {err.max():.3e}, max err / bar {np.max(err / bar):.3f}")
    assert (err <= bar).all(), np.max(err / bar)
    # a single draw has no spread, whatever its size
    _, one, _, _ = raw_chain(p, dev(V[:1]), x, samples=False)
    assert torch.equal(one, torch.zeros_like(one))


@pytest.mark.parametrize("M", [64, 200])
def test_new_inputs_against_float64(world, M):
    ctx, plan, _ = world
    p = plan(M, 1)
    _, z, ell = inputs(M)
    rng = np.random.default_rng(5 + M)
    Ns, T = 257, 37
    xs = rng.uniform(-13, 13, size=(Ns, D))  # off the training set, some outside the hull of z
    V = rng.standard_normal((T, 1, M))
    mu0 = (0.5 * rng.standard_normal((1, Ns))).astype(np.float32)
    mean, var, resid, F = p.predict_chain(dev(V), dev(xs), dev(mu0), samples=True)
    phis = phi_f64(xs, z, ell)
    F_ref = mu0.astype(np.float64) + np.einsum("na,tla->tln", phis, V)
    mean_ref = F_ref.mean(0)
    e_F, e_m = np.abs(host(F) - F_ref).max(), np.abs(host(mean) - mean_ref).max()
    print(f"F: max err {e_F:.3e} (bar {2e-5 * np.abs(F_ref).max():.3e}); mean: {e_m:.3e} (bar {2e-5 * np.abs(mean_ref).max():.3e})")
    assert e_F <= 2e-5 * np.abs(F_ref).max()
    assert e_m <= 2e-5 * np.abs(mean_ref).max()
    assert np.isfinite(host(var)).all() and (host(var) >= host(resid)).all()


def test_position_independence(world, A):
    ctx, plan, _ = world
    M, L, T = 64, 2, 5
    p = plan(M, L)
    rng = np.random.default_rng(9)
    Ns = 65536 + 300  # two chunks
    xs = dev(rng.uniform(-10, 10, size=(Ns, D)))
    V = dev(rng.standard_normal((T, L, M)))
    mu0 = dev((0.5 * rng.standard_normal((L, Ns))).astype(np.float32))
    full = raw_chain(p, V, xs, mu0)
    again = raw_chain(p, V, xs, mu0)
    for a, b in zip(full, again):
        assert torch.equal(a, b)
    idx = torch.tensor([65835, 0, 65536, 127, 5, 128, 65535, 4097, 65537, 300, 31999, 65700], device="cuda")
    sub = raw_chain(p, V, xs[idx].contiguous(), mu0[:, idx].contiguous())
    assert torch.equal(sub[0], full[0][:, idx]) and torch.equal(sub[1], full[1][:, idx])
    assert torch.equal(sub[2], full[2][idx]) and torch.equal(sub[3], full[3][:, :, idx])
    # a plan without the marginal image (the plan of Gibbs sweeps) holds the same generator: the same bits
    bare = plan(M, L, A.Plan.NO_MARGINALS)
    for a, b in zip(raw_chain(bare, V, xs[idx].contiguous(), mu0[:, idx].contiguous()), sub):
        assert torch.equal(a, b)


def _mixture_data(A, name, rng):
    x, z, ell = inputs(64)
    f = np.sin(x[:, 0]) * np.cos(0.5 * x[:, 1])
    if name == "bernoulli":
        lik = A.BernoulliLikelihood()
        y = (rng.uniform(size=N) < 1 / (1 + np.exp(-2 * f))).astype(np.uint8)
    else:
        lik = A.HeteroscedasticGaussianLikelihood(2.0)
        y = f + 0.3 * rng.standard_normal(N)
    return lik, x, y, z, ell


@pytest.mark.parametrize("name", ["bernoulli", "heterogauss"])
def test_mixture_of_y(A, name):
    rng = np.random.default_rng(31)
    lik, x, y, z, ell = _mixture_data(A, name, rng)
    L = lik._nlatent
    ctx = A.Context(0, seed=21)
    gib = A.SparseGibbs.from_inputs(lik, dev(x), dev(y), dev(z), ell, jitter=JITTER, ctx=ctx)
    T, Ns = 20, 200
    chain = gib.run(T)
    xs = x[:Ns] + 0.05
    xs_d, ys_d = dev(xs), dev(y[:Ns])
    mean, var, resid, F = gib.predict(xs_d, chain, samples=True)
    assert tuple(mean.shape) == (L, Ns) and tuple(var.shape) == (L, Ns) and tuple(F.shape) == (T, L, Ns)
    assert torch.isfinite(mean).all() and torch.isfinite(var).all() and (var >= resid).all()
    ey, vy, lp = gib.predict_y(xs_d, chain, ys_d)
    total = gib.heldout_logp(xs_d, ys_d, chain)
    # the reference: operators.predictive per draw on the device F[t] and resid, combined in numpy float64
    d = resid.to(torch.float64)
    d = d if L == 1 else d.unsqueeze(1).expand(Ns, L).contiguous()
    E, Vr, LP = [], [], []
    for t in range(T):
        f = F[t, 0].to(torch.float64) if L == 1 else F[t].t().contiguous().to(torch.float64)
        m, v, lg = A.predictive(lik, (f, d), ys_d, ctx=ctx)
        E.append(host(m)), Vr.append(host(v)), LP.append(host(lg))
    E, Vr, LP = np.array(E), np.array(Vr), np.array(LP)
    ey_ref = E.mean(0)
    vy_ref = (Vr + E * E).mean(0) - ey_ref ** 2
    mx = LP.max(0)
    lp_ref = mx + np.log(np.exp(LP - mx).sum(0)) - np.log(T)
    print(f"E[y] {relmax(host(ey), ey_ref):.2e}  Var[y] {relmax(host(vy), vy_ref):.2e}  log p {relmax(host(lp), lp_ref):.2e}")
    assert relmax(host(ey), ey_ref) <= 1e-12
    assert relmax(host(lp), lp_ref) <= 1e-12
    assert relmax(host(vy), vy_ref) <= 1e-10
    assert abs(total - host(lp).sum()) <= 1e-12 * abs(host(lp).sum())


def test_errors_leave_the_context_usable(A):
    from agpl_amd import _ffi

    ctx = A.Context(0, seed=3)
    M = 64
    x, z, ell = inputs(M)
    rng = np.random.default_rng(2)
    xd, zd = dev(x), dev(z)
    plan = A.Plan.from_inputs(xd, zd, ell, jitter=JITTER, ctx=ctx)
    V = dev(rng.standard_normal((20, 1, M)))
    # a plan from materialised features has no generator
    Phi = dev((rng.standard_normal((N, M)) / np.sqrt(M)).astype(np.float32))
    kd = torch.ones(N, device="cuda")
    flat = A.Plan(Phi, kd, 1, ctx)
    with pytest.raises(A.ArgumentError):
        flat.predict_chain(V, xd)
    out = torch.empty((1, N), dtype=torch.float32, device="cuda")
    ptr = lambda t: C.c_void_p(t.data_ptr())
    rc = _ffi.chain_lib().agpl_plan_predict_chain(flat._h, C.c_int32(20), ptr(V), C.c_int64(N), ptr(xd), None, ptr(out), ptr(out), None,
                                                  None)
    assert rc == _ffi.ERR_INVALID_ARGUMENT
    lik = A.BernoulliLikelihood()
    y = dev((rng.uniform(size=N) < 0.5).astype(np.uint8))
    with pytest.raises(A.ArgumentError):
        A.SparseGibbs(lik, Phi, kd, y, ctx=ctx).predict(xd, V)
    # T = 0
    with pytest.raises(A.ArgumentError):
        plan.predict_chain(V[:0], xd)
    rc = _ffi.chain_lib().agpl_plan_predict_chain(plan._h, C.c_int32(0), ptr(V), C.c_int64(N), ptr(xd), None, ptr(out), ptr(out), None,
                                                  None)
    assert rc == _ffi.ERR_INVALID_ARGUMENT
    # a non-finite draw is named
    Vb = V.clone()
    Vb[13, 0, 7] = float("nan")
    Vb[17, 0, 3] = float("inf")
    with pytest.raises(A.DomainError, match="13"):
        plan.predict_chain(Vb, xd)
    # a non-finite input spoils its own point only
    xb = xd.clone()
    xb[5, 1] = float("nan")
    mean, var, resid, F = plan.predict_chain(V, xb, samples=True)
    good = torch.ones(N, dtype=torch.bool, device="cuda")
    good[5] = False
    assert torch.isnan(mean[:, 5]).all() and torch.isnan(var[:, 5]).all() and torch.isnan(F[:, :, 5]).all()
    assert torch.isfinite(mean[:, good]).all() and torch.isfinite(var[:, good]).all() and torch.isfinite(F[:, :, good]).all()
    ref = plan.predict_chain(V, xd, samples=True)
    assert torch.equal(mean[:, good], ref[0][:, good]) and torch.equal(F[:, :, good], ref[3][:, :, good])
    # the same context: a fresh build, two sweeps and a prediction
    gib = A.SparseGibbs.from_inputs(lik, xd, y, zd, ell, jitter=JITTER, ctx=ctx)
    chain = gib.run(2)
    mean, var, _ = gib.predict(xd, chain)
    assert torch.isfinite(chain).all() and torch.isfinite(mean).all() and torch.isfinite(var).all()
