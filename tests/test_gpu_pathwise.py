"""GPU tests of pathwise posterior function draws (include/agpl_pathwise.h: agpl_plan_sample_paths; csrc/agpl_pathwise.hip;
Plan.sample_paths, SparseCAVI.sample_paths, SparseGibbs.sample_paths, Paths):

* the draws against the float64 reference with the plan's own (exact) features, inside the element-wise bars of
  tests/pathwise_reference.py, on its cases (M = 5, 64, 300; F = 16, 100, 1000; L = 1, 3; D = 1, 3, 16; the five kinds; T L = 1, 33,
  128, 129; mu0 and Xi present and absent; jitter 1e-6 and 1e-3), with Ns = 0, 1, 127, 128, 129, 257;
* determinism and position independence, bitwise: alone, inside a larger call, at another position, across the sub-chunk seam
  (F = 8192: sub-chunks of 8192 points), through a plan with and without the marginal image;
* W = 0, Xi = NULL against predict_chain's per-draw means;
* the sample mean and covariance of 4096 paths of a trained SparseCAVI against predict and C_model (every entry, 5 sigma);
* re-evaluation of a Paths object; SparseGibbs.sample_paths against the reference given the chain;
* argument and domain errors, a non-finite x, after which the context still works.
"""
import ctypes as C

import numpy as np
import pytest

import chain_reference as CR
import pathwise_reference as R

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")


@pytest.fixture(scope="module")
def A():
    import agpl_amd

    return agpl_amd


def host(t):
    return t.detach().cpu().numpy()


def dev(a, dtype=None):
    if a is None:
        return None
    t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    return t if dtype is None else t.to(dtype)


def kernel_arg(kind):
    return ("rq", R.ALPHA) if kind == "rq" else kind


def raw_paths(plan, V, omega, phase, W, Xi, x_s, mu0_s=None, fill=-7.0):
    """The C entry point on device tensors: F [T, L, Ns] float32."""
    from agpl_amd import _ffi

    T, Fn, Ns = V.shape[0], omega.shape[0], x_s.shape[0]
    out = torch.full((T, plan.L, Ns), fill, dtype=torch.float32, device="cuda")
    ptr = lambda t: C.c_void_p(0 if t is None else t.data_ptr())
    plan.call("agpl_plan_sample_paths", C.c_int32(T), ptr(V), C.c_int32(Fn), ptr(omega), ptr(phase), ptr(W), ptr(Xi), C.c_int64(Ns),
              ptr(x_s), ptr(mu0_s), ptr(out), lib=_ffi.pathwise_lib())
    return out


@pytest.fixture(scope="module")
def ctx(A):
    return A.Context(0, seed=17)


def make_plan(A, ctx, c, flags=0):
    x, z, ell = R.case_inputs(c)
    return A.Plan.from_inputs(dev(x), dev(z), ell, variance=R.VARIANCE, jitter=c.jitter, L=c.L, ctx=ctx, flags=flags,
                              kernel=kernel_arg(c.kind))


@pytest.mark.parametrize("c", R.CASES, ids=lambda c: c.id)
def test_draws_against_float64_with_exact_features(A, ctx, c):
    plan = make_plan(A, ctx, c)
    x, z, ell = R.case_inputs(c)
    draws = R.case_draws(c)
    omega, phase, V, W, Xi, mu0 = draws
    Phi = host(plan.features()).astype(np.float64)
    ref, bars, cc = R.case_reference(c, Phi, x, z, ell, draws, plan.scale_exp)
    d = [dev(a) for a in (V, omega, phase, W, Xi)]
    xd, md = dev(x), dev(mu0)
    F = raw_paths(plan, *d, xd, md)
    ctx.synchronize()
    err = np.abs(host(F).astype(np.float64) - ref)
    print(f"{c.id}: max |c| {np.abs(cc).max():.3e}, max |F| {np.abs(ref).max():.3e}, max err {err.max():.3e}, "
          f"max err / bar {np.max(err / bars.F):.3f} (bar parts at the worst entry: rel {bars.rel.flat[np.argmax(err / bars.F)]:.2e} "
          f"abs {bars.abs.flat[np.argmax(err / bars.F)]:.2e} cos {bars.cos.flat[np.argmax(err / bars.F)]:.2e})")
    assert (err <= bars.F).all(), np.max(err / bars.F)
    # the same bits again, and at every Ns: a value depends on its input alone
    assert torch.equal(raw_paths(plan, *d, xd, md), F)
    for Ns in (0, 1, 127, 128, 129):
        sub = raw_paths(plan, *d, xd[:Ns].contiguous(), None if md is None else md[:, :Ns].contiguous())
        assert tuple(sub.shape) == (c.T, c.L, Ns) and torch.equal(sub, F[:, :, :Ns])


def test_position_independence_and_the_sub_chunk_seam(A, ctx):
    c = R.Case("se", 5, 8192, 2, 3, 3, 1e-6, True, True)
    plan = make_plan(A, ctx, c)
    rng = np.random.default_rng(9)
    Ns = 8192 + 129  # the Psi image of F = 8192 holds 8192 points: two sub-chunks
    xs = dev(rng.uniform(-3, 3, size=(Ns, c.D)))
    mu0 = dev((0.5 * rng.standard_normal((c.L, Ns))).astype(np.float32))
    omega, phase = R.spectral(c.kind, c.F, c.D, rng)
    d = [dev(a) for a in (rng.standard_normal((c.T, c.L, c.M)), omega, phase, rng.standard_normal((c.T, c.L, c.F)),
                          rng.standard_normal((c.T, c.L, c.M)))]
    full = raw_paths(plan, *d, xs, mu0)
    assert torch.equal(raw_paths(plan, *d, xs, mu0), full)
    idx = torch.tensor([8320, 0, 8192, 127, 5, 128, 8191, 4097, 8193, 300], device="cuda")
    sub = raw_paths(plan, *d, xs[idx].contiguous(), mu0[:, idx].contiguous())
    assert torch.equal(sub, full[:, :, idx])
    one = raw_paths(plan, *d, xs[8192:8193].contiguous(), mu0[:, 8192:8193].contiguous())
    assert torch.equal(one, full[:, :, 8192:8193])
    # a plan without the marginal image (the plan of Gibbs sweeps) holds the same generator: the same bits
    bare = make_plan(A, ctx, c, A.Plan.NO_MARGINALS)
    assert torch.equal(raw_paths(bare, *d, xs[idx].contiguous(), mu0[:, idx].contiguous()), sub)


def test_zero_weights_give_predict_chain(A, ctx):
    """W = 0, Xi = NULL: c = V and the draw is mu0 + phi' V_t, predict_chain's per-draw mean, within the sum of the two calls' bars."""
    c = R.Case("matern32", 64, 100, 3, 43, 3, 1e-6, True, False)
    plan = make_plan(A, ctx, c)
    x, z, ell = R.case_inputs(c)
    omega, phase, V, W, _, mu0 = R.case_draws(c)
    W0 = np.zeros_like(W)
    Phi = host(plan.features()).astype(np.float64)
    F = raw_paths(plan, dev(V), dev(omega), dev(phase), dev(W0), None, dev(x), dev(mu0))
    Fc = plan.predict_chain(dev(V), dev(x), dev(mu0), samples=True)[3]
    cref = CR.reference(Phi, V, mu0.astype(np.float64))
    bar_c = CR.bars(Phi, cref, CR.plan_padded(c.M)).F
    ref = R.reference(Phi, R.psi_f64(x, ell, omega, phase), V, W0, 0.0, mu0)
    bar_p = R.bars(Phi, R.psi_f64(x, ell, omega, phase), V, W0, np.sqrt(R.VARIANCE * 2.0 / c.F), ref, plan.scale_exp).F
    err = np.abs(host(F).astype(np.float64) - host(Fc).astype(np.float64))
    print(f"max |paths - predict_chain| {err.max():.3e}, max err / (sum of bars) {np.max(err / (bar_c + bar_p)):.3f}")
    assert (err <= bar_c + bar_p).all()
    assert (np.abs(host(F) - ref) <= bar_p).all()


def _trained_cavi(A, ctx):
    rng = np.random.default_rng(41)
    N, M = 2000, 32
    x = rng.uniform(-3, 3, size=(N, 1))
    y = (rng.uniform(size=N) < 1 / (1 + np.exp(-2 * np.sin(2 * x[:, 0])))).astype(np.uint8)
    z = np.linspace(-3, 3, M)[:, None]
    ell, jitter = 0.3, 1e-6  # 1.5 grid steps: K_ZZ is well conditioned, the float32 generator's features are close to float64's
    cavi = A.SparseCAVI.from_inputs(A.BernoulliLikelihood(), dev(x), dev(y), dev(z), ell, variance=1.5, jitter=jitter, ctx=ctx)
    cavi.run(10)
    return cavi, z, np.array([ell]), 1.5, jitter


def test_statistics_of_paths_from_a_trained_cavi(A, ctx):
    cavi, z, ell, s2, jitter = _trained_cavi(A, ctx)
    T, Fn = 4096, 2048
    gen = torch.Generator(device="cuda").manual_seed(2024)
    paths = cavi.sample_paths(T, nfeatures=Fn, generator=gen)
    xs = np.linspace(-2.9, 2.9, 9)[:, None] + 0.013
    f = host(paths(dev(xs))).astype(np.float64)[:, 0]
    assert f.shape == (T, 9)
    mu, var = (host(t).astype(np.float64)[0] for t in cavi.predict(dev(xs)))
    Linv = R.whitening("se", z / ell, 1.0, s2, jitter)
    Phi = R.phi_f64("se", xs / ell, z / ell, 1.0, s2, Linv)
    S = host(cavi.S)[0][: len(z), : len(z)]
    omega, phase = host(paths.omega), host(paths.phase)
    Cm = R.c_model(Phi, R.psi_f64(xs, ell, omega, phase), R.psi_f64(z, ell, omega, phase), Linv, S, np.sqrt(s2 * 2.0 / Fn), jitter)
    Ce = R.c_exact(R.kernel_matrix("se", xs / ell, xs / ell, 1.0, s2), Phi, S)
    print(f"max |C_model - C_exact| {np.abs(Cm - Ce).max():.4f} at max |C| {np.abs(Ce).max():.3f}; predict's var against diag C_exact "
          f"{np.abs(var - np.diag(Ce)).max():.2e}")
    em, bm = np.abs(f.mean(0) - mu), 5 * np.sqrt(np.diag(Cm) / T) + 1e-5 * (1 + np.abs(mu))
    print(f"mean: max err {em.max():.4f}, max err / bar {np.max(em / bm):.3f}")
    assert (em <= bm).all()
    err, bar = np.abs(np.cov(f.T, bias=True) - Cm), R.mc_bar(Cm, T)
    print(f"covariance: max err {err.max():.4f}, max err / bar {np.max(err / bar):.3f}")
    assert (err <= bar).all()
    # the same seed gives the same paths
    again = cavi.sample_paths(T, nfeatures=Fn, generator=torch.Generator(device="cuda").manual_seed(2024))
    assert torch.equal(again(dev(xs)), paths(dev(xs)))


def test_a_paths_object_is_a_function(A, ctx):
    """Evaluated at x_a, then at x_b, it gives what one evaluation at their union gives, bit for bit."""
    c = R.Case("matern52", 64, 100, 3, 5, 3, 1e-6, False, True)
    plan = make_plan(A, ctx, c)
    rng = np.random.default_rng(3)
    V = dev(rng.standard_normal((c.T, c.L, c.M)))
    paths = plan.sample_paths(V=V, nfeatures=c.F, generator=torch.Generator(device="cuda").manual_seed(5))
    xa, xb = dev(rng.uniform(-3, 3, size=(130, c.D))), dev(rng.uniform(-3, 3, size=(77, c.D)))
    fa, fb, fu = paths(xa), paths(xb), paths(torch.cat([xa, xb]))
    assert tuple(fu.shape) == (c.T, c.L, 207) and fu.dtype == torch.float32
    assert torch.equal(torch.cat([fa, fb], dim=2), fu)
    assert torch.equal(paths(xa), fa)


def test_paths_from_a_gibbs_chain(A, ctx):
    rng = np.random.default_rng(8)
    N, M, T, Fn = 300, 16, 6, 100
    x = rng.uniform(-3, 3, size=(N, 1))
    y = (rng.uniform(size=N) < 1 / (1 + np.exp(-2 * np.sin(2 * x[:, 0])))).astype(np.uint8)
    z, ell, jitter = np.linspace(-3, 3, M)[:, None], np.array([0.6]), 1e-6
    gib = A.SparseGibbs.from_inputs(A.BernoulliLikelihood(), dev(x), dev(y), dev(z), 0.6, jitter=jitter, ctx=ctx)
    chain = gib.run(T)
    paths = gib.sample_paths(chain, nfeatures=Fn, generator=torch.Generator(device="cuda").manual_seed(1))
    F = paths(dev(x))  # at the training inputs the plan's own features are known exactly
    assert tuple(F.shape) == (T, 1, N) and torch.equal(paths.V, chain)
    Phi = host(gib.plan.features()).astype(np.float64)
    Linv = R.whitening("se", z / ell, 1.0, 1.0, jitter)
    omega, phase, W, Xi = (host(t) for t in (paths.omega, paths.phase, paths.W, paths.Xi))
    s = np.sqrt(2.0 / Fn)
    cc = R.coefficients(host(chain), W, Xi, R.psi_f64(z, ell, omega, phase), Linv, s, jitter)
    Psi = R.psi_f64(x, ell, omega, phase)
    ref = R.reference(Phi, Psi, cc, W, s)
    bar = R.bars(Phi, Psi, cc, W, s, ref, gib.plan.scale_exp, 2 * np.pi + (np.abs(x / ell) @ np.abs(omega).T).max(), 1).F
    err = np.abs(host(F) - ref)
    print(f"max |c| {np.abs(cc).max():.3e}, max err {err.max():.3e}, max err / bar {np.max(err / bar):.3f}")
    assert (err <= bar).all()


def test_errors_leave_the_context_usable(A, ctx):
    from agpl_amd import _ffi

    c = R.Case("se", 64, 100, 1, 20, 1, 1e-6, False, True)
    plan = make_plan(A, ctx, c)
    x, _, _ = R.case_inputs(c)
    omega, phase, V, W, Xi, _ = R.case_draws(c)
    V, omega, phase, W, Xi, xd = (dev(a) for a in (V, omega, phase, W, Xi, x))
    good = raw_paths(plan, V, omega, phase, W, Xi, xd)
    lib = _ffi.pathwise_lib()
    ptr = lambda t: C.c_void_p(0 if t is None else t.data_ptr())
    out = torch.full((c.T, 1, R.N), -7.0, dtype=torch.float32, device="cuda")

    def rc(h=plan._h, T=c.T, Vv=V, Fn=c.F, om=omega, ph=phase, Ww=W, Ns=R.N, xx=xd, oo=out):
        return lib.agpl_plan_sample_paths(h, C.c_int32(T), ptr(Vv), C.c_int32(Fn), ptr(om), ptr(ph), ptr(Ww), ptr(Xi), C.c_int64(Ns), ptr(xx),
                                          None, ptr(oo))

    # a plan from materialised features has no generator
    rng = np.random.default_rng(2)
    flat = A.Plan(dev((rng.standard_normal((R.N, c.M)) / 8).astype(np.float32)), torch.ones(R.N, device="cuda"), 1, ctx)
    assert rc(h=flat._h) == _ffi.ERR_INVALID_ARGUMENT
    with pytest.raises(A.ArgumentError):
        flat.sample_paths(4)
    assert rc(h=None) == _ffi.ERR_INVALID_ARGUMENT
    for kw in (dict(T=0), dict(Fn=0), dict(Fn=8193), dict(Ns=-1), dict(Vv=None), dict(om=None), dict(ph=None), dict(Ww=None), dict(xx=None),
               dict(oo=None)):
        assert rc(**kw) == _ffi.ERR_INVALID_ARGUMENT, kw
    assert rc(Ns=0) == _ffi.AGPL_OK
    assert torch.equal(out, torch.full_like(out, -7.0))
    # non-finite draws and features are named; nothing is written
    for name, t, where, word in (("V", V, (13, 0, 7), "13"), ("W", W, (11, 0, 99), "11"), ("Xi", Xi, (17, 0, 3), "17"),
                                 ("omega", omega, (42, 0), "42"), ("phase", phase, (77,), "77")):
        bad = t.clone()
        bad[where] = float("nan") if name != "W" else float("inf")
        args = dict(V=V, omega=omega, phase=phase, W=W, Xi=Xi)
        args[name] = bad
        with pytest.raises(A.DomainError, match=word):
            raw_paths(plan, args["V"], args["omega"], args["phase"], args["W"], args["Xi"], xd)
    Vb = V.clone()
    Vb[3, 0, 1] = float("inf")
    assert rc(Vv=Vb) == _ffi.ERR_DOMAIN
    ctx.synchronize()
    assert torch.equal(out, torch.full_like(out, -7.0))
    # a non-finite input spoils its own point only
    xb = xd.clone()
    xb[5, 0] = float("nan")
    xb[200, 0] = float("inf")
    F = raw_paths(plan, V, omega, phase, W, Xi, xb)
    ok = torch.ones(R.N, dtype=torch.bool, device="cuda")
    ok[5] = ok[200] = False
    assert torch.isnan(F[:, :, ~ok]).all() and torch.equal(F[:, :, ok], good[:, :, ok])
    # and the context still works
    assert torch.equal(raw_paths(plan, V, omega, phase, W, Xi, xd), good)
