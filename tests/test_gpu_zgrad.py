"""agpl_plan_inducing_grad (include/agpl_zgrad.h; Plan.inducing_grad, SparseCAVI.hyper_grad(inducing=True)) on the GPU against the
float64 autograd reference of tests/zgrad_reference.py evaluated at the plan's own m, S, beta, gamma after three real sweeps.

The problems, shapes and seeds are those of tests/test_gpu_hyper_grad.py (N = 1000: a ragged last tile; 65536 + 300: two chunks;
M = 40 padded to 256, 256 exact, 300: three live row blocks, the last ragged; D = 1, 3, 16: the three compile-time bounds; L = 1 and
2; all five kinds; mu0 absent and nonzero); in the Matern-1/2 case z[0] = x[17] exactly (r = 0).  Errors are
|device - reference| / scale per component, worst over (a, d), scale = the reference's sum of |terms|
(zgrad_reference.ZGRAD_BAR_FULL / _POINTS / _KZZ hold the bars and the measured values).  The whole gradient is taken at the sweep's
own G, g; the K_ZZ bar is on the float64 K_ZZ sequence itself, so its two calls take G, g formed in float64 from the reference's
features at the plan's gamma, beta (the same difference at the sweep's G, g, which carry the accumulation's 2^-22, is printed)."""
import numpy as np
import pytest

import kernels_reference as K
import test_gpu_hyper_grad as T
import zgrad_reference as ZR

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

CASES, IDS, SEEDS, JITTER = T.CASES, T.IDS, T.SEEDS, T.JITTER
host, dev = T.host, T.dev


@pytest.fixture(scope="module")
def A():
    import agpl_amd

    return agpl_amd


@pytest.fixture(scope="module")
def ctx(A):
    return A.Context(0, seed=17)


_FITTED = {}


def fitted(A, ctx, case, seed):
    """T.fitted (three sweeps and one more pass) of a case, once per (case, seed); Matern-1/2: an inducing input on a point."""
    key = (CASES.index(case), seed)
    if key not in _FITTED:
        lik, y, inp = T.problem(A, case, seed)
        if case[0] == K.MATERN12:
            inp["z"] = inp["z"].copy()
            inp["z"][0] = inp["x"][17]
        cavi = T.build(A, ctx, lik, y, inp)
        cavi.run(3)
        cavi.accumulate()
        cavi.check()
        _FITTED[key] = (cavi, inp)
    return _FITTED[key]


def reference(cavi, inp, mu0="own"):
    return ZR.gradient_z(m=host(cavi.m), S=host(cavi.S), beta=host(cavi.beta).astype(np.float64),
                         gamma=host(cavi.gamma).astype(np.float64), **{**inp, "mu0": inp["mu0"] if mu0 == "own" else mu0})


def float64_naturals(cavi, inp):
    """G_l = Phi Diag(gamma_l) Phi', g_l = Phi beta_l in float64 from the reference's own features (tests/kernels_reference.py) at the
    plan's gamma, beta: what the sweep exchanges, without the 2^-22 of its split-float16 accumulation."""
    Phi, _, _ = K.phi_f64(inp["kind"], inp["x"], inp["z"], inp["ell"], inp["s2"], inp["jitter"], inp["param"])  # [N, M]
    gamma, beta = host(cavi.gamma).astype(np.float64), host(cavi.beta).astype(np.float64)
    G = np.stack([(Phi * gamma[l][:, None]).T @ Phi for l in range(cavi.L)])
    g = np.stack([Phi.T @ beta[l] for l in range(cavi.L)])
    return dev(G), dev(g)


def full_call(cavi, x=None, **kw):
    return cavi.plan.inducing_grad(cavi.x if x is None else x, cavi.beta, cavi.gamma, cavi.mu0, cavi.G, cavi.g, **kw)


@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_gradient_against_the_float64_reference(A, ctx, case, seed):
    cavi, inp = fitted(A, ctx, case, seed)
    full = host(full_call(cavi))
    pts = host(cavi.plan.inducing_grad(cavi.x, cavi.beta, cavi.gamma, cavi.mu0))
    G64, g64 = float64_naturals(cavi, inp)
    full64 = host(cavi.plan.inducing_grad(cavi.x, cavi.beta, cavi.gamma, cavi.mu0, G64, g64))
    ref = reference(cavi, inp)
    assert full.shape == pts.shape == ref["grad"].shape == inp["z"].shape
    e_full = np.abs(full - ref["grad"]) / ref["scale"]
    if inp["mu0"] is None:  # G = NULL: the points' part alone; the difference of the two calls: the K_ZZ part
        e_pts = np.abs(pts - ref["points"]) / ref["scale_points"]
        e_kzz, e_kzz_sweep = np.abs(full64 - pts - ref["kzz"]) / ref["scale_kzz"], np.abs(full - pts - ref["kzz"]) / ref["scale_kzz"]
    else:  # with a prior mean the G = NULL call carries the -m h' term of the K_ZZ part: K_ZZ part(mu0) - K_ZZ part(no mu0)
        ref0 = reference(cavi, inp, mu0=None)
        e_pts = np.abs(pts - (ref["points"] + ref["kzz"] - ref0["kzz"])) / ref["scale"]
        e_kzz, e_kzz_sweep = np.abs(full64 - pts - ref0["kzz"]) / ref0["scale_kzz"], np.abs(full - pts - ref0["kzz"]) / ref0["scale_kzz"]
    e_full64 = np.abs(full64 - ref["grad"]) / ref["scale"]
    print(f"ZGRAD_ERR case={IDS[CASES.index(case)]} seed={seed} full={e_full.max():.3e} points={e_pts.max():.3e} kzz={e_kzz.max():.3e} "
          f"kzz_at_sweep_Gg={e_kzz_sweep.max():.3e} full_at_f64_Gg={e_full64.max():.3e} "
          f"max|grad|={np.abs(ref['grad']).max():.4g} max scale={ref['scale'].max():.4g} min scale={ref['scale'].min():.4g}")
    assert np.isfinite(full).all() and np.isfinite(pts).all()
    assert e_full.max() <= ZR.ZGRAD_BAR_FULL and e_pts.max() <= ZR.ZGRAD_BAR_POINTS and e_kzz.max() <= ZR.ZGRAD_BAR_KZZ


@pytest.mark.parametrize("case", [CASES[1], CASES[2], CASES[5]], ids=[IDS[1], IDS[2], IDS[5]])
def test_with_theta_is_hyper_grad_to_the_bit(A, ctx, case):
    cavi, _ = fitted(A, ctx, case, 3)
    for G, g in ((cavi.G, cavi.g), (None, None)):
        want = cavi.plan.hyper_grad(cavi.x, cavi.beta, cavi.gamma, cavi.mu0, G, g)
        theta, gz = cavi.plan.inducing_grad(cavi.x, cavi.beta, cavi.gamma, cavi.mu0, G, g, with_theta=True)
        assert torch.equal(theta, want)
        assert torch.equal(gz, cavi.plan.inducing_grad(cavi.x, cavi.beta, cavi.gamma, cavi.mu0, G, g))


def test_two_calls_give_the_same_bits_and_a_copy_of_x_changes_nothing(A, ctx):
    cavi, _ = fitted(A, ctx, CASES[5], 3)
    a, b, c = full_call(cavi), full_call(cavi), full_call(cavi, cavi.x.clone())
    assert torch.equal(a, b) and torch.equal(a, c)
    assert torch.equal(cavi.plan.features(0, 300), cavi.plan.features(0, 300))  # (the plan still serves)


def test_one_process_equals_the_sum_of_two_half_shards(A, ctx):
    """Plans of the two halves of the points carrying the whole run's q(v); the K_ZZ part (the exchanged G, g) on the first."""
    case = CASES[5]
    cavi, inp = fitted(A, ctx, case, 4)
    whole = host(full_call(cavi))
    st, N, h = cavi.plan.state(), cavi.N, cavi.N // 2 + 37
    total = np.zeros_like(whole)
    for k, (i0, i1) in enumerate([(0, h), (h, N)]):
        p = A.Plan.from_inputs(cavi.x[i0:i1], dev(inp["z"]), inp["ell"], variance=inp["s2"], jitter=JITTER, L=cavi.L, ctx=ctx,
                               kernel=K.python_kernel(case[0]))
        p.load_state(st)
        sl = lambda t: t[:, i0:i1].contiguous()
        total += host(p.inducing_grad(cavi.x[i0:i1], sl(cavi.beta), sl(cavi.gamma), sl(cavi.mu0), cavi.G if k == 0 else None,
                                      cavi.g if k == 0 else None))
    scale = reference(cavi, inp)["scale"]
    print("ZGRAD_SHARD", (np.abs(total - whole) / scale).max())
    assert np.all(np.abs(total - whole) <= 1e-10 * scale)


def test_sparse_cavi_hyper_grad_with_inducing_is_the_plan_call(A, ctx):
    cavi, _ = fitted(A, ctx, CASES[0], 3)
    theta, gz = full_call(cavi, with_theta=True)
    plain = cavi.hyper_grad()
    G0, g0, b0, c0 = cavi.G.clone(), cavi.g.clone(), cavi.beta.clone(), cavi.gamma.clone()
    got = cavi.hyper_grad(inducing=True)
    assert torch.equal(cavi.G, G0) and torch.equal(cavi.g, g0)  # (the sweep's state is untouched)
    assert torch.equal(cavi.beta, b0) and torch.equal(cavi.gamma, c0)
    np.testing.assert_array_equal(np.concatenate([got["log_lengthscale"].numpy(), [got["log_variance"]]]), host(theta))
    np.testing.assert_array_equal(got["z"].numpy(), host(gz))
    assert got["z"].dtype == torch.float64 and tuple(got["z"].shape) == (cavi.M, cavi.plan.D)
    again = cavi.hyper_grad()  # without the flag: unchanged, and no "z"
    assert sorted(again) == ["log_lengthscale", "log_variance"] == sorted(plain)
    assert torch.equal(again["log_lengthscale"], plain["log_lengthscale"]) and again["log_variance"] == plain["log_variance"]
    assert torch.equal(again["log_lengthscale"], got["log_lengthscale"]) and again["log_variance"] == got["log_variance"]


def test_errors_leave_the_context_usable(A, ctx):
    cavi, inp = fitted(A, ctx, CASES[0], 3)
    good = lambda: cavi.plan.inducing_grad(cavi.x, cavi.beta, cavi.gamma, None, cavi.G, cavi.g)
    want = good()
    Phi = cavi.plan.features()
    resid = cavi.plan.resid.clone()
    feat = A.Plan(Phi, resid, 1, ctx)  # a plan made from features
    with pytest.raises(A.ArgumentError):
        feat.inducing_grad(cavi.x, cavi.beta, cavi.gamma)
    raw = lambda plan, *a: A._ffi.check(ctx._h, A._ffi.zgrad_lib().agpl_plan_inducing_grad(plan._h, *a))
    with pytest.raises(A.ArgumentError):
        raw(feat, cavi.N, cavi.x.data_ptr(), None, cavi.beta.data_ptr(), cavi.gamma.data_ptr(), None, None, None, want.data_ptr())
    assert torch.equal(good(), want)
    with pytest.raises(A.ArgumentError):  # a null output
        raw(cavi.plan, cavi.N, cavi.x.data_ptr(), None, cavi.beta.data_ptr(), cavi.gamma.data_ptr(), None, None, None, None)
    with pytest.raises(A.ArgumentError):  # exactly one of G, g
        raw(cavi.plan, cavi.N, cavi.x.data_ptr(), None, cavi.beta.data_ptr(), cavi.gamma.data_ptr(), cavi.G.data_ptr(), None, None,
            want.clone().data_ptr())
    assert torch.equal(good(), want)
    with pytest.raises(A.ArgumentError):  # N different from the plan's
        cavi.plan.inducing_grad(cavi.x[:500], cavi.beta[:, :500].contiguous(), cavi.gamma[:, :500].contiguous())
    bad = cavi.x.clone()
    bad[321, 0] = float("nan")
    with pytest.raises(A.DomainError, match="point 321 "):  # (with the index)
        cavi.plan.inducing_grad(bad, cavi.beta, cavi.gamma, None, cavi.G, cavi.g)
    assert torch.equal(good(), want)
    gib = A.Plan.from_inputs(cavi.x, dev(inp["z"]), inp["ell"], jitter=JITTER, ctx=ctx, flags=A.Plan.NO_MARGINALS)
    with pytest.raises(A.ArgumentError):
        gib.inducing_grad(cavi.x, cavi.beta, cavi.gamma)
    assert torch.equal(good(), want)
