"""agpl_plan_hyper_grad (include/agpl_hyper.h; Plan.hyper_grad, SparseCAVI.hyper_grad) on the GPU against the float64 autograd
reference of tests/hyper_reference.py evaluated at the plan's own m, S, beta, gamma after three real sweeps.

Shapes: N = 1000 (a ragged last tile) and 65536 + 300 (two chunks); M = 40 (padded to 256), 256 (exact), 300 (padded to 512: C has
three live row blocks, the last ragged); D = 1, 3, 16 (the three compile-time bounds of the contraction); L = 1 (Bernoulli) and 2
(heteroscedastic Gaussian); all five kinds; mu0 absent and nonzero; jitter 1e-6; three seeds of the data.
Errors are |device - reference| / scale, scale = the reference's sum of |terms| (hyper_reference.HYPER_BAR_FULL / _POINTS / _KZZ
hold the bars and the measured values)."""
import numpy as np
import pytest

import hyper_reference as HR
import kernels_reference as K

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

JITTER = 1e-6
# (kind, N, M, D, L, mu0)
CASES = [(K.SE, 1000, 40, 1, 1, False), (K.MATERN12, 1000, 256, 3, 2, True), (K.MATERN32, 1000, 300, 16, 1, True),
         (K.MATERN52, 65536 + 300, 40, 1, 2, False), (K.RQ, 1000, 300, 3, 1, False), (K.SE, 65536 + 300, 40, 3, 1, True)]
IDS = ["se-N1000-M40-D1-L1", "matern12-N1000-M256-D3-L2-mu0", "matern32-N1000-M300-D16-L1-mu0", "matern52-N65836-M40-D1-L2",
       "rq-N1000-M300-D3-L1", "se-N65836-M40-D3-L1-mu0"]
SEEDS = [3, 4, 5]


@pytest.fixture(scope="module")
def A():
    import agpl_amd

    return agpl_amd


def host(t):
    return t.detach().cpu().numpy()


def dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    return t if dtype is None else t.to(dtype)


@pytest.fixture(scope="module")
def ctx(A):
    return A.Context(0, seed=17)


def problem(A, case, seed):
    """Host data of a case: (lik, y, inputs of the reference)."""
    kind, N, M, D, L, with_mu0 = case
    x, z, ell = K.workload(N, M, D, seed=seed)
    rng = np.random.default_rng(seed + 40)
    f = np.sin(x[:, 0])
    if L == 1:
        lik, y = A.BernoulliLikelihood(), (rng.uniform(size=N) < 1 / (1 + np.exp(-2 * f))).astype(np.uint8)
    else:
        lik, y = A.HeteroscedasticGaussianLikelihood(2.0), (f + 0.3 * rng.standard_normal(N)).astype(np.float32)
    mu0 = (0.3 * np.cos(x[:, 0])[None, :] * np.arange(1, L + 1)[:, None]).astype(np.float32) if with_mu0 else None
    s2 = 1.0 if D == 1 else 2.5
    return lik, y, dict(kind=kind, param=K.param_of(kind), x=x, z=z, ell=ell, s2=s2, jitter=JITTER, mu0=mu0)


def build(A, ctx, lik, y, inp, i0=0, i1=None, group=None):
    """SparseCAVI.from_inputs on points i0 .. i1 - 1 of a problem."""
    mu0 = None if inp["mu0"] is None else dev(inp["mu0"][:, i0:i1])
    return A.SparseCAVI.from_inputs(lik, dev(inp["x"][i0:i1]), dev(y[i0:i1]), dev(inp["z"]), inp["ell"], variance=inp["s2"],
                                    jitter=JITTER, mu0=mu0, ctx=ctx, group=group, keep_points=True, keep_inputs=True,
                                    kernel=K.python_kernel(inp["kind"]))


def fitted(A, ctx, case, seed):
    """The SparseCAVI of a case after three sweeps and one more pass (beta, gamma, G, g of the CURRENT q(v)), and its inputs."""
    lik, y, inp = problem(A, case, seed)
    cavi = build(A, ctx, lik, y, inp)
    cavi.run(3)
    cavi.accumulate()
    cavi.check()
    return cavi, inp


def reference(cavi, inp, mu0="own"):
    return HR.gradient(m=host(cavi.m), S=host(cavi.S), beta=host(cavi.beta).astype(np.float64),
                       gamma=host(cavi.gamma).astype(np.float64), **{**inp, "mu0": inp["mu0"] if mu0 == "own" else mu0})


@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_gradient_against_the_float64_reference(A, ctx, case, seed):
    cavi, inp = fitted(A, ctx, case, seed)
    plan, xd = cavi.plan, cavi.x
    full = host(plan.hyper_grad(xd, cavi.beta, cavi.gamma, cavi.mu0, cavi.G, cavi.g))
    pts = host(plan.hyper_grad(xd, cavi.beta, cavi.gamma, cavi.mu0))
    ref = reference(cavi, inp)
    e_full = np.abs(full - ref["grad"]) / ref["scale"]
    if inp["mu0"] is None:  # G = NULL: the points' part alone; the difference of the two calls: the K_ZZ part
        e_pts = np.abs(pts - ref["points"]) / ref["scale_points"]
        e_kzz = np.abs(full - pts - ref["kzz"]) / ref["scale_kzz"]
    else:  # with a prior mean the G = NULL call carries the -m h' term of the K_ZZ part: K_ZZ part(mu0) - K_ZZ part(no mu0)
        ref0 = reference(cavi, inp, mu0=None)
        e_pts = np.abs(pts - (ref["points"] + ref["kzz"] - ref0["kzz"])) / ref["scale"]
        e_kzz = np.abs(full - pts - ref0["kzz"]) / ref0["scale_kzz"]
    print(f"HYPER_ERR case={IDS[CASES.index(case)]} seed={seed} full={e_full.max():.3e} points={e_pts.max():.3e} kzz={e_kzz.max():.3e} "
          f"grad={np.array2string(ref['grad'], precision=4)} scale={np.array2string(ref['scale'], precision=4)}")
    assert np.isfinite(full).all() and np.isfinite(pts).all()
    assert e_full.max() <= HR.HYPER_BAR_FULL and e_pts.max() <= HR.HYPER_BAR_POINTS and e_kzz.max() <= HR.HYPER_BAR_KZZ


def test_two_calls_give_the_same_bits_and_a_copy_of_x_changes_nothing(A, ctx):
    cavi, _ = fitted(A, ctx, CASES[5], 3)
    call = lambda xx: cavi.plan.hyper_grad(xx, cavi.beta, cavi.gamma, cavi.mu0, cavi.G, cavi.g)
    a, b, c = call(cavi.x), call(cavi.x), call(cavi.x.clone())
    assert torch.equal(a, b) and torch.equal(a, c)
    assert torch.equal(cavi.plan.features(0, 300), cavi.plan.features(0, 300))  # (the plan still serves)


def test_one_process_equals_the_sum_of_two_half_shards(A, ctx):
    """Plans of the two halves of the points carrying the whole run's q(v); the K_ZZ part (the exchanged G, g) on the first."""
    case = CASES[5]
    cavi, inp = fitted(A, ctx, case, 4)
    whole = host(cavi.plan.hyper_grad(cavi.x, cavi.beta, cavi.gamma, cavi.mu0, cavi.G, cavi.g))
    st, N, h = cavi.plan.state(), cavi.N, cavi.N // 2 + 37
    total = np.zeros_like(whole)
    for k, (i0, i1) in enumerate([(0, h), (h, N)]):
        p = A.Plan.from_inputs(cavi.x[i0:i1], dev(inp["z"]), inp["ell"], variance=inp["s2"], jitter=JITTER, L=cavi.L, ctx=ctx,
                               kernel=K.python_kernel(case[0]))
        p.load_state(st)
        sl = lambda t: t[:, i0:i1].contiguous()
        total += host(p.hyper_grad(cavi.x[i0:i1], sl(cavi.beta), sl(cavi.gamma), sl(cavi.mu0), cavi.G if k == 0 else None,
                                   cavi.g if k == 0 else None))
    scale = reference(cavi, inp)["scale"]
    print("HYPER_SHARD", np.abs(total - whole) / scale)
    assert np.all(np.abs(total - whole) <= 1e-10 * scale)


def test_sparse_cavi_hyper_grad_is_the_plan_call(A, ctx):
    cavi, _ = fitted(A, ctx, CASES[0], 3)
    want = host(cavi.plan.hyper_grad(cavi.x, cavi.beta, cavi.gamma, cavi.mu0, cavi.G, cavi.g))
    G0, g0, b0, c0 = cavi.G.clone(), cavi.g.clone(), cavi.beta.clone(), cavi.gamma.clone()
    got = cavi.hyper_grad()
    assert torch.equal(cavi.G, G0) and torch.equal(cavi.g, g0)  # (the sweep's state is untouched)
    assert torch.equal(cavi.beta, b0) and torch.equal(cavi.gamma, c0)
    np.testing.assert_array_equal(np.concatenate([got["log_lengthscale"].numpy(), [got["log_variance"]]]), want)


def test_errors_leave_the_context_usable(A, ctx):
    cavi, inp = fitted(A, ctx, CASES[0], 3)
    good = lambda: cavi.plan.hyper_grad(cavi.x, cavi.beta, cavi.gamma, None, cavi.G, cavi.g)
    want = good()
    Phi = cavi.plan.features()
    resid = cavi.plan.resid.clone()
    feat = A.Plan(Phi, resid, 1, ctx)  # a plan made from features
    with pytest.raises(A.ArgumentError):
        feat.hyper_grad(cavi.x, cavi.beta, cavi.gamma)
    with pytest.raises(A.ArgumentError):
        A._ffi.check(ctx._h, A._ffi.hyper_lib().agpl_plan_hyper_grad(feat._h, cavi.N, cavi.x.data_ptr(), None, cavi.beta.data_ptr(),
                                                                      cavi.gamma.data_ptr(), None, None, want.data_ptr()))
    assert torch.equal(good(), want)
    with pytest.raises(A.ArgumentError):  # N different from the plan's
        cavi.plan.hyper_grad(cavi.x[:500], cavi.beta[:, :500].contiguous(), cavi.gamma[:, :500].contiguous())
    bad = cavi.x.clone()
    bad[321, 0] = float("nan")
    with pytest.raises(A.DomainError):
        cavi.plan.hyper_grad(bad, cavi.beta, cavi.gamma, None, cavi.G, cavi.g)
    assert torch.equal(good(), want)
    gib = A.Plan.from_inputs(cavi.x, dev(inp["z"]), inp["ell"], jitter=JITTER, ctx=ctx, flags=A.Plan.NO_MARGINALS)
    with pytest.raises(A.ArgumentError):
        gib.hyper_grad(cavi.x, cavi.beta, cavi.gamma)
    assert torch.equal(good(), want)
