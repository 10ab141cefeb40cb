"""The chunk, sub-chunk and group seams of the "new inputs" entry points, each crossed at the smallest shape that reaches it
(tests/seam_shapes.py holds the shapes; tests/test_seam_shapes_cpu.py holds them against the constants in the sources):

1. agpl_plan_predict over its 65536-point chunk, L = 1 (direct) and L = 3 (mu0, mu, var staged through pitched copies);
2. agpl_plan_sample_paths over the chunk, and over a sub-chunk seam inside the SECOND chunk (F = 8192); the all-zero operands;
3. agpl_plan_inducing_grad over the tile-group seam (M D = 4800: chunk one runs as groups of 436 and 76 tiles) and the chunk seam;
4. agpl_plan_hyper_grad with L = 2, a prior mean and two chunks (hy_h_kernel's mu0 at c0 > 0, pitch N);
5. agpl_predictive beyond its cap of 1024 workgroups: the stride loops of both kernels and the 1024-partial second level.

A wrong offset or pitch in these loops gives plausible numbers, not a crash.  The checks are bit equality with calls that stay inside
one chunk / one launch (which the sibling modules judge against float64), the bars tests/zgrad_reference.py and
tests/hyper_reference.py already hold, the sharding identities at their siblings' 1e-10 of scale, and for the device sum the bound
that holds for ANY order of n float64 additions."""
import ctypes as C
import math

import numpy as np
import pytest

import hyper_reference as HR
import kernels_reference as K
import pathwise_reference as PR
import seam_shapes as S
import test_gpu_hyper_grad as TH
import test_gpu_pathwise as TP
import test_gpu_predictive as TY
import zgrad_reference as ZR

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

host, dev, JITTER = TH.host, TH.dev, TH.JITTER


@pytest.fixture(scope="module")
def A():
    import agpl_amd

    return agpl_amd


@pytest.fixture(scope="module")
def ctx(A):
    return A.Context(0, seed=17)


def same(a, b):
    """Bit equality of two tuples of tensors."""
    return all(torch.equal(s, t) for s, t in zip(a, b))


# ---- 1. agpl_plan_predict ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("L,with_mu0", [(1, True), (3, True), (3, False)], ids=["L1-mu0", "L3-mu0", "L3"])
def test_predict_across_the_chunk_seam(A, ctx, L, with_mu0):
    """The full call against calls that stay inside one chunk: a window across the seam, the head, a gather.  One-chunk predict is
    judged against float64 in tests/test_gpu_kernels.py; bit equality carries that over the seam."""
    assert L in S.PREDICT_LS
    M, D, Ns = S.PREDICT_M, S.PREDICT_D, S.PREDICT_NS
    x, z, ell = K.workload(300, M, D, seed=3)
    plan = A.Plan.from_inputs(dev(x), dev(z), ell, variance=2.5, jitter=JITTER, L=L, ctx=ctx)
    rng = np.random.default_rng([L, 11])
    B = rng.standard_normal((L, M, M // 2))
    Gd = dev(np.einsum("lak,lbk->lab", B, B) * (0.5 + np.arange(L))[:, None, None])  # positive semi-definite, another per latent
    gd = dev(rng.standard_normal((L, M)))
    plan.call("agpl_plan_update", C.c_void_p(Gd.data_ptr()), C.c_void_p(gd.data_ptr()), C.c_void_p(0), C.c_void_p(0))
    ctx.synchronize()
    xs = dev(rng.uniform(-10, 10, size=(Ns, D)))
    mu0 = dev((3.0 * (1.0 + np.arange(L))[:, None] + 0.5 * rng.standard_normal((L, Ns))).astype(np.float32)) if with_mu0 else None
    cut = lambda i: (xs[i].contiguous(), None if mu0 is None else mu0[:, i].contiguous())
    full = plan.predict(xs, mu0)
    assert all(tuple(t.shape) == (L, Ns) and bool(torch.isfinite(t).all()) for t in full)
    assert same(plan.predict(xs, mu0), full)
    w = slice(S.PREDICT_WINDOW, Ns)
    assert same(plan.predict(*cut(w)), [t[:, w] for t in full])
    h = slice(0, S.PREDICT_HEAD)
    assert same(plan.predict(*cut(h)), [t[:, h] for t in full])
    idx = torch.tensor(S.PREDICT_GATHER, device="cuda")
    assert same(plan.predict(*cut(idx)), [t[:, idx] for t in full])


# ---- 2. agpl_plan_sample_paths -------------------------------------------------------------------------------------------------------

def _paths_case(F):
    return PR.Case("se", 5, F, 3, 2, 3, 1e-6, True, True)


@pytest.mark.parametrize("shape", [S.PATHS_SMALL, S.PATHS_LARGE], ids=["F100-chunk", "F8192-chunk-and-sub-chunk"])
def test_sample_paths_across_the_chunk_seam(A, ctx, shape):
    F, Ns, gather = shape
    c = _paths_case(F)
    plan = TP.make_plan(A, ctx, c)
    rng = np.random.default_rng([F, 9])
    xs = dev(rng.uniform(-3, 3, size=(Ns, c.D)))
    mu0 = dev((0.5 * rng.standard_normal((c.L, Ns))).astype(np.float32))
    omega, phase = PR.spectral(c.kind, c.F, c.D, rng)
    d = [dev(a) for a in (rng.standard_normal((c.T, c.L, c.M)), omega, phase, rng.standard_normal((c.T, c.L, c.F)),
                          rng.standard_normal((c.T, c.L, c.M)))]
    full = TP.raw_paths(plan, *d, xs, mu0)
    assert tuple(full.shape) == (c.T, c.L, Ns) and bool(torch.isfinite(full).all())
    assert torch.equal(TP.raw_paths(plan, *d, xs, mu0), full)
    idx = torch.tensor(gather, device="cuda")
    sub = TP.raw_paths(plan, *d, xs[idx].contiguous(), mu0[:, idx].contiguous())
    assert torch.equal(sub, full[:, :, idx])
    w = slice(S.PATHS_WINDOW, Ns)
    assert torch.equal(TP.raw_paths(plan, *d, xs[w].contiguous(), mu0[:, w].contiguous()), full[:, :, w])
    bare = TP.make_plan(A, ctx, c, A.Plan.NO_MARGINALS)
    assert torch.equal(TP.raw_paths(bare, *d, xs[idx].contiguous(), mu0[:, idx].contiguous()), sub)


def test_sample_paths_of_all_zero_operands(A, ctx):
    """V = 0, W = 0, Xi = NULL: c = 0 and s W = 0, the one input on which both operands have no scale bound; every product is a
    product with zero, so the draw is mu0 exactly (0 without one)."""
    c = _paths_case(100)
    plan = TP.make_plan(A, ctx, c)
    rng = np.random.default_rng(5)
    Ns = S.PATHS_ZERO_NS
    xs = dev(rng.uniform(-3, 3, size=(Ns, c.D)))
    mu0 = dev((3.0 + 0.5 * rng.standard_normal((c.L, Ns))).astype(np.float32))
    omega, phase = PR.spectral(c.kind, c.F, c.D, rng)
    V, W = dev(np.zeros((c.T, c.L, c.M))), dev(np.zeros((c.T, c.L, c.F)))
    got = TP.raw_paths(plan, V, dev(omega), dev(phase), W, None, xs, mu0)
    assert torch.equal(got, mu0[None].expand(c.T, c.L, Ns))
    got = TP.raw_paths(plan, V, dev(omega), dev(phase), W, None, xs, None)
    assert torch.equal(got, torch.zeros_like(got))


# ---- 3. agpl_plan_inducing_grad ------------------------------------------------------------------------------------------------------

ZCASE = (K.MATERN32, S.ZGRAD_N, S.ZGRAD_M, S.ZGRAD_D, 1, False)
ZID = "matern32-N65836-M300-D16-L1"


@pytest.fixture(scope="module")
def zworld(A, ctx):
    """The fitted SparseCAVI of ZCASE (three sweeps and one more pass) and the float64 points' part, computed once: the chunked
    reference of the first group's points [0, ZGRAD_CUT), of the rest, and their sum (the whole: the part is a sum over points)."""
    cavi, inp = TH.fitted(A, ctx, ZCASE, 3)
    q = dict(m=host(cavi.m), S=host(cavi.S))
    beta, gamma = host(cavi.beta).astype(np.float64), host(cavi.gamma).astype(np.float64)
    parts = []
    for i0, i1 in ((0, S.ZGRAD_CUT), (S.ZGRAD_CUT, S.ZGRAD_N)):
        parts.append(ZR.points_part_chunked(**{**inp, "x": inp["x"][i0:i1]}, **q, beta=beta[:, i0:i1], gamma=gamma[:, i0:i1], chunk=4096))
    ref = {k: parts[0][k] + parts[1][k] for k in ("points", "scale_points")}
    # the K_ZZ half's scale from the first 1000 points: that half is a sum over the points too, so 1000 of them UNDERSTATE its scale
    # at N = 65836 -- the shard identity below is judged on a smaller scale than its sibling's, never a larger one
    small = ZR.gradient_z(**{**inp, "x": inp["x"][:1000]}, **q, beta=beta[:, :1000], gamma=gamma[:, :1000])
    return cavi, inp, ref, parts[0], small["scale_kzz"]


def _shard(A, ctx, cavi, inp, case, i0, i1):
    """A plan of points i0 .. i1 - 1 carrying the whole run's q(v), and those points' x, beta, gamma, mu0."""
    p = A.Plan.from_inputs(cavi.x[i0:i1], dev(inp["z"]), inp["ell"], variance=inp["s2"], jitter=JITTER, L=cavi.L, ctx=ctx,
                           kernel=K.python_kernel(case[0]))
    p.load_state(cavi.plan.state())
    sl = lambda t: None if t is None else t[:, i0:i1].contiguous()
    return p, cavi.x[i0:i1], sl(cavi.beta), sl(cavi.gamma), sl(cavi.mu0)


def test_inducing_grad_points_part_against_float64_across_the_group_seam(A, ctx, zworld):
    """Judged on zgrad_reference.ZGRAD_BAR_POINTS as it stands.  points: the whole call; first_group: a plan of the first 436 tiles
    alone, which runs as one launch -- an error that grew from tile 436 on would separate the two.  Measured on an MI355X:
    points 1.271e-07, first_group 1.298e-07 of scale (bar 9.944e-06)."""
    cavi, inp, ref, ref_first, _ = zworld
    pts = host(cavi.plan.inducing_grad(cavi.x, cavi.beta, cavi.gamma, None))
    p, x, beta, gamma, _ = _shard(A, ctx, cavi, inp, ZCASE, 0, S.ZGRAD_CUT)
    first = host(p.inducing_grad(x, beta, gamma, None))
    e_pts = np.abs(pts - ref["points"]) / ref["scale_points"]
    e_first = np.abs(first - ref_first["points"]) / ref_first["scale_points"]
    print(f"ZGRAD_ERR case={ZID} seed=3 points={e_pts.max():.3e} first_group={e_first.max():.3e} bar={ZR.ZGRAD_BAR_POINTS:.3e} "
          f"max err / bar {e_pts.max() / ZR.ZGRAD_BAR_POINTS:.3f} max|points|={np.abs(ref['points']).max():.4g} "
          f"max scale={ref['scale_points'].max():.4g} min scale={ref['scale_points'].min():.4g}")
    assert pts.shape == ref["points"].shape == inp["z"].shape and np.isfinite(pts).all()
    assert e_pts.max() <= ZR.ZGRAD_BAR_POINTS and e_first.max() <= ZR.ZGRAD_BAR_POINTS


def test_inducing_grad_theta_is_hyper_grad_to_the_bit_across_the_group_seam(A, ctx, zworld):
    """hyper_grad fills ``part`` in one launch per chunk, inducing_grad group by group: the D + 1 numbers must not know.  And two
    calls give the same bits."""
    cavi = zworld[0]
    for G, g in ((cavi.G, cavi.g), (None, None)):
        want = cavi.plan.hyper_grad(cavi.x, cavi.beta, cavi.gamma, None, G, g)
        theta, gz = cavi.plan.inducing_grad(cavi.x, cavi.beta, cavi.gamma, None, G, g, with_theta=True)
        assert bool(torch.isfinite(want).all()) and torch.equal(theta, want)
        again = cavi.plan.inducing_grad(cavi.x, cavi.beta, cavi.gamma, None, G, g)
        assert torch.equal(gz, again) and torch.equal(again, cavi.plan.inducing_grad(cavi.x, cavi.beta, cavi.gamma, None, G, g))


def test_inducing_grad_equals_the_sum_of_the_first_group_and_the_rest(A, ctx, zworld):
    """Shards cut at tile 436 of chunk one: the first is exactly the whole call's first launch; G, g on the first."""
    cavi, inp, ref, _, scale_kzz = zworld
    whole = host(cavi.plan.inducing_grad(cavi.x, cavi.beta, cavi.gamma, None, cavi.G, cavi.g))
    total = np.zeros_like(whole)
    for k, (i0, i1) in enumerate([(0, S.ZGRAD_CUT), (S.ZGRAD_CUT, S.ZGRAD_N)]):
        p, x, beta, gamma, _ = _shard(A, ctx, cavi, inp, ZCASE, i0, i1)
        total += host(p.inducing_grad(x, beta, gamma, None, cavi.G if k == 0 else None, cavi.g if k == 0 else None))
    scale = ref["scale_points"] + scale_kzz
    err = np.abs(total - whole) / scale
    print(f"ZGRAD_SHARD case={ZID} max err {err.max():.3e} bar 1e-10, max err / bar {err.max() / 1e-10:.3f}")
    assert np.all(np.abs(total - whole) <= 1e-10 * scale)


# ---- 4. agpl_plan_hyper_grad, L = 2, a prior mean, two chunks ------------------------------------------------------------------------

HCASE = (K.SE, S.HYPER_N, 40, 3, 2, True)
HID = "se-N65836-M40-D3-L2-mu0"


@pytest.fixture(scope="module")
def hworld(A, ctx):
    cavi, inp = TH.fitted(A, ctx, HCASE, 3)
    return cavi, inp, TH.reference(cavi, inp), TH.reference(cavi, inp, mu0=None)


def test_hyper_grad_two_latents_with_a_prior_mean_over_two_chunks(A, ctx, hworld):
    """The assertions of test_gpu_hyper_grad.py::test_gradient_against_the_float64_reference (its prior-mean branch), one seed.
    Measured on an MI355X: full 7.245e-09, points 2.180e-09, kzz 2.949e-07 of scale (0.009, 0.006, 0.021 of the bars)."""
    cavi, inp, ref, ref0 = hworld
    call = lambda *Gg: cavi.plan.hyper_grad(cavi.x, cavi.beta, cavi.gamma, cavi.mu0, *Gg)
    full, pts = host(call(cavi.G, cavi.g)), host(call())
    e_full = np.abs(full - ref["grad"]) / ref["scale"]
    e_pts = np.abs(pts - (ref["points"] + ref["kzz"] - ref0["kzz"])) / ref["scale"]
    e_kzz = np.abs(full - pts - ref0["kzz"]) / ref0["scale_kzz"]
    print(f"HYPER_ERR case={HID} seed=3 full={e_full.max():.3e} points={e_pts.max():.3e} kzz={e_kzz.max():.3e} "
          f"max err / bar {e_full.max() / HR.HYPER_BAR_FULL:.3f} {e_pts.max() / HR.HYPER_BAR_POINTS:.3f} {e_kzz.max() / HR.HYPER_BAR_KZZ:.3f} "
          f"grad={np.array2string(ref['grad'], precision=4)} scale={np.array2string(ref['scale'], precision=4)}")
    assert np.isfinite(full).all() and np.isfinite(pts).all()
    assert e_full.max() <= HR.HYPER_BAR_FULL and e_pts.max() <= HR.HYPER_BAR_POINTS and e_kzz.max() <= HR.HYPER_BAR_KZZ
    assert torch.equal(call(cavi.G, cavi.g), call(cavi.G, cavi.g)) and torch.equal(call(), call())
    assert np.array_equal(host(call(cavi.G, cavi.g)), full)


def test_hyper_grad_equals_the_sum_of_shards_cut_at_the_chunk(A, ctx, hworld):
    """The second shard reads the same prior mean at c0 = 0 with its own pitch (300), the whole call at c0 = 65536 with pitch N."""
    cavi, inp, ref, _ = hworld
    whole = host(cavi.plan.hyper_grad(cavi.x, cavi.beta, cavi.gamma, cavi.mu0, cavi.G, cavi.g))
    total = np.zeros_like(whole)
    for k, (i0, i1) in enumerate([(0, S.HYPER_CUT), (S.HYPER_CUT, S.HYPER_N)]):
        p, x, beta, gamma, mu0 = _shard(A, ctx, cavi, inp, HCASE, i0, i1)
        total += host(p.hyper_grad(x, beta, gamma, mu0, cavi.G if k == 0 else None, cavi.g if k == 0 else None))
    err = np.abs(total - whole) / ref["scale"]
    print(f"HYPER_SHARD case={HID} max err {err.max():.3e} bar 1e-10, max err / bar {err.max() / 1e-10:.3f}")
    assert np.all(np.abs(total - whole) <= 1e-10 * ref["scale"])


# ---- 5. agpl_predictive beyond 1024 workgroups ---------------------------------------------------------------------------------------

def _device_sum_checks(A, ctx, lik, mu, var, y, lp, **kw):
    """log_predictive_density against math.fsum of the same call's logp.  The bar n 2^-53 sum |logp| holds for every order in which n
    float64 terms can be added ((n - 1) roundings, each at most 2^-53 of a partial sum <= sum |logp|): no measured margin."""
    n = lp.numel()
    s1 = A.log_predictive_density(lik, (mu, var), y, ctx=ctx, **kw)
    s2 = A.log_predictive_density(lik, (mu, var), y, ctx=ctx, **kw)
    terms = lp.cpu().tolist()
    ref, bar = math.fsum(terms), n * 2.0 ** -53 * math.fsum(abs(t) for t in terms)
    print(f"device sum of {n} log densities: {s1!r}, fsum {ref!r}, |diff| {abs(s1 - ref):.3e}, bar {bar:.3e}, max err / bar "
          f"{abs(s1 - ref) / bar:.3f}")
    assert math.isfinite(ref) and np.float64(s1).tobytes() == np.float64(s2).tobytes()
    assert abs(s1 - ref) <= bar
    bad = var.clone()
    bad.view(n, -1)[n - 2, 0] = float("nan")  # in the strided part
    assert math.isnan(A.log_predictive_density(lik, (mu, bad), y, ctx=ctx, **kw))


@pytest.mark.parametrize("kind", ["bernoulli", "heterogauss"])
def test_predictive_scalar_beyond_the_launch_cap(A, ctx, kind):
    n = S.PRED_SCALAR_N
    rng = np.random.default_rng(21)
    shape = (n, 2) if kind == "heterogauss" else (n,)
    mu_h = rng.uniform(-4, 4, shape)
    mu, var = TY._dev(mu_h), TY._dev(np.exp(rng.uniform(np.log(0.05), np.log(2.0), shape)) ** 2)
    if kind == "bernoulli":
        lik, y = A.BernoulliLikelihood(), TY._dev(rng.integers(0, 2, n).astype(np.uint8))
    else:
        lik, y = A.HeteroscedasticGaussianLikelihood(2.0), TY._dev(mu_h[:, 0] + 0.7 * rng.standard_normal(n))
    long = A.predictive(lik, (mu, var), y, ctx=ctx)
    assert all(t.numel() == n and bool(torch.isfinite(t).all()) for t in long)
    for a, b in S.PRED_SCALAR_SLICES:  # (no random numbers on this path: a point's outputs depend on its inputs alone)
        short = A.predictive(lik, (mu[a:b].contiguous(), var[a:b].contiguous()), y[a:b].contiguous(), ctx=ctx)
        assert same(short, [t[a:b] for t in long]), (a, b)
    _device_sum_checks(A, ctx, lik, mu, var, y, long[2])
    torch.cuda.synchronize()


@pytest.mark.parametrize("bijective", [False, True], ids=["softmax", "bijective"])
def test_predictive_categorical_beyond_the_launch_cap(A, ctx, bijective):
    n, ns, sweep = S.PRED_CAT_N, 16, 7
    L, Kc = (2, 3) if bijective else (3, 3)
    rng = np.random.default_rng(31 + bijective)
    lik = A.CategoricalLikelihood(rng.normal(size=Kc) * 0.5, bijective=bijective)
    mu = TY._dev(rng.uniform(-3, 3, (n, L)))
    var = TY._dev(np.exp(rng.uniform(np.log(0.05), np.log(2.0), (n, L))) ** 2)
    cls = rng.integers(0, Kc, n)
    y_h = np.zeros((n, L), dtype=np.uint8)
    y_h[cls < L, cls[cls < L]] = 1  # class L of the bijective link: the all-zero row
    y = TY._dev(y_h)
    probs, _, lp = A.predictive(lik, (mu, var), y, nsamples=ns, sweep=sweep, ctx=ctx)
    assert tuple(probs.shape) == (n, Kc) and bool(torch.isfinite(probs).all()) and bool(torch.isfinite(lp).all())
    dev_sum = float((probs.sum(1) - 1.0).abs().max())
    print(f"categorical, n = {n}: worst |row sum - 1| {dev_sum:.3e}, bar 1e-12")
    assert dev_sum <= 1e-12
    try:
        for a, b in S.PRED_CAT_SLICES:  # a point's draws come from (seed, point offset + i, sweep)
            ctx.set_point_offset(a)
            short = A.predictive(lik, (mu[a:b].contiguous(), var[a:b].contiguous()), y[a:b].contiguous(), nsamples=ns, sweep=sweep, ctx=ctx)
            assert torch.equal(short[0], probs[a:b]) and torch.equal(short[2], lp[a:b]), (a, b)
    finally:
        ctx.set_point_offset(0)
    assert same(A.predictive(lik, (mu, var), y, nsamples=ns, sweep=sweep, ctx=ctx)[::2], (probs, lp))
    _device_sum_checks(A, ctx, lik, mu, var, y, lp, nsamples=ns, sweep=sweep)
    torch.cuda.synchronize()
