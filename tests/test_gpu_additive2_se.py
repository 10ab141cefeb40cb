"""The second-order additive squared exponential kernel (include/agpl_kernels.h: AGPL_KERNEL_ADDITIVE2_SE = 40,
``kernel=("additive2_se", w)``) on the device against float64 numpy, on the workload, jitter and bars of tests/test_gpu_additive_se.py
(N = 300; M = 37 and 300, either side of one 256-row pad; D = 1, 2 (the smallest with a pair), 3 (S1 - e_d has two terms), 16 (the
unroll limit); w = 0.3 and 1).  Every test here fails on the parent, where the name is no kernel."""
import numpy as np
import pytest

import kernels_reference as K
from test_gpu_additive_se import JITTER, N, NAT_TOL, A, ctx, dev, host, k_add, workload  # noqa: F401  (A, ctx: fixtures)

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
W = 0.3


def terms(a, b, ell, w):
    """e [.., D] and c [.., D] with k = s2 (w1 S1 + w2 E2), d k / d u_d = s2 (-u_d e_d) c_d, d k / d log ell_d = s2 u_d^2 e_d c_d."""
    u = (a[:, None, :] - b[None, :, :]) / ell
    e, D = np.exp(-0.5 * u * u), u.shape[-1]
    w1, w2 = (w / D, (1 - w) / (D * (D - 1) / 2)) if D > 1 else (1.0, 0.0)
    E2 = sum(e[..., i] * e[..., i + 1:].sum(-1) for i in range(D - 1))  # every pair once, no cancellation
    return u, e, w1 + w2 * (e.sum(-1, keepdims=True) - e), w1 * e.sum(-1) + w2 * E2


def k2(a, b, ell, s2, w=W):
    return s2 * terms(a, b, ell, w)[3]


def linv(z, ell, s2, w, jitter):
    return np.linalg.solve(np.linalg.cholesky(k2(z, z, ell, s2, w) + jitter * np.eye(len(z))), np.eye(len(z)))


def build(A, ctx, M, D, s2, kernel=("additive2_se", W), ell=None, x=None, jitter=JITTER):
    xw, z, e = workload(M, D)
    return A.Plan.from_inputs(dev(xw if x is None else x), dev(z), e if ell is None else ell, variance=s2, jitter=jitter, ctx=ctx,
                              kernel=kernel)


def test_the_kernel_is_accepted_and_its_share_checked(A, ctx):
    plan = build(A, ctx, 37, 2, 1.0)
    assert (plan.kernel, plan.kernel_param) == ("additive2_se", W) and A.sparse.kernel_kind(("additive2_se", W)) == (40, W)
    for bad in (0.0, -1.0, 1.5, float("nan"), float("inf")):
        with pytest.raises(A.ArgumentError, match="first-order share"):
            A.Plan.from_inputs(None, None, 1.0, kernel=("additive2_se", bad))


@pytest.mark.parametrize("M", [37, 300])
def test_identities_at_one_dimension_and_at_full_first_order_share(A, ctx, M):
    a, b = build(A, ctx, M, 1, 2.5), build(A, ctx, M, 1, 2.5, "se")
    assert torch.equal(a.features(), b.features()) and torch.equal(a.resid, b.resid)
    jitter = M * (2.0 ** -23 * 2.5 / 1e-5) ** 2  # the features bar's (test_features_match_float64), whose floor this holds
    for D in (3, 16):  # w = 1 is the additive kind
        a, b = build(A, ctx, M, D, 2.5, ("additive2_se", 1.0), jitter=jitter), build(A, ctx, M, D, 2.5, "additive_se", jitter=jitter)
        print(f"W=1 M={M} D={D}: bit-identical to additive_se: {torch.equal(a.features(), b.features())}")
        assert np.abs(host(a.features()) - host(b.features())).max() <= 1e-5


@pytest.mark.parametrize("M,D,s2,w,dom", [(37, 2, 2.5, W, 1), (300, 2, 1.0, W, 1), (37, 3, 2.5, W, 1), (300, 3, 1.0, 1.0, 1), (37, 16, 1.0, W, 1),
                                          (300, 16, 2.5, W, 1), (37, 3, 1.0, W, 20), (300, 3, 2.5, W, 20)])
def test_features_match_float64(A, ctx, M, D, s2, w, dom):
    """The bar and the derived jitter of tests/test_gpu_additive_se.py::test_features_match_float64.  dom = 20: the first lengthscale is
    20 x smaller, one dimension dominates every sum, where E2 formed as (S1^2 - sum e_d^2) / 2 in float32 would cancel."""
    jitter = M * (2.0 ** -23 * s2 / 1e-5) ** 2
    x, z, ell = workload(M, D)
    ell = ell / np.where(np.arange(D) == 0, dom, 1)
    Phi = (linv(z, ell, s2, w, jitter) @ k2(z, x, ell, s2, w)).T
    plan = build(A, ctx, M, D, s2, ("additive2_se", w), ell=ell, jitter=jitter)
    err = np.abs(host(plan.features()) - Phi).max()
    err_se = np.abs(host(build(A, ctx, M, D, s2, "se", ell=ell, jitter=jitter).features()) - K.phi_f64(K.SE, x, z, ell, s2, jitter)[0]).max()
    print(f"FEATURES M={M} D={D} s2={s2} w={w} dom={dom}: err {err:.3e} SE generator's {err_se:.3e} max |phi| {np.abs(Phi).max():.3f}")
    assert np.abs(Phi).max() > 0.1 and (host(plan.resid) >= 0).all() and err <= max(1e-5, 2 * err_se), (err, err_se)


def fit(A, ctx, M, D, s2, sweeps=10, jitter=JITTER, **kw):
    x, z, ell = workload(M, D)
    y = (np.random.default_rng(21).uniform(size=N) < 1 / (1 + np.exp(-2 * (np.sin(x[:, 0]) + 0.1 * x[:, -1])))).astype(np.uint8)
    cavi = A.SparseCAVI.from_inputs(A.BernoulliLikelihood(), dev(x), dev(y), dev(z), ell, variance=s2, jitter=jitter, ctx=ctx,
                                    kernel=("additive2_se", W), **kw)
    cavi.run(sweeps)
    cavi.check()
    return cavi, x, y, z, ell


@pytest.mark.parametrize("M,D,s2", [(37, 3, 2.5), (300, 16, 1.0)])
def test_consumers_after_ten_sweeps(A, ctx, M, D, s2):
    """Bit-exactness (predict at the plan's x is marginals; a shard cut inside a tile holds the full plan's rows), then predict_cov and
    predict_grad within the 2e-5 bars of tests/test_gpu_additive_se.py from the plan's own (U, v), and G, g against the oracle."""
    from oracle import oracle as O

    cavi, x, y, z, ell = fit(A, ctx, M, D, s2)
    (mu_t, var_t), (mu_m, var_m) = cavi.predict(dev(x)), cavi.marginals()
    assert torch.equal(mu_t, mu_m) and torch.equal(var_t, var_m)
    full, part = build(A, ctx, M, D, s2), build(A, ctx, M, D, s2, x=x[100:250].copy())
    assert torch.equal(part.features(), full.features()[100:250]) and torch.equal(part.resid, full.resid[100:250])
    U, v = np.tril(host(cavi.plan.U_colmajor)[0].T[:M, :M]), host(cavi.plan.v)[0, :M]
    xs = np.random.default_rng(23).uniform(-11, 11, size=(40, D))
    Linv = linv(z, ell, s2, W, JITTER)
    phis = Linv @ k2(z, xs, ell, s2)
    cov_ref = k2(xs, xs, ell, s2) + phis.T @ (U.T @ U - np.eye(M)) @ phis
    cov = host(cavi.predict_cov(dev(xs)))[0]
    assert np.abs(cov - cov_ref).max() <= 2e-5 * np.abs(cov_ref).max() and np.array_equal(cov, cov.T)
    u, e, c, _ = terms(z, xs, ell, W)  # [M, Ns, D]; u = (z - x) / ell, so d k / d x_d = +s2 u_d e_d c_d / ell_d
    dphi = np.einsum("ab,bnd->dna", Linv, s2 * u * e * c / ell)
    rmu, Td = np.einsum("a,dna->dn", U.T @ v, dphi), np.einsum("ab,dnb->dna", U, dphi)
    rvar = (s2 * (2 - W) / (D * ell * ell))[:, None] - (dphi * dphi).sum(-1) + (Td * Td).sum(-1)
    dmu, dvar = cavi.predict_grad(dev(xs))
    g_mu = np.abs(host(dmu)[0] - rmu).max(-1) / np.abs(rmu).max(-1)
    g_var = np.abs(host(dvar)[0] - rvar).max(-1) / np.abs(rvar).max(-1)
    print(f"COV {np.abs(cov - cov_ref).max() / (2e-5 * np.abs(cov_ref).max()):.3f} GRAD mean {g_mu.max() / 2e-5:.3f} var {g_var.max() / 2e-5:.3f} of the bars")
    assert (g_mu <= 2e-5).all() and (g_var <= 2e-5).all(), (g_mu, g_var)
    F, kd = host(cavi.plan.features()), host(cavi.plan.resid).astype(np.float64)
    S, m = np.eye(M)[None], np.zeros((1, M))
    for _ in range(10):
        G, g = O.cavi_pass(O.bernoulli(), F, kd, y, -S, m)
        S, m = O.gaussian_update(G, g)
    assert np.abs(host(cavi.G) - G).max() < NAT_TOL * np.abs(G).max() and np.abs(host(cavi.g) - g).max() < NAT_TOL * np.abs(g).max()


@pytest.mark.parametrize("D", [3, 16])
def test_hyper_and_inducing_gradients_against_central_differences(A, ctx, D):
    """As tests/test_gpu_additive_se.py's: every entry against central differences (step 1e-6) of the float64 bound, distinct
    lengthscales, within HYPER_BAR_FULL / ZGRAD_BAR_FULL of the sum of |terms| (the two derivative identities, restated in ``terms``)."""
    import hyper_reference as HR
    import zgrad_reference as ZR

    M, s2, jitter, h = 37, 2.5, 1e-6, 1e-6
    cavi, x, _, z, ell = fit(A, ctx, M, D, s2, sweeps=3, jitter=jitter, keep_points=True, keep_inputs=True)
    cavi.accumulate()
    cavi.check()
    gz = cavi.plan.inducing_grad(cavi.x, cavi.beta, cavi.gamma, None, cavi.G, cavi.g, with_theta=True)[1]
    th = cavi.plan.hyper_grad(cavi.x, cavi.beta, cavi.gamma, None, cavi.G, cavi.g)
    t = lambda a: torch.as_tensor(np.asarray(a, np.float64))
    q = [t(host(a)) for a in (cavi.m, cavi.S, cavi.beta, cavi.gamma)]
    eye = jitter * np.eye(M)
    Lb = lambda zz, le, ls: float(HR._bound(t(k2(zz, x, np.exp(le), np.exp(ls))), t(k2(zz, zz, np.exp(le), np.exp(ls)) + eye),
                                            t(np.exp(ls)), *q, None))
    le, ls = np.log(ell), np.log(s2)
    num = np.array([(Lb(z, le + h * e, ls) - Lb(z, le - h * e, ls)) / (2 * h) for e in np.eye(D)] + [(Lb(z, le, ls + h) - Lb(z, le, ls - h)) / (2 * h)])
    numz = np.array([(Lb(z + h * e.reshape(M, D), le, ls) - Lb(z - h * e.reshape(M, D), le, ls)) / (2 * h) for e in np.eye(M * D)]).reshape(M, D)
    kzx, Kzz = t(k2(z, x, ell, s2)).requires_grad_(True), t(k2(z, z, ell, s2) + eye).requires_grad_(True)
    Wk, Kb = (g.numpy() for g in torch.autograd.grad(HR._bound(kzx, Kzz, t(s2), *q, None), (kzx, Kzz)))
    (ux, ex, cx, kx), (uz, ez, cz, kz) = terms(z, x, ell, W), terms(z, z, ell, W)
    ex, ez = s2 * ex * cx, s2 * ez * cz  # |d k / d u_d| = |u_d| times these
    sc_th = np.append((np.abs(Wk)[..., None] * ux * ux * ex).sum((0, 1)) + (np.abs(Kb)[..., None] * uz * uz * ez).sum((0, 1)),
                      np.abs(Wk * s2 * kx).sum() + np.abs(Kb * s2 * kz).sum() + np.abs(0.5 * q[3].numpy() * s2).sum())
    sc_z = (np.abs(Wk)[..., None] * np.abs(ux) * ex / ell).sum(1) + 2 * (np.abs(Kb + Kb.T)[..., None] / 2 * np.abs(uz) * ez / ell).sum(1)
    e_th, e_z = np.abs(host(th) - num) / sc_th, np.abs(host(gz) - numz) / sc_z
    print(f"HYPER D={D}: theta {e_th.max() / HR.HYPER_BAR_FULL:.3f} of the bar; z {e_z.max() / ZR.ZGRAD_BAR_FULL:.3f} of the bar, max |dz| {np.abs(numz).max():.3e}")
    assert np.abs(num).min() > 0 and e_th.max() <= HR.HYPER_BAR_FULL and e_z.max() <= ZR.ZGRAD_BAR_FULL, (e_th, e_z.max())


def test_spectral_frequencies(A, ctx):
    """The Monte-Carlo bar of tests/test_gpu_additive_se.py, 5 / sqrt(2 F); the share of one-dimensional features within 5 binomial
    standard errors of w; the additive kind's stream of draws restated from its rule (normals, one dimension, phase)."""
    D, F = 3, 4096
    gen = lambda: torch.Generator(device="cuda").manual_seed(5)
    paths = build(A, ctx, 37, D, 1.0).sample_paths(2, nfeatures=F, generator=gen())
    omega, nz = host(paths.omega), (host(paths.omega) != 0).sum(1)
    assert omega.shape == (F, D) and np.isin(nz, (1, 2)).all() and torch.isfinite(paths(dev(workload(37, D)[0]))).all()
    assert abs((nz == 1).mean() - W) <= 5 * np.sqrt(W * (1 - W) / F)
    du = np.random.default_rng(6).uniform(-3, 3, size=(50, D))
    err = np.abs(np.cos(du @ omega.T).mean(1) - k2(du, np.zeros((1, D)), np.ones(D), 1.0)[:, 0])
    print(f"SPECTRAL max err {err.max():.4f} bar {5 / np.sqrt(2 * F):.4f} share of one-dimensional features {(nz == 1).mean():.4f}")
    assert err.max() <= 5 / np.sqrt(2 * F)
    om, ph = A.spectral_frequencies("additive_se", F, D, generator=gen())
    g = gen()
    n = torch.randn((F, D), dtype=torch.float64, device="cuda", generator=g)
    n = n * torch.nn.functional.one_hot(torch.randint(0, D, (F,), device="cuda", generator=g), D)
    assert torch.equal(om, n) and torch.equal(ph, torch.rand(F, dtype=torch.float64, device="cuda", generator=g) * (2.0 * np.pi))


def test_selection_and_refusals(A, ctx):
    import test_gpu_kernels as TK
    from agpl_amd import _ffi

    x, z, ell = workload(37, 3)
    with pytest.raises(A.AGPLError, match="select_inducing_greedy") as e:
        A.select_inducing(dev(x), 8, ell, ctx=ctx, kernel=("additive2_se", W))
    assert e.value.code == _ffi.ERR_UNSUPPORTED
    for kind, words in ((15, "unknown kernel kind"), (39, "unknown kernel kind"), (40, "first-order share")):  # (40 with w = 1.5)
        rc, pl, msg = TK.raw_plan(A, ctx, "stationary", kind, 1.5, x, z, ell)
        assert rc == _ffi.ERR_INVALID_ARGUMENT and pl is None and words in msg, (kind, rc, msg)
    Mg, s2 = 20, 2.5
    zg, info = A.select_inducing_greedy(dev(x), Mg, ell, variance=s2, kernel=("additive2_se", W), threshold=1e-12, ctx=ctx, return_info=True)
    Kxx, piv = k2(x, x, ell, s2), []
    d, cols = np.diag(Kxx).copy(), np.zeros((Mg, N))
    for j in range(Mg):  # numpy's pivoted Cholesky of the float64 K_XX, ties to the lowest index
        p = int(np.argmax(d))
        cols[j] = (Kxx[p] - cols[:j, p] @ cols[:j]) / np.sqrt(d[p])
        d = np.maximum(d - cols[j] ** 2, 0.0)
        d[p] = 0.0
        piv.append((p, d.sum() / s2))
    import greedy_reference as G

    trace = np.array([t for _, t in piv])
    assert np.array_equal(info["indices"], [p for p, _ in piv]) and np.array_equal(host(zg), x[[p for p, _ in piv]])
    assert (np.abs(info["trace"] - trace) - 0.5 * N * 2.0 ** -G.trace_shift(N) <= 1e-10 * trace).all()
