"""The all-orders additive (ANOVA) squared exponential kernel (include/agpl_kernels.h: kind 80, ``kernel=("anova_se", eta)``) on the
device against a float64 numpy restatement of k = s2 prod_d (1 - eta (1 - exp(-u_d^2 / 2))).  Every test here fails on the parent,
where the name is no kernel.  Inputs, structure and bars are those of tests/test_gpu_se_matern.py."""
import numpy as np
import pytest

from test_gpu_additive_se import A, ctx, dev, host  # noqa: F401  (A, ctx: fixtures)
from test_gpu_matern_product import fit, workload  # (the inputs and the Bernoulli fit take the kernel= value as is)

pytestmark = [pytest.mark.gpu, pytest.mark.parametrize("eta", [0.3, 1.0])]
torch = pytest.importorskip("torch")


def terms(eta, a, b, ell):
    """u [.., D], k / s2 and d (k / s2) / d u_d [.., D] = eta (-u_d e_d) prod_{d' != d} g_d' (the product without d, no division)."""
    u = (a[:, None, :] - b[None, :, :]) / ell
    e = np.exp(-0.5 * u * u)
    g = 1 - eta * (1 - e)
    excl = np.stack([np.delete(g, d, -1).prod(-1) for d in range(u.shape[-1])], -1)
    return u, g.prod(-1), -eta * u * e * excl


def kern(eta, a, b, ell, s2):
    return s2 * terms(eta, a, b, ell)[1]


def linv(eta, z, ell, s2, jitter):
    return np.linalg.solve(np.linalg.cholesky(kern(eta, z, z, ell, s2) + jitter * np.eye(len(z))), np.eye(len(z)))


@pytest.mark.parametrize("D", [1, 2, 16])
@pytest.mark.parametrize("M", [5, 260])
@pytest.mark.parametrize("N", [1, 257])
def test_features_match_float64(A, ctx, eta, N, M, D):
    """The bar of tests/test_gpu_se_matern.py: err <= max(1e-5, 2 err_two), err_two the error of the two-step route (float32 K from
    numpy, float64 L^-1, A.whiten_features) on the same points, the jitter derived as there.  At eta = 1 the "se" plan of the same
    inputs is held to the same bar (bit equality is printed, not assumed)."""
    s2, name = 2.5, ("anova_se", eta)
    jitter = M * (2.0 ** -23 * s2 / 1e-5) ** 2
    x, z, ell = workload(N, M, D)
    plan = A.Plan.from_inputs(dev(x), dev(z), ell, variance=s2, jitter=jitter, ctx=ctx, kernel=name)
    assert (plan.kernel, plan.kernel_param) == name and A.sparse.kernel_kind(name) == (80, eta)
    Li = linv(eta, z, ell, s2, jitter)
    Phi = (Li @ kern(eta, z, x, ell, s2)).T
    K32 = np.zeros((N, (M + 127) // 128 * 128), np.float32)
    K32[:, :M] = kern(eta, x, z, ell, s2)
    bar = max(1e-5, 2 * np.abs(host(A.whiten_features(torch.from_numpy(K32).cuda(), Li, ctx=ctx))[:, :M] - Phi).max())
    F, res = host(plan.features()), host(plan.resid)
    err = np.abs(F - Phi).max()
    print(f"FEATURES eta={eta} N={N} M={M} D={D}: err {err:.3e} bar {bar:.3e} max |phi| {np.abs(Phi).max():.3f}")
    assert F.shape == (N, M) and np.abs(Phi).max() > 0.1 and err <= bar and (res >= 0).all()
    assert np.abs(res - np.maximum(s2 - (Phi * Phi).sum(1), 0)).max() <= 1e-5 * s2
    if eta == 1.0:
        se = A.Plan.from_inputs(dev(x), dev(z), ell, variance=s2, jitter=jitter, ctx=ctx, kernel="se")
        print(f"eta=1 N={N} M={M} D={D}: bit-identical to se: {torch.equal(se.features(), plan.features())}")
        assert np.abs(host(se.features()) - F).max() <= bar


def test_derivative_consumers_against_central_differences(A, ctx, eta):
    """hyper_grad and inducing_grad: every entry against central differences (step 1e-6) of the float64 bound within HYPER_BAR_FULL /
    ZGRAD_BAR_FULL of the sum of |terms|.  predict_grad: mean and variance within 2e-5 of the float64 moments formed from central
    differences (step 1e-6 lengthscales) of the reference kernel in x; the last test point is 1e3 in every input, where k is the
    constant s2 (1 - eta)^D and the variance is the prior's, s2 eta / ell_d^2."""
    import hyper_reference as HR
    import zgrad_reference as ZR

    N, M, D, s2, jitter, h = 257, 5, 3, 2.5, 1e-6, 1e-6
    cavi, x, _, z, ell = fit(A, ctx, ("anova_se", eta), N, M, D, s2, 3, jitter, keep_points=True, keep_inputs=True)
    cavi.accumulate()
    cavi.check()
    gz = cavi.plan.inducing_grad(cavi.x, cavi.beta, cavi.gamma, None, cavi.G, cavi.g, with_theta=True)[1]
    th = cavi.plan.hyper_grad(cavi.x, cavi.beta, cavi.gamma, None, cavi.G, cavi.g)
    t = lambda a: torch.as_tensor(np.asarray(a, np.float64))
    q = [t(host(a)) for a in (cavi.m, cavi.S, cavi.beta, cavi.gamma)]
    eye = jitter * np.eye(M)
    Lb = lambda zz, le, ls: float(HR._bound(t(kern(eta, zz, x, np.exp(le), np.exp(ls))), t(kern(eta, zz, zz, np.exp(le), np.exp(ls)) + eye),
                                            t(np.exp(ls)), *q, None))
    le, ls = np.log(ell), np.log(s2)
    num = np.array([(Lb(z, le + h * e, ls) - Lb(z, le - h * e, ls)) / (2 * h) for e in np.eye(D)] + [(Lb(z, le, ls + h) - Lb(z, le, ls - h)) / (2 * h)])
    numz = np.array([(Lb(z + h * e.reshape(M, D), le, ls) - Lb(z - h * e.reshape(M, D), le, ls)) / (2 * h) for e in np.eye(M * D)]).reshape(M, D)
    kzx, Kzz = t(kern(eta, z, x, ell, s2)).requires_grad_(True), t(kern(eta, z, z, ell, s2) + eye).requires_grad_(True)
    Wk, Kb = (g.numpy() for g in torch.autograd.grad(HR._bound(kzx, Kzz, t(s2), *q, None), (kzx, Kzz)))
    (ux, kx, dx), (uz, kz, dz) = terms(eta, z, x, ell), terms(eta, z, z, ell)
    sc_th = np.append((np.abs(Wk)[..., None] * np.abs(ux * dx) * s2).sum((0, 1)) + (np.abs(Kb)[..., None] * np.abs(uz * dz) * s2).sum((0, 1)),
                      np.abs(Wk * s2 * kx).sum() + np.abs(Kb * s2 * kz).sum() + np.abs(0.5 * q[3].numpy() * s2).sum())
    sc_z = (np.abs(Wk)[..., None] * np.abs(dx) * s2 / ell).sum(1) + 2 * (np.abs(Kb + Kb.T)[..., None] / 2 * np.abs(dz) * s2 / ell).sum(1)
    e_th, e_z = np.abs(host(th) - num) / sc_th, np.abs(host(gz) - numz) / sc_z
    print(f"HYPER eta={eta}: theta {e_th.max() / HR.HYPER_BAR_FULL:.3f} of the bar; z {e_z.max() / ZR.ZGRAD_BAR_FULL:.3f} of the bar")
    assert np.abs(num).min() > 0 and e_th.max() <= HR.HYPER_BAR_FULL and e_z.max() <= ZR.ZGRAD_BAR_FULL, (e_th, e_z.max())
    U, v = np.tril(host(cavi.plan.U_colmajor)[0].T[:M, :M]), host(cavi.plan.v)[0, :M]
    xs = np.vstack([np.random.default_rng(23).uniform(-2, 2, size=(40, D)) * ell / np.sqrt(D), z[:1], np.full((1, D), 1e3)])
    Li = linv(eta, z, ell, s2, jitter)
    dphi = np.stack([Li @ (kern(eta, z, xs + h * ell * e, ell, s2) - kern(eta, z, xs - h * ell * e, ell, s2)) / (2 * h * ell[d])
                     for d, e in enumerate(np.eye(D))]).transpose(0, 2, 1)  # [D, Ns, M]
    rmu, Td = np.einsum("a,dna->dn", U.T @ v, dphi), np.einsum("ab,dnb->dna", U, dphi)
    prior = s2 * eta / (ell * ell)
    rvar = prior[:, None] - (dphi * dphi).sum(-1) + (Td * Td).sum(-1)
    dmu, dvar = cavi.predict_grad(dev(xs))
    g_mu = np.abs(host(dmu)[0] - rmu).max(-1) / np.abs(rmu).max(-1)
    g_var = np.abs(host(dvar)[0] - rvar).max(-1) / np.abs(rvar).max(-1)
    print(f"GRAD eta={eta}: mean {g_mu.max() / 2e-5:.3f} var {g_var.max() / 2e-5:.3f} of the bars")
    assert (g_mu <= 2e-5).all() and (g_var <= 2e-5).all() and (np.abs(rvar[:, -1] / prior - 1) < 1e-12).all()


def test_predict_cov_selection_and_spectral_frequencies(A, ctx, eta):
    from agpl_amd import _ffi

    N, M, D, s2, jitter, name = 300, 8, 3, 2.5, 1e-6, ("anova_se", eta)
    cavi, x, _, z, ell = fit(A, ctx, name, N, M, D, s2, 3, jitter)
    U = np.tril(host(cavi.plan.U_colmajor)[0].T[:M, :M])
    xs = np.random.default_rng(23).uniform(-2, 2, size=(150, D)) * ell / np.sqrt(D)  # (two 128-point tiles: a mirrored off-diagonal tile)
    phis = linv(eta, z, ell, s2, jitter) @ kern(eta, z, xs, ell, s2)
    cov_ref = kern(eta, xs, xs, ell, s2) + phis.T @ (U.T @ U - np.eye(M)) @ phis
    cov = host(cavi.predict_cov(dev(xs)))[0]
    assert np.abs(cov - cov_ref).max() <= 2e-5 * np.abs(cov_ref).max() and np.array_equal(cov, cov.T)
    with pytest.raises(A.AGPLError, match="select_inducing_greedy") as e:
        A.select_inducing(dev(x), M, ell, ctx=ctx, kernel=name)
    assert e.value.code == _ffi.ERR_UNSUPPORTED
    zg, info = A.select_inducing_greedy(dev(x), M, ell, variance=s2, kernel=name, threshold=1e-12, ctx=ctx, return_info=True)
    Kxx, piv = kern(eta, x, x, ell, s2), []
    d, cols = np.diag(Kxx).copy(), np.zeros((M, N))
    for j in range(M):  # numpy's pivoted Cholesky of the float64 K_XX, ties to the lowest index
        piv.append(int(np.argmax(d)))
        cols[j] = (Kxx[piv[j]] - cols[:j, piv[j]] @ cols[:j]) / np.sqrt(d[piv[j]])
        d = np.maximum(d - cols[j] ** 2, 0.0)
        d[piv[j]] = 0.0
    assert np.array_equal(info["indices"], piv) and np.array_equal(host(zg), x[piv])
    F = 4096  # the random-feature estimate of k / s2 at three lags: within 4 standard errors, the per-feature variance of cos(omega . du)
    omega = host(A.spectral_frequencies(name, F, D, generator=torch.Generator(device="cuda").manual_seed(5))[0])  # being (1 + k(2 du)) / 2 - k(du)^2
    du, o = np.array([[0.6, -0.5, 0.0], [0.0, 0.0, 0.7], [1.0, 0.4, -1.0]]), np.zeros((1, D))
    k1, k2 = kern(eta, du, o, np.ones(D), 1.0)[:, 0], kern(eta, 2 * du, o, np.ones(D), 1.0)[:, 0]
    err, bound = np.abs(np.cos(du @ omega.T).mean(1) - k1), 4 / np.sqrt(F) * np.sqrt((1 + k2) / 2 - k1 * k1)
    zeros = (omega == 0).mean()  # each entry is zeroed with probability 1 - eta, independently: F D Bernoulli draws
    print(f"SPECTRAL eta={eta}: err / bound {err / bound}; zero share {zeros:.4f}")
    assert (err <= bound).all() and abs(zeros - (1 - eta)) <= 4 * np.sqrt(eta * (1 - eta) / (F * D))


def test_ten_sweeps_against_the_oracle(A, ctx, eta):
    """N = 600, M = 12, D = 2: the oracle fed the plan's own features, 1e-5 on the natural parameters (tests/test_gpu_kernels.py)."""
    from oracle import oracle as O

    M = 12
    cavi, _, y, _, _ = fit(A, ctx, ("anova_se", eta), 600, M, 2, 1.0, 10, 1e-6)
    F, kd = host(cavi.plan.features()), host(cavi.plan.resid).astype(np.float64)
    S, m = np.eye(M)[None], np.zeros((1, M))
    for _ in range(10):
        G, g = O.cavi_pass(O.bernoulli(), F, kd, y, -S, m)
        S, m = O.gaussian_update(G, g)
    assert np.abs(host(cavi.G) - G).max() < 1e-5 * np.abs(G).max() and np.abs(host(cavi.g) - g).max() < 1e-5 * np.abs(g).max()
