"""The squared exponential x categorical kernel (include/agpl_kernels.h: kind 96, ``kernel=("se_categorical", C)``) on the device against
a float64 numpy restatement of k = s2 exp(-(sum_{d < D - C} u_d^2 + sum_{d >= D - C} [x_d != x'_d] / ell_d^2) / 2).  Every test here
fails on the parent, where the name is no kernel.  Structure and bars are those of tests/test_gpu_anova_se.py; the codes are drawn from
0 ... 4, so that equal and unequal pairs meet in every quad of inducing inputs."""
import numpy as np
import pytest

from test_gpu_additive_se import A, ctx, dev, host  # noqa: F401  (A, ctx: fixtures)

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
S2, N = 2.5, 300  # (N: two ragged 128-point tiles)


def workload(n, M, D, C, seed=7, levels=5):
    rng = np.random.default_rng(seed)
    ell = np.r_[np.where(np.arange(D - C) % 2 == 0, 0.3, 3.0), 0.7 + 0.4 * np.arange(C)]
    x, z = (np.c_[rng.uniform(-2, 2, (m, D - C)) * ell[:D - C] / np.sqrt(D), rng.integers(0, levels, (m, C))].astype(np.float64) for m in (n, M))
    return x, z, ell


def terms(C, a, b, ell):
    """The warped u [n, m, D] (u_d = [codes differ] / ell_d in the last C inputs), k / s2 = exp(-|u|^2 / 2) and d u_d / d a_d [D]."""
    d = a[:, None, :] - b[None, :, :]
    lead = np.arange(a.shape[1]) < a.shape[1] - C
    u = np.where(lead, d, d != 0) / ell
    return u, np.exp(-0.5 * (u * u).sum(-1)), lead / ell


def kern(C, a, b, ell):
    return S2 * terms(C, a, b, ell)[1]


def linv(C, z, ell, jitter):
    return np.linalg.solve(np.linalg.cholesky(kern(C, z, z, ell) + jitter * np.eye(len(z))), np.eye(len(z)))


@pytest.mark.parametrize("D,C,levels", [(1, 1, 5), (3, 1, 5), (4, 2, 5), (16, 3, 5), (2, 2, 5), (3, 1, 1)])
@pytest.mark.parametrize("M", [5, 130])
def test_features_match_float64(A, ctx, M, D, C, levels):
    """The bar of tests/test_gpu_anova_se.py: err <= max(1e-5, 2 err_two), err_two the error of the two-step route (float32 K from
    numpy, float64 L^-1, A.whiten_features) on the same points, the jitter derived as there.  levels = 1: the categorical column is
    constant over x and z, and the "se" plan of the leading inputs is held to the same bar (not bit for bit)."""
    name, jitter = ("se_categorical", C), M * (2.0 ** -23 * S2 / 1e-5) ** 2
    x, z, ell = workload(N, M, D, C, levels=levels)
    plan = A.Plan.from_inputs(dev(x), dev(z), ell, variance=S2, jitter=jitter, ctx=ctx, kernel=name)
    assert (plan.kernel, plan.kernel_param) == name
    Li = linv(C, z, ell, jitter)
    Phi = (Li @ kern(C, z, x, ell)).T
    K32 = np.zeros((N, (M + 127) // 128 * 128), np.float32)
    K32[:, :M] = kern(C, x, z, ell)
    bar = max(1e-5, 2 * np.abs(host(A.whiten_features(torch.from_numpy(K32).cuda(), Li, ctx=ctx))[:, :M] - Phi).max())
    F, res = host(plan.features()), host(plan.resid)
    err = np.abs(F - Phi).max()
    print(f"FEATURES M={M} D={D} C={C} levels={levels}: err {err:.3e} bar {bar:.3e} max |phi| {np.abs(Phi).max():.3f}")
    assert F.shape == (N, M) and np.abs(Phi).max() > 0.1 and err <= bar and (res >= 0).all()
    assert np.abs(res - np.maximum(S2 - (Phi * Phi).sum(1), 0)).max() <= 1e-5 * S2
    if levels == 1:
        se = A.Plan.from_inputs(dev(x[:, :D - C]), dev(z[:, :D - C]), ell[:D - C], variance=S2, jitter=jitter, ctx=ctx, kernel="se")
        assert np.abs(host(se.features()) - F).max() <= bar


@pytest.fixture(scope="module")
def fitted(A, ctx):
    """Two Bernoulli sweeps at N = 300, M = 5, (D, C) = (4, 2), and the natural parameters they end with; shared and not changed."""
    x, z, ell = workload(N, 5, 4, 2)
    y = (np.random.default_rng(21).uniform(size=N) < 1 / (1 + np.exp(1 - 2 * np.sin(3 * x[:, 0] / ell[0]) - x[:, 3]))).astype(np.uint8)
    cavi = A.SparseCAVI.from_inputs(A.BernoulliLikelihood(), dev(x), dev(y), dev(z), ell, variance=S2, jitter=1e-6, ctx=ctx,
                                    kernel=("se_categorical", 2), keep_points=True, keep_inputs=True)
    cavi.run(2)
    cavi.check()
    Gg = host(cavi.G).copy(), host(cavi.g).copy()
    cavi.accumulate()
    cavi.check()
    M = 5
    return cavi, x, y, z, ell, Gg, np.tril(host(cavi.plan.U_colmajor)[0].T[:M, :M]), host(cavi.plan.v)[0, :M], linv(2, z, ell, 1e-6)


def test_two_sweeps_against_the_reference_sweep(fitted):
    """The float64 oracle's two sweeps on the REFERENCE features, 1e-5 on the natural parameters (tests/test_gpu_anova_se.py's bar)."""
    from oracle import oracle as O

    _, x, y, z, ell, (Gd, gd), _, _, Li = fitted
    Phi = (Li @ kern(2, z, x, ell)).T
    S, m = np.eye(5)[None], np.zeros((1, 5))
    for _ in range(2):
        G, g = O.cavi_pass(O.bernoulli(), Phi, np.maximum(S2 - (Phi * Phi).sum(1), 0), y, -S, m)
        S, m = O.gaussian_update(G, g)
    print(f"SWEEPS: G {np.abs(Gd - G).max() / np.abs(G).max():.3e} g {np.abs(gd - g).max() / np.abs(g).max():.3e} (bar 1e-5)")
    assert np.abs(Gd - G).max() < 1e-5 * np.abs(G).max() and np.abs(gd - g).max() < 1e-5 * np.abs(g).max()


def test_predict_and_predict_cov(fitted):
    cavi, _, _, z, ell, _, U, v, Li = fitted
    xs = workload(150, 1, 4, 2, seed=23)[0]  # (two 128-point tiles: a mirrored off-diagonal tile)
    phis = Li @ kern(2, z, xs, ell)
    cov_ref, mu_ref = kern(2, xs, xs, ell) + phis.T @ (U.T @ U - np.eye(5)) @ phis, (U.T @ v) @ phis
    cov, (mu, var) = host(cavi.predict_cov(dev(xs)))[0], cavi.predict(dev(xs))
    assert np.abs(cov - cov_ref).max() <= 2e-5 * np.abs(cov_ref).max() and np.array_equal(cov, cov.T)
    assert np.abs(host(mu)[0] - mu_ref).max() <= 2e-5 * np.abs(mu_ref).max()
    assert np.abs(host(var)[0] - np.diag(cov_ref)).max() <= 2e-5 * np.diag(cov_ref).max()


def test_gradients_against_the_closed_forms(A, ctx, fitted):
    """hyper_grad and inducing_grad against the closed-form float64 gradient of the reference bound (its derivatives in K_ZX, K_ZZ and
    s2 by autograd of tests/hyper_reference.py's _bound, then d k / d log ell_d = u_d^2 k and d k / d z_ad = -k u_d / ell_d, 0 in a
    categorical input) within HYPER_BAR_FULL / ZGRAD_BAR_FULL of the sum of |terms|; the categorical columns of the inducing gradient
    are exactly 0.  predict_grad: leading inputs within 2e-5 of the float64 moments, categorical outputs exactly 0; all 0 at C = D."""
    import hyper_reference as HR
    import zgrad_reference as ZR

    cavi, x, _, z, ell, _, U, v, Li = fitted
    M, D, C = 5, 4, 2
    gz = host(cavi.plan.inducing_grad(cavi.x, cavi.beta, cavi.gamma, None, cavi.G, cavi.g, with_theta=True)[1])
    th = host(cavi.plan.hyper_grad(cavi.x, cavi.beta, cavi.gamma, None, cavi.G, cavi.g))
    t = lambda a: torch.as_tensor(np.asarray(a, np.float64))
    q = [t(host(a)) for a in (cavi.m, cavi.S, cavi.beta, cavi.gamma)]
    leaves = [t(a).requires_grad_(True) for a in (kern(C, z, x, ell), kern(C, z, z, ell) + 1e-6 * np.eye(M), S2)]
    Wk, Kb, gs = (g.numpy() for g in torch.autograd.grad(HR._bound(*leaves, *q, None), leaves))
    (ux, kx, da), (uz, kz, _) = terms(C, z, x, ell), terms(C, z, z, ell)
    tx, tz = (Wk * S2 * kx)[..., None] * ux, ((Kb + Kb.T) / 2 * S2 * kz)[..., None] * uz  # (coefficient k) u_d, per pair and input
    ref_th = np.append((tx * ux).sum((0, 1)) + (tz * uz).sum((0, 1)), (Wk * S2 * kx).sum() + (Kb * S2 * kz).sum() + S2 * gs)
    sc_th = np.append(np.abs(tx * ux).sum((0, 1)) + np.abs(tz * uz).sum((0, 1)),
                      np.abs(Wk * S2 * kx).sum() + np.abs(Kb * S2 * kz).sum() + np.abs(0.5 * q[3].numpy() * S2).sum())
    ref_z, sc_z = -(tx * da).sum(1) - 2 * (tz * da).sum(1), np.abs(tx * da).sum(1) + 2 * np.abs(tz * da).sum(1)
    e_th, e_z = np.abs(th - ref_th) / sc_th, np.abs(gz - ref_z)[:, :D - C] / sc_z[:, :D - C]
    print(f"HYPER: theta {e_th.max() / HR.HYPER_BAR_FULL:.3f} of the bar; z {e_z.max() / ZR.ZGRAD_BAR_FULL:.3f} of the bar")
    assert np.abs(ref_th).min() > 0 and e_th.max() <= HR.HYPER_BAR_FULL and e_z.max() <= ZR.ZGRAD_BAR_FULL and (gz[:, D - C:] == 0.0).all()
    xs = workload(40, 1, D, C, seed=23)[0]
    us, ks, dx = terms(C, xs, z, ell)
    dphi = np.einsum("ab,nbd->dna", Li, -(S2 * ks)[..., None] * us * dx)[:D - C]  # d phi(x_n) / d x_nd, leading d
    rmu, Td = np.einsum("a,dna->dn", U.T @ v, dphi), np.einsum("ab,dnb->dna", U, dphi)
    rvar = (S2 / ell[:D - C] ** 2)[:, None] - (dphi * dphi).sum(-1) + (Td * Td).sum(-1)
    dmu, dvar = (host(a)[0] for a in cavi.predict_grad(dev(xs)))
    g_mu, g_var = np.abs(dmu[:D - C] - rmu).max(-1) / np.abs(rmu).max(-1), np.abs(dvar[:D - C] - rvar).max(-1) / np.abs(rvar).max(-1)
    print(f"GRAD: mean {g_mu.max() / 2e-5:.3f} var {g_var.max() / 2e-5:.3f} of the bars")
    assert (g_mu <= 2e-5).all() and (g_var <= 2e-5).all() and (dmu[D - C:] == 0.0).all() and (dvar[D - C:] == 0.0).all()
    x2, z2, ell2 = workload(N, M, 2, 2)
    both = A.Plan.from_inputs(dev(x2), dev(z2), ell2, variance=S2, jitter=1e-2, ctx=ctx, kernel=("se_categorical", 2)).predict_grad(dev(x2[:40]))
    assert all(a.shape == (1, 2, 40) and (host(a) == 0.0).all() for a in both)


def test_selection_and_spectral_frequencies(A, ctx, fitted):
    import greedy_reference as G
    from agpl_amd import _ffi

    M, D, C, name = 8, 3, 1, ("se_categorical", 1)
    x, _, ell = workload(N, M, D, C)
    with pytest.raises(A.AGPLError, match="select_inducing_greedy") as e:
        A.select_inducing(dev(x), M, ell, ctx=ctx, kernel=name)
    assert e.value.code == _ffi.ERR_UNSUPPORTED
    zg, info = A.select_inducing_greedy(dev(x), M, ell, variance=S2, kernel=name, threshold=1e-12, ctx=ctx, return_info=True)
    Kxx, piv, trace = kern(C, x, x, ell), [], []
    d, cols = np.diag(Kxx).copy(), np.zeros((M, N))
    for j in range(M):  # numpy's pivoted Cholesky of the float64 K_XX, ties to the lowest index
        piv.append(int(np.argmax(d)))
        cols[j] = (Kxx[piv[j]] - cols[:j, piv[j]] @ cols[:j]) / np.sqrt(d[piv[j]])
        d = np.maximum(d - cols[j] ** 2, 0.0)
        d[piv[j]] = 0.0
        trace.append(d.sum() / S2)
    assert np.array_equal(info["indices"], piv) and np.array_equal(host(zg), x[piv])
    assert (np.abs(info["trace"] - np.array(trace)) - 0.5 * N * 2.0 ** -G.trace_shift(N) <= 1e-10 * np.array(trace)).all()
    F = 4096  # the random-feature estimate of k / s2 at three lags (equal codes; unequal codes; unequal codes and a continuous lag): within
    gen = torch.Generator(device="cuda").manual_seed(5)  # 4 standard errors, the per-feature variance being (1 + k(2 du)) / 2 - k(du)^2
    omega = host(A.spectral_frequencies(name, F, D, generator=gen, lengthscale=ell)[0])
    du, o = np.array([[0.6, -0.5, 0.0], [0.0, 0.0, 2.0], [1.0, 0.4, -3.0]]) * np.r_[ell[:2], 1.0], np.zeros((1, D))
    k1, k2 = kern(C, du, o, ell)[:, 0] / S2, kern(C, 2 * du, o, ell)[:, 0] / S2
    err, bound = np.abs(np.cos((du / ell) @ omega.T).mean(1) - k1), 4 / np.sqrt(F) * np.sqrt((1 + k2) / 2 - k1 * k1)
    print(f"SPECTRAL: err / bound {err / bound}")
    assert (err <= bound).all() and len(np.unique(np.rint(omega[:, 2] * 64 / (2 * np.pi * ell[2])))) > 32
    with pytest.raises(_ffi.ArgumentError, match="pass lengthscale="):
        A.spectral_frequencies(name, 16, D)
    f = fitted[0].sample_paths(4, nfeatures=256)(dev(fitted[1][:40]))  # (the plan passes its own kernel and lengthscales)
    assert f.shape == (4, 1, 40) and torch.isfinite(f).all()
