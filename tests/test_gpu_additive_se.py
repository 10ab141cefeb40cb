"""The additive squared exponential kernel (include/agpl_kernels.h: AGPL_KERNEL_ADDITIVE_SE = 14, ``kernel="additive_se"``; 12 is
refused as no kind by tests/test_gpu_se_cosine.py, so the kind took the next free even number) on the device against float64 numpy.
Every test here fails on the parent ("additive_se" is no kernel there).  Inputs: x, z of tests/kernels_reference.py (N = 300; M = 37
and 300: the tile, pad and triangular-skip seams), lengthscales 4.8 .. 8 so that the mean u_d^2 is 2.9 .. 1.0.  K_ZZ of this kernel has
at most D r significant eigenvalues, r = 13 or so for one squared exponential over a range of 4 lengthscales, far fewer than M = 300:
the jitter is 1e-4, which bounds cond(K_ZZ + jitter I) by M s2 / jitter whatever the rank (the features test, whose bar has an
absolute floor, derives its own)."""
import numpy as np
import pytest

import kernels_reference as K

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

N, JITTER, NAT_TOL = K.N, 1e-4, 1e-5
SHAPES = [(37, 1, 1.0), (300, 1, 2.5), (37, 3, 2.5), (300, 3, 1.0), (37, 16, 1.0), (300, 16, 2.5)]  # (M, D, s2)


def k_add(a, b, ell, s2):
    u = (a[:, None, :] - b[None, :, :]) / ell
    return s2 * np.exp(-0.5 * u * u).mean(-1)


def phi_f64(x, z, ell, s2, jitter=JITTER):
    Linv = np.linalg.solve(np.linalg.cholesky(k_add(z, z, ell, s2) + jitter * np.eye(len(z))), np.eye(len(z)))
    Phi = (Linv @ k_add(z, x, ell, s2)).T
    return Phi, np.maximum(s2 - (Phi * Phi).sum(1), 0.0), Linv


def workload(M, D):
    x, z, _ = K.workload(N, M, D)
    return x, z, np.linspace(4.8, 8.0, D) if D > 1 else np.array([4.8])


@pytest.fixture(scope="module")
def A():
    import agpl_amd

    return agpl_amd


@pytest.fixture(scope="module")
def ctx(A):
    return A.Context(0, seed=19)


def host(t):
    return t.detach().cpu().numpy()


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def build(A, ctx, M, D, s2, kernel="additive_se", ell=None, x=None, jitter=JITTER):
    xw, z, e = workload(M, D)
    return A.Plan.from_inputs(dev(xw if x is None else x), dev(z), e if ell is None else ell, variance=s2, jitter=jitter, ctx=ctx,
                              kernel=kernel)


@pytest.mark.parametrize("M,D,s2", SHAPES)
def test_features_match_float64(A, ctx, M, D, s2):
    """The bar of tests/test_gpu_kernels.py, max(1e-5, 2 x the squared exponential generator's own error on the same inputs).  Its floor
    is absolute, so the jitter here follows from the number formats.  The generator's k is float32 by design (D float32 exponentials
    summed in float32): |dk| <= 2^-23 s2 per entry, and d phi_n = L^-1 dk_n with |L^-1|_2 <= jitter^-1/2 gives
    |d phi_n| <= sqrt(M) 2^-23 s2 jitter^-1/2.  The floor 1e-5 is within reach of float32 terms at all only from
    jitter = M (2^-23 s2 / 1e-5)^2 on: 5.3e-3 ... 0.27 for these shapes.  (At the module's 1e-4, rounding L^-1 and k to float32 in numpy
    alone gives 2.7e-5 at (37, 3, 2.5): cond(K_ZZ + jitter I) is 5.8e5 for this kernel and 1.1e4 for the squared exponential.)"""
    jitter = M * (2.0 ** -23 * s2 / 1e-5) ** 2
    x, z, ell = workload(M, D)
    plan = build(A, ctx, M, D, s2, jitter=jitter)
    assert plan.kernel == "additive_se" and A.sparse.kernel_kind("additive_se") == (14, 0.0)
    Phi, res, _ = phi_f64(x, z, ell, s2, jitter)
    err = np.abs(host(plan.features()) - Phi).max()
    err_se = np.abs(host(build(A, ctx, M, D, s2, "se", jitter=jitter).features()) - K.phi_f64(K.SE, x, z, ell, s2, jitter)[0]).max()
    print(f"FEATURES M={M} D={D} s2={s2}: err {err:.3e} SE generator's {err_se:.3e} bar {max(1e-5, 2 * err_se):.3e} max |phi| {np.abs(Phi).max():.3f}")
    assert np.abs(Phi).max() > 0.1 and (host(plan.resid) >= 0).all()
    assert err <= max(1e-5, 2 * err_se), (err, err_se)


@pytest.mark.parametrize("M", [37, 300])
def test_one_dimension_is_the_squared_exponential_bit_for_bit(A, ctx, M):
    a, b = build(A, ctx, M, 1, 2.5), build(A, ctx, M, 1, 2.5, "se")
    assert torch.equal(a.features(), b.features()) and torch.equal(a.resid, b.resid)


def test_dimensions_are_summed_and_lengthscales_keep_their_order(A, ctx):
    """The bar of test_kinds_differ, 1e-3 of the features' scale: against the product kernel, and against permuted lengthscales."""
    F = host(build(A, ctx, 37, 3, 1.0).features())
    for other in (build(A, ctx, 37, 3, 1.0, "se"), build(A, ctx, 37, 3, 1.0, ell=workload(37, 3)[2][::-1].copy())):
        assert np.abs(F - host(other.features())).max() > 1e-3 * np.abs(F).max()


def fit(A, ctx, M, D, s2, L=1, sweeps=3, jitter=JITTER, **kw):
    x, z, ell = workload(M, D)
    f = np.sin(x[:, 0]) + (0.1 * x[:, -1] if D > 1 else 0.0)
    rng = np.random.default_rng(21)
    if L == 1:
        lik, y = A.BernoulliLikelihood(), (rng.uniform(size=N) < 1 / (1 + np.exp(-2 * f))).astype(np.uint8)
    else:
        lik, y = A.HeteroscedasticGaussianLikelihood(2.0), (f + 0.3 * rng.standard_normal(N)).astype(np.float32)
    cavi = A.SparseCAVI.from_inputs(lik, dev(x), dev(y), dev(z), ell, variance=s2, jitter=jitter, ctx=ctx, kernel="additive_se", **kw)
    cavi.run(sweeps)
    cavi.check()
    return cavi, x, y, z, ell


@pytest.mark.parametrize("M,D,s2,L", [(37, 3, 2.5, 1), (300, 16, 1.0, 2)])
def test_predict_at_the_training_inputs_is_marginals(A, ctx, M, D, s2, L):
    cavi, x = fit(A, ctx, M, D, s2, L)[:2]
    (mu_t, var_t), (mu_m, var_m) = cavi.predict(dev(x)), cavi.marginals()
    assert mu_t.shape == (L, N) and torch.equal(mu_t, mu_m) and torch.equal(var_t, var_m)


@pytest.mark.parametrize("M,D,s2", [(37, 16, 1.0), (300, 3, 2.5)])
def test_a_shard_inside_a_tile_holds_the_full_plans_rows(A, ctx, M, D, s2):
    full, part = build(A, ctx, M, D, s2), build(A, ctx, M, D, s2, x=workload(M, D)[0][100:250].copy())
    assert torch.equal(part.features(), full.features()[100:250]) and torch.equal(part.resid, full.resid[100:250])


@pytest.mark.parametrize("M,D,s2", [(37, 3, 2.5), (300, 16, 1.0)])
def test_predict_cov_and_grad_against_float64(A, ctx, M, D, s2):
    """2e-5 of the max (per dimension for the gradient), the bars of tests/test_gpu_se_cosine.py, from the plan's own (U, v)."""
    cavi, x, _, z, ell = fit(A, ctx, M, D, s2, sweeps=10)
    U, v = np.tril(host(cavi.plan.U_colmajor)[0].T[:M, :M]), host(cavi.plan.v)[0, :M]
    xs = np.random.default_rng(23).uniform(-11, 11, size=(40, D))
    Linv = phi_f64(x, z, ell, s2)[2]
    phis = Linv @ k_add(z, xs, ell, s2)  # [M, Ns]
    cov_ref = k_add(xs, xs, ell, s2) + phis.T @ (U.T @ U - np.eye(M)) @ phis
    cov = host(cavi.predict_cov(dev(xs)))[0]
    print(f"COV M={M} D={D}: {np.abs(cov - cov_ref).max() / (2e-5 * np.abs(cov_ref).max()):.3f} of the bar")
    assert np.abs(cov - cov_ref).max() <= 2e-5 * np.abs(cov_ref).max() and np.array_equal(cov, cov.T)
    u = (xs[None, :, :] - z[:, None, :]) / ell  # [M, Ns, D];  d k / d x_d = -(s2 / D) u_d e_d / ell_d
    dphi = np.einsum("ab,bnd->dna", Linv, -(s2 / D) * u * np.exp(-0.5 * u * u) / ell)
    rmu = np.einsum("a,dna->dn", U.T @ v, dphi)
    Td = np.einsum("ab,dnb->dna", U, dphi)
    rvar = (s2 / (D * ell * ell))[:, None] - (dphi * dphi).sum(-1) + (Td * Td).sum(-1)
    dmu, dvar = cavi.predict_grad(dev(xs))
    g_mu = np.abs(host(dmu)[0] - rmu).max(-1) / np.abs(rmu).max(-1)
    g_var = np.abs(host(dvar)[0] - rvar).max(-1) / np.abs(rvar).max(-1)
    print(f"GRAD mean {g_mu.max() / 2e-5:.3f} var {g_var.max() / 2e-5:.3f} of the bar")
    assert (g_mu <= 2e-5).all() and (g_var <= 2e-5).all(), (g_mu, g_var)


def test_hyper_and_inducing_gradients_against_central_differences(A, ctx):
    """N = 300, M = 37, D = 3, three distinct lengthscales: every entry of the gradient against central differences (step 1e-6) of the
    float64 bound (tests/hyper_reference.py: _bound), within HYPER_BAR_FULL / ZGRAD_BAR_FULL of the sum of |terms|."""
    import hyper_reference as HR
    import zgrad_reference as ZR

    M, D, s2, jitter, h = 37, 3, 2.5, 1e-6, 1e-6
    cavi, x, _, z, ell = fit(A, ctx, M, D, s2, jitter=jitter, keep_points=True, keep_inputs=True)
    cavi.accumulate()
    cavi.check()
    gz = cavi.plan.inducing_grad(cavi.x, cavi.beta, cavi.gamma, None, cavi.G, cavi.g, with_theta=True)[1]
    th = cavi.plan.hyper_grad(cavi.x, cavi.beta, cavi.gamma, None, cavi.G, cavi.g)
    t = lambda a: torch.as_tensor(np.asarray(a, np.float64))
    q = [t(host(a)) for a in (cavi.m, cavi.S, cavi.beta, cavi.gamma)]
    eye = jitter * np.eye(M)
    Lb = lambda zz, le, ls: float(HR._bound(t(k_add(zz, x, np.exp(le), np.exp(ls))), t(k_add(zz, zz, np.exp(le), np.exp(ls)) + eye),
                                            t(np.exp(ls)), *q, None))
    le, ls = np.log(ell), np.log(s2)
    num = np.array([(Lb(z, le + h * e, ls) - Lb(z, le - h * e, ls)) / (2 * h) for e in np.eye(D)] + [(Lb(z, le, ls + h) - Lb(z, le, ls - h)) / (2 * h)])
    numz = np.array([(Lb(z + h * e.reshape(M, D), le, ls) - Lb(z - h * e.reshape(M, D), le, ls)) / (2 * h) for e in np.eye(M * D)]).reshape(M, D)
    # the scales: sum of |dLb / dk x dk / dtheta| over the entries of K_ZX and K_ZZ (and the prior-variance term of log s2)
    kzx, Kzz = t(k_add(z, x, ell, s2)).requires_grad_(True), t(k_add(z, z, ell, s2) + eye).requires_grad_(True)
    Wk, Kb = (g.numpy() for g in torch.autograd.grad(HR._bound(kzx, Kzz, t(s2), *q, None), (kzx, Kzz)))
    ux, uz = (z[:, None, :] - x[None, :, :]) / ell, (z[:, None, :] - z[None, :, :]) / ell
    ex, ez = (s2 / D) * np.exp(-0.5 * ux * ux), (s2 / D) * np.exp(-0.5 * uz * uz)
    sc_th = np.append((np.abs(Wk)[..., None] * ux * ux * ex).sum((0, 1)) + (np.abs(Kb)[..., None] * uz * uz * ez).sum((0, 1)),
                      np.abs(Wk * ex.sum(-1)).sum() + np.abs(Kb * ez.sum(-1)).sum() + np.abs(0.5 * q[3].numpy() * s2).sum())
    sc_z = (np.abs(Wk)[..., None] * np.abs(ux) * ex / ell).sum(1) + 2 * (np.abs(Kb + Kb.T)[..., None] / 2 * np.abs(uz) * ez / ell).sum(1)
    e_th, e_z = np.abs(host(th) - num) / sc_th, np.abs(host(gz) - numz) / sc_z
    print(f"HYPER theta {np.array2string(host(th), precision=4)} central {np.array2string(num, precision=4)}: {e_th.max() / HR.HYPER_BAR_FULL:.3f} "
          f"of the bar; z {e_z.max() / ZR.ZGRAD_BAR_FULL:.3f} of the bar, max |dz| {np.abs(numz).max():.3e}")
    assert np.abs(num).min() > 0 and e_th.max() <= HR.HYPER_BAR_FULL and e_z.max() <= ZR.ZGRAD_BAR_FULL, (e_th, e_z.max())


def test_spectral_frequencies_and_sample_paths(A, ctx):
    """The empirical kernel of F = 4096 features at 50 pairs within 5 / sqrt(2 F), the Monte-Carlo bar of
    tests/test_pathwise_reference_cpu.py::test_spectral_rule_gives_the_kernel."""
    D, F = 3, 4096
    paths = build(A, ctx, 37, D, 1.0).sample_paths(2, nfeatures=F, generator=torch.Generator(device="cuda").manual_seed(5))
    omega = host(paths.omega)
    assert omega.shape == (F, D) and ((omega != 0).sum(1) == 1).all() and torch.isfinite(paths(dev(workload(37, D)[0]))).all()
    du = np.random.default_rng(6).uniform(-3, 3, size=(50, D))
    err = np.abs(np.cos(du @ omega.T).mean(1) - np.exp(-0.5 * du * du).mean(1))
    print(f"SPECTRAL max err {err.max():.4f} bar {5 / np.sqrt(2 * F):.4f}")
    assert err.max() <= 5 / np.sqrt(2 * F)


def test_ten_sweeps_against_the_oracle(A, ctx):
    from oracle import oracle as O

    M, D = 300, 3
    cavi, _, y, _, _ = fit(A, ctx, M, D, 1.0, sweeps=10)
    F, kd = host(cavi.plan.features()), host(cavi.plan.resid).astype(np.float64)
    S, m = np.eye(M)[None], np.zeros((1, M))
    for _ in range(10):
        G, g = O.cavi_pass(O.bernoulli(), F, kd, y, -S, m)
        S, m = O.gaussian_update(G, g)
    dG, dg = np.abs(host(cavi.G) - G).max() / np.abs(G).max(), np.abs(host(cavi.g) - g).max() / np.abs(g).max()
    print(f"SWEEPS rel G {dG:.3e} rel g {dg:.3e}")
    assert dG < NAT_TOL and dg < NAT_TOL


def test_kmeans_refuses_the_kind_and_greedy_selection_is_the_pivoted_cholesky(A, ctx):
    import greedy_reference as G
    from agpl_amd import _ffi

    x, _, ell = workload(37, 3)
    with pytest.raises(A.AGPLError, match="select_inducing_greedy") as e:
        A.select_inducing(dev(x), 8, ell, ctx=ctx, kernel="additive_se")
    assert e.value.code == _ffi.ERR_UNSUPPORTED
    Mg, s2 = 20, 2.5  # (the context is still usable)
    z, info = A.select_inducing_greedy(dev(x), Mg, ell, variance=s2, kernel="additive_se", threshold=1e-12, ctx=ctx, return_info=True)
    Kxx, piv, trace = k_add(x, x, ell, s2), [], []
    d, cols = np.diag(Kxx).copy(), np.zeros((Mg, N))
    for j in range(Mg):  # numpy's pivoted Cholesky of the float64 K_XX, ties to the lowest index
        p = int(np.argmax(d))
        cols[j] = (Kxx[p] - cols[:j, p] @ cols[:j]) / np.sqrt(d[p])
        d = np.maximum(d - cols[j] ** 2, 0.0)
        d[p] = 0.0
        piv.append(p)
        trace.append(d.sum() / s2)
    assert np.array_equal(info["indices"], piv) and np.array_equal(host(z), x[piv])
    et = np.abs(info["trace"] - np.array(trace)) - 0.5 * N * 2.0 ** -G.trace_shift(N)
    assert (et <= 1e-10 * np.array(trace)).all()
