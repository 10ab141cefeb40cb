"""agpl_expected_loglik on the device (include/agpl_likgrad.h): E_q log p(y | f) and its derivatives for the likelihood's
log-parameters against float64 integration (tests/likgrad_reference.py: scipy.integrate.quad), the exact edges, the seams of the
two-level sums, every output alone, the sweep driver's expected_loglik / bound, and the learning loop."""
import ctypes as C
import dataclasses

import numpy as np
import pytest

import likgrad_reference as R

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

# worst |device - reference| / max(1, |reference|) over the 512 cases of a kind, ell and dell together: 10 x the worst value measured
# on one MI355X (the margin covers another compiler's math library).  MEASURED holds those worst values (DESIGN.md 4.21 has them split
# into ell and dell); all are far below the 1e-6 beyond which the issue calls the quadrature rule defective.
MEASURED = {"bernoulli": 2.526e-12, "negbinomial": 6.437e-12, "studentt": 1.419e-10, "poisson": 7.603e-12, "laplace": 4.325e-13,
            "heterogauss": 8.783e-11}
BLOCK, MAXBLOCKS = 512, 256  # the kernel's workgroup and the edge of the second level of its sums


@pytest.fixture(scope="module")
def A():
    import agpl_amd

    return agpl_amd


@pytest.fixture(scope="module")
def ctx(A):
    return A.Context(seed=4321)


def _lik(A, kind, p):
    return {"bernoulli": lambda: A.BernoulliLikelihood(), "negbinomial": lambda: A.NegativeBinomialLikelihood(p[0]),
            "studentt": lambda: A.StudentTLikelihood(p[0], p[1]), "poisson": lambda: A.PoissonLikelihood(p[0]),
            "laplace": lambda: A.LaplaceLikelihood(p[0]), "heterogauss": lambda: A.HeteroscedasticGaussianLikelihood(p[0])}[kind]()


def _dev(a):
    return torch.as_tensor(np.ascontiguousarray(a)).cuda()


def _run(A, ctx, lik, mu, var, y):
    tot, grad, ell, dell = A.expected_loglik(lik, _dev(mu), _dev(var), _dev(y), ctx=ctx, per_point=True)
    P = len(lik._param_names)
    return tot, grad.numpy(), ell.cpu().numpy(), dell.cpu().numpy() if P else np.empty((len(ell), 0))


def _raw(A, ctx, lik, n, mu, var, y, ell=None, dell=None, ell_sum=None, grad_sum=None):
    """The C entry point's status, no exception."""
    from agpl_amd import _ffi

    d = lik.desc()
    ptr = lambda t: C.c_void_p(0 if t is None else t.data_ptr())
    rc = _ffi.likgrad_lib().agpl_expected_loglik(ctx.bind(), C.byref(d), C.c_int64(n), ptr(mu), ptr(var), ptr(y), ptr(ell), ptr(dell),
                                                 ptr(ell_sum), ptr(grad_sum))
    torch.cuda.synchronize()
    return rc


@pytest.mark.parametrize("kind", R.KINDS)
def test_point_by_point_against_float64_integration(A, ctx, kind):
    worst_e = worst_d = 0.0
    n = 0
    for p, y, mu, var, ell_r, dell_r, eerr, derr in R.box(kind):
        _, _, ell, dell = _run(A, ctx, _lik(A, kind, p), mu, var, y)
        assert np.isfinite(ell).all() and np.isfinite(dell).all()
        worst_e = max(worst_e, (np.abs(ell - ell_r) / np.maximum(1.0, np.abs(ell_r))).max())
        if dell_r.size:
            worst_d = max(worst_d, (np.abs(dell - dell_r) / np.maximum(1.0, np.abs(dell_r))).max())
        n += len(y)
    print(f"LIKGRAD {kind}: worst |device - quad| / max(1, |quad|): ell {worst_e:.3e}, dell {worst_d:.3e} over {n} cases")
    assert n == 512
    assert max(worst_e, worst_d) <= 10.0 * MEASURED[kind]


def test_zero_variance_is_the_pointwise_likelihood_and_its_derivatives(A, ctx):
    """ell to 1e-12 of |log p(y | mu)|; a derivative is a difference of terms of the size of max(1, |value|) (r psi(y + r) - r psi(r),
    y - lambda sigma(f)), so it is held to 1e-12 of max(1, |reference|)."""
    for kind in R.KINDS:
        p, y, mu, var = R.cases(kind, 5)[0]
        _, _, ell, dell = _run(A, ctx, _lik(A, kind, p), mu, np.zeros_like(var), y)
        yf = y.astype(np.float64)
        f, g = (mu[:, 0], mu[:, 1]) if kind == "heterogauss" else (mu, None)
        ref = R.loglik(kind, p, yf, f, g)
        dref = np.array([R.dloglik(kind, p, yf[i], f[i], None if g is None else g[i]) for i in range(len(y))]) if R.NPARAMS[kind] else dell
        re = (np.abs(ell - ref) / np.abs(ref)).max()
        rd = (np.abs(dell - dref) / np.maximum(1.0, np.abs(dref))).max() if dell.size else 0.0
        print(f"LIKGRAD var = 0 {kind}: ell {re:.3e} relative, dell {rd:.3e} of max(1, |ref|)")
        assert re <= 1e-12 and rd <= 1e-12, kind


def test_bad_marginals_give_nan_at_that_point_only_and_negative_counts_minus_inf(A, ctx):
    for kind in R.KINDS:
        p, y, mu, var = (a.copy() if isinstance(a, np.ndarray) else a for a in R.cases(kind, 6)[0])
        bad = {3: ("var", -1.0), 10: ("var", np.nan), 20: ("mu", np.inf), 33: ("var", np.inf), 40: ("mu", np.nan)}
        for i, (what, val) in bad.items():
            (var if what == "var" else mu).reshape(len(y), -1)[i, -1] = val
        if kind in ("negbinomial", "poisson"):
            y[50] = -1
        if kind in ("studentt", "laplace", "heterogauss"):  # a non-finite real y follows the convention of a negative count
            y[60], y[61], y[62] = np.inf, -np.inf, np.nan
        tot, grad, ell, dell = _run(A, ctx, _lik(A, kind, p), mu, var, y)
        idx = np.zeros(len(y), dtype=bool)
        idx[list(bad)] = True
        assert np.isnan(ell[idx]).all() and np.isnan(dell[idx]).all(), kind
        ok = ~idx
        if kind in ("negbinomial", "poisson"):
            assert ell[50] == -np.inf
            ok[50] = False
        if kind in ("studentt", "laplace", "heterogauss"):
            assert ell[60] == -np.inf and ell[61] == -np.inf and np.isnan(ell[62]) and np.isnan(dell[60:63]).all(), kind
            ok[60:63] = False
        assert np.isfinite(ell[ok]).all() and np.isfinite(dell[ok]).all(), kind
        assert np.isnan(tot) and np.isnan(grad).all()  # the NaN reaches the sums


def test_errors_leave_the_context_usable(A, ctx):
    from agpl_amd import _ffi

    n = 8
    mu, var = torch.zeros(n, dtype=torch.float64, device="cuda"), torch.ones(n, dtype=torch.float64, device="cuda")
    mu2, var2 = torch.zeros((n, 2), dtype=torch.float64, device="cuda"), torch.ones((n, 2), dtype=torch.float64, device="cuda")
    yr, yi = torch.zeros(n, dtype=torch.float64, device="cuda"), torch.ones(n, dtype=torch.int32, device="cuda")
    yu = torch.ones((n, 2), dtype=torch.uint8, device="cuda")
    out, gs = torch.empty(n, dtype=torch.float64, device="cuda"), torch.empty(2, dtype=torch.float64, device="cuda")
    bad = [(A.CategoricalLikelihood(2), mu2, var2, yu), (A.CategoricalLikelihood(3, bijective=True), mu2, var2, yu),
           (A.NegativeBinomialLikelihood(0.0), mu, var, yi), (A.NegativeBinomialLikelihood(float("nan")), mu, var, yi),
           (A.StudentTLikelihood(-1.0, 1.0), mu, var, yr), (A.StudentTLikelihood(3.0, 0.0), mu, var, yr),
           (A.StudentTLikelihood(float("inf"), 1.0), mu, var, yr), (A.PoissonLikelihood(0.0), mu, var, yi),
           (A.LaplaceLikelihood(-2.0), mu, var, yr), (A.HeteroscedasticGaussianLikelihood(0.0), mu2, var2, yr)]
    for lik, m, v, y in bad:
        assert _raw(A, ctx, lik, n, m, v, y, ell=out) == _ffi.ERR_INVALID_ARGUMENT, lik
        assert _ffi.lib().agpl_last_error(ctx._h)
    bern, yb = A.BernoulliLikelihood(), torch.ones(n, dtype=torch.uint8, device="cuda")
    assert _raw(A, ctx, bern, n, mu, var, yb, ell=out, grad_sum=gs) == _ffi.ERR_INVALID_ARGUMENT
    assert _raw(A, ctx, bern, n, mu, var, yb, ell=out, dell=out) == _ffi.ERR_INVALID_ARGUMENT
    assert _raw(A, ctx, bern, -1, mu, var, yb, ell=out) == _ffi.ERR_INVALID_ARGUMENT
    assert _raw(A, ctx, bern, n, mu, var, None, ell=out) == _ffi.ERR_INVALID_ARGUMENT
    with pytest.raises(A.ArgumentError):
        A.expected_loglik(A.CategoricalLikelihood(2), mu2, var2, yu, ctx=ctx)
    # the context still works: E log sigma(f) under N(0, 1), and n = 0 gives zero sums
    assert _raw(A, ctx, bern, n, mu, var, yb, ell=out) == 0
    ref = R.ref_ell("bernoulli", (0.0,), 1, 0.0, 1.0)[0]
    assert np.abs(out.cpu().numpy() - ref).max() <= 1e-9
    gs.fill_(7.0)
    assert _raw(A, ctx, A.StudentTLikelihood(3.0, 1.0), 0, None, None, None, ell_sum=out[:1], grad_sum=gs) == 0
    assert float(out[0]) == 0.0 and gs.cpu().tolist() == [0.0, 0.0]


def _laplace_data(n, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    mu = 4.0 * torch.rand(n, dtype=torch.float64, device="cuda", generator=g) - 2.0
    var = torch.rand(n, dtype=torch.float64, device="cuda", generator=g) + 0.01
    y = mu + 3.0 + torch.randn(n, dtype=torch.float64, device="cuda", generator=g)  # |y - mu| ~ 3: ell < 0 < dell at nearly every point
    return mu, var, y


@pytest.mark.parametrize("n", [1, BLOCK - 1, BLOCK, BLOCK + 1, BLOCK * MAXBLOCKS - 1, BLOCK * MAXBLOCKS + 1])
def test_sums_at_the_reduction_seams(A, ctx, n):
    lik = A.LaplaceLikelihood(1.0)
    mu, var, y = _laplace_data(n, 100 + n % 7)
    tot, grad, ell, dell = A.expected_loglik(lik, mu, var, y, ctx=ctx, per_point=True)
    e, d = ell.cpu().numpy(), dell.cpu().numpy()[:, 0]
    assert abs(tot - e.sum()) <= 1e-12 * abs(e.sum()) and abs(float(grad[0]) - d.sum()) <= 1e-12 * abs(d.sum())
    tot2, grad2 = A.expected_loglik(lik, mu, var, y, ctx=ctx)
    assert tot2 == tot and float(grad2[0]) == float(grad[0])  # bit-identical from call to call
    if n > 1:
        h = n // 2
        ta, ga = A.expected_loglik(lik, mu[:h], var[:h], y[:h], ctx=ctx)
        tb, gb = A.expected_loglik(lik, mu[h:], var[h:], y[h:], ctx=ctx)
        assert abs(ta + tb - tot) <= 1e-12 * abs(tot) and abs(float(ga[0] + gb[0]) - float(grad[0])) <= 1e-12 * abs(float(grad[0]))


def test_every_output_alone(A, ctx):
    lik = A.StudentTLikelihood(3.0, 0.5)
    n = BLOCK + 5
    mu, var, y = _laplace_data(n, 3)
    f64 = dict(dtype=torch.float64, device="cuda")
    full = dict(ell=torch.empty(n, **f64), dell=torch.empty((n, 2), **f64), ell_sum=torch.empty(1, **f64), grad_sum=torch.empty(2, **f64))
    assert _raw(A, ctx, lik, n, mu, var, y, **full) == 0
    for name, ref in full.items():
        one = torch.full_like(ref, -7.0)
        assert _raw(A, ctx, lik, n, mu, var, y, **{name: one}) == 0
        assert torch.equal(one, ref), name
    assert _raw(A, ctx, lik, n, mu, var, y) == 0  # nothing asked for


N_FIT, M_FIT, JITTER = 4096, 32, 1e-3  # (the jitter of tests/hyper_learn_reference.py: K_ZZ of this grid stays well conditioned as the lengthscale moves)


def _data(A, ctx, gen, seed=5):
    """x, y of the synthetic workload.  It defines no Laplace data, so those are made here: its inputs, its latent
    f*(x) = 2 sin(0.7 x) + cos(0.23 x) (tests/hyper_learn_reference.py) and Laplace(beta) noise by inversion, float32 as synth_xy's."""
    if gen.kind != A.LaplaceLikelihood.kind:
        x, y = A.synth_xy(gen, seed, 0, N_FIT, ctx=ctx)
    else:
        x, _ = A.synth_xy(A.StudentTLikelihood(), seed, 0, N_FIT, ctx=ctx)
        u = torch.rand(N_FIT, dtype=torch.float64, device="cuda", generator=torch.Generator(device="cuda").manual_seed(seed)) - 0.5
        y = (2.0 * torch.sin(0.7 * x) + torch.cos(0.23 * x) - gen.beta * torch.sign(u) * torch.log1p(-2.0 * u.abs())).to(torch.float32)
    return x, y, torch.linspace(-10.0, 10.0, M_FIT, dtype=torch.float64, device="cuda")


def _fit(A, ctx, lik, gen, nsweeps, seed=5):
    x, y, z = _data(A, ctx, gen, seed)
    th = torch.tensor([1.5, 2.0], dtype=torch.float64).log()  # (through the logarithm, as learn_hyperparameters holds them)
    cavi = A.SparseCAVI.from_inputs(lik, x, y, z, th[:-1].exp(), float(th[-1].exp()), JITTER, ctx=ctx, keep_inputs=True)
    for _ in range(nsweeps):
        cavi.sweep()
    cavi.check()
    return cavi, x, y, z


def _ref_of_fit(kind, lik, cavi):
    mu, var = cavi.marginals()
    p = tuple(float(getattr(lik, k)) for k in lik._param_names)
    return R.ref_sums(kind, p, cavi.y.cpu().numpy().astype(np.float64), mu[0].cpu().numpy().astype(np.float64),
                      var[0].cpu().numpy().astype(np.float64))


def test_expected_loglik_of_a_fit_and_the_bound(A, ctx):
    lik = A.StudentTLikelihood(4.0, 0.5)
    cavi, _, _, _ = _fit(A, ctx, lik, lik, 5)
    ell, grad = cavi.expected_loglik()
    ell_r, grad_r, err = _ref_of_fit("studentt", lik, cavi)
    print(f"LIKGRAD fit: ell {ell:.10f} ref {ell_r:.10f}, grad {grad.tolist()} ref {grad_r.tolist()}, quad_vec error estimate {err:.2e}")
    # N points, each within the per-point bar times max(1, |its value|); the values of a fit are of one size, |sum| / N
    bar = 10.0 * MEASURED["studentt"] * N_FIT * max(1.0, abs(ell_r) / N_FIT)
    assert abs(ell - ell_r) <= bar + err and np.abs(grad.numpy() - grad_r).max() <= bar + err
    assert cavi.expected_loglik(grad=False) == (ell, None)
    assert cavi.bound() == ell - cavi._kl_v()
    bern = A.BernoulliLikelihood()
    cb, _, _, _ = _fit(A, ctx, bern, bern, 5)
    b, e = cb.bound(), cb.elbo()
    print(f"LIKGRAD bernoulli: bound {b:.6f} >= elbo {e:.6f}")
    assert b >= e
    tot, g = cb.expected_loglik()
    assert g.numel() == 0 and b == tot - cb._kl_v()


@pytest.mark.parametrize("kind", ["laplace", "studentt"])
def test_the_loop_learns_the_noise_scale(A, ctx, kind):
    gen = A.LaplaceLikelihood(0.25) if kind == "laplace" else A.StudentTLikelihood(4.0, 0.25)
    start = dataclasses.replace(gen, **{("beta" if kind == "laplace" else "sigma"): 1.0})
    k = len(start._param_names) - 1  # the scale is the last parameter
    x, y, z = _data(A, ctx, gen)
    lr = 0.05
    cavi, tr = A.learn_hyperparameters(start, x, y, z, 1.5, 2.0, nouter=30, nsweeps=2, lr=lr, jitter=JITTER, ctx=ctx, learn_likelihood=True)
    P = len(start._param_names)
    assert tr["lik"].shape == (31, P) and len(tr["ell"]) == 30 and tr["log_lengthscale"].shape == (31, 1)
    assert torch.equal(tr["lik"][0], torch.tensor([getattr(start, n) for n in start._param_names], dtype=torch.float64).log())
    assert [getattr(cavi.lik, n) for n in start._param_names] == pytest.approx(tr["lik"][-1].exp().tolist(), rel=1e-15)
    # the first step: Adam's is lr g / (|g| + eps), the sign of the reference gradient at the marginals the loop's first two sweeps give
    first, _, _, _ = _fit(A, ctx, start, gen, 2)
    assert first.expected_loglik()[0] == pytest.approx(tr["ell"][0], rel=1e-9)  # (the same state: the sweep is deterministic)
    _, grad_r, _ = _ref_of_fit(kind, start, first)
    step = (tr["lik"][1] - tr["lik"][0]).numpy()
    print(f"LIKGRAD loop {kind}: reference gradient {grad_r.tolist()}, first step {step.tolist()}, log-parameters {tr['lik'][0].tolist()} -> "
          f"{tr['lik'][-1].tolist()}, ell {tr['ell'][0]:.3f} -> {tr['ell'][-1]:.3f}")
    for j in range(P):
        assert np.sign(step[j]) == np.sign(grad_r[j]) and abs(abs(step[j]) - lr) <= 1e-6 * lr
    # direction, not recovery: the scale ends closer to the generating 0.25 than it started
    target = np.log(0.25)
    assert abs(float(tr["lik"][-1, k]) - target) < abs(float(tr["lik"][0, k]) - target)


def test_learn_likelihood_off_changes_no_byte_and_parameterless_kinds_are_refused(A, ctx):
    lik = A.LaplaceLikelihood(0.25)
    x, y, z = _data(A, ctx, lik)
    kw = dict(nouter=3, nsweeps=2, lr=0.05, jitter=JITTER, ctx=ctx)
    _, a = A.learn_hyperparameters(lik, x, y, z, 1.5, 2.0, **kw)
    _, b = A.learn_hyperparameters(lik, x, y, z, 1.5, 2.0, learn_likelihood=False, **kw)
    assert a["log_lengthscale"].numpy().tobytes() == b["log_lengthscale"].numpy().tobytes()
    assert a["elbo"] == b["elbo"] and "lik" not in b and "ell" not in b
    for bad in (A.BernoulliLikelihood(), A.CategoricalLikelihood(3)):
        with pytest.raises(A.ArgumentError):
            A.learn_hyperparameters(bad, x, y, z, 1.5, 2.0, learn_likelihood=True, **kw)
    # the convenience loop: the kernel fixed, no plan rebuilt, cavi.lik replaced
    cavi = A.SparseCAVI.from_inputs(A.LaplaceLikelihood(1.0), x, y, z, 1.5, 2.0, JITTER, ctx=ctx)
    plan = cavi.plan
    tr = A.learn_likelihood(cavi, nouter=5, nsweeps=2, lr=0.05)
    assert cavi.plan is plan and tr["lik"].shape == (6, 1) and len(tr["ell"]) == 5
    assert float(tr["lik"][-1, 0]) < 0.0 and cavi.lik.beta == pytest.approx(float(tr["lik"][-1, 0].exp()), rel=1e-15)
    with pytest.raises(A.ArgumentError):
        A.learn_likelihood(A.SparseCAVI.from_inputs(A.BernoulliLikelihood(), x, (y > 0).to(torch.uint8), z, 1.5, 2.0, JITTER, ctx=ctx))
