"""The per-point likelihood rules on the device, point by point, over the edge grid of tests/lik_rules_reference.py: the array-fed
operators in float32 and float64 and the float64 ELBO terms against mpmath within bars derived from the arithmetic (or in the expected
non-finite class), the sweep's per-point kernel against the float32 operators bit for bit, and the domain report of every likelihood.
The reference, the bars, the grid and what "unresolved" means are the docstring of tests/lik_rules_reference.py;
tests/test_lik_rules_reference_cpu.py holds them against the oracle and against wrong variants without a GPU.

Every case prints ``LIK_RULES_GPU <what>: worst ratio`` before it asserts."""
import numpy as np
import pytest

import lik_rules_reference as R

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")


@pytest.fixture(scope="module")
def A():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import __graft_entry__ as g

    g.build()
    import agpl_amd

    return agpl_amd


@pytest.fixture(scope="module")
def ctx(A):
    return A.Context(0, seed=20241019)


def make_lik(A, kind, params):
    if kind == "bernoulli":
        return A.BernoulliLikelihood()
    if kind == "negbin":
        return A.NegativeBinomialLikelihood(params["r"])
    if kind == "studentt":
        return A.StudentTLikelihood(params["nu"], params["sigma"])
    if kind in ("cat", "catbij"):
        return A.CategoricalLikelihood(np.array(params["logtheta"], np.float64), bijective=kind == "catbij")
    if kind == "poisson":
        return A.PoissonLikelihood(params["lam"])
    if kind == "laplace":
        return A.LaplaceLikelihood(params["beta"])
    return A.HeteroscedasticGaussianLikelihood(params["lam"])


def _tdt(fmt):
    return torch.float32 if fmt.name == "f32" else torch.float64


def _dev(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda().to(dtype).contiguous()


def _y_dev(lik, ys, tdt):
    """y of n points ([n][Ly] floats) as the operators take it."""
    a = np.asarray(ys, np.float64)
    if lik.ykind == "real":
        return _dev(a[:, 0], tdt)
    dt = torch.uint8 if lik.ykind == "u8" else torch.int32
    a = a.astype(np.int64)
    return _dev(a if lik._nlatent > 1 else a[:, 0], dt)


def _cols(t, n):
    """[n] or [n, La] device tensor -> [n][La] floats (exact)."""
    return t.detach().cpu().numpy().astype(np.float64).reshape(n, -1)


class DeviceImpl:
    """The device's operators behind the interface of lik_rules_reference.ModelImpl: one launch per call."""

    def __init__(self, A, ctx):
        self.A, self.ctx = A, ctx

    def _qf(self, lik, mus, vs, tdt):
        mu, var = np.asarray(mus, np.float64), np.asarray(vs, np.float64)
        if lik._nlatent == 1:
            mu, var = mu[:, 0], var[:, 0]
        return _dev(mu, tdt), _dev(var, tdt)

    def aux_posterior(self, kind, fmt, params, ys, mus, vs):
        A, tdt, n = self.A, _tdt(fmt), len(ys)
        lik = make_lik(A, kind, params)
        yd = _y_dev(lik, ys, tdt)
        q = A.aux_posterior(lik, yd, self._qf(lik, mus, vs, tdt), ctx=self.ctx)
        phi = q.inds[0]
        if "y" in phi.keys():
            assert torch.equal(phi["y"].reshape(-1), yd.reshape(-1)), "integer copy of y is not bit-exact"
        f = [_cols(phi[k], n) for k in phi.keys() if k != "y"]
        return [(f[0][i], f[1][i] if len(f) > 1 else [], f[2][i][0] if len(f) > 2 else None) for i in range(n)]

    def _q(self, lik, fmt, ys, q1s, q2s):
        A, tdt, n = self.A, _tdt(fmt), len(ys)
        q = A.init_aux_posterior(lik, n, dtype=tdt, ctx=self.ctx)
        phi = q.inds[0]
        names = [k for k in phi.keys() if k != "y"]
        phi[names[0]].copy_(_dev(q1s, tdt).reshape(phi[names[0]].shape))
        if len(names) > 1 and len(q2s[0]):
            phi[names[1]].copy_(_dev(q2s, tdt).reshape(phi[names[1]].shape))
        return q

    def expected_pp(self, kind, fmt, params, ys, q1s, q2s, mugs):
        A, tdt, n = self.A, _tdt(fmt), len(ys)
        lik = make_lik(A, kind, params)
        q = self._q(lik, fmt, ys, q1s, q2s)
        qf = None
        if kind == "hetero":
            m = np.zeros((n, 2))
            m[:, 1] = mugs
            qf = (_dev(m, tdt), _dev(np.ones((n, 2)), tdt))
        beta, gamma = A.expected_auglik_potential_and_precision(lik, q, _y_dev(lik, ys, tdt), qf, ctx=self.ctx)
        g = np.stack([t.detach().cpu().numpy().astype(np.float64) for t in gamma], 1)
        b = np.stack([t.detach().cpu().numpy().astype(np.float64) for t in beta], 1)
        return [(g[i], b[i]) for i in range(n)]

    def elbo_term(self, kind, which, params, y, q1, q2, mu, var, copies=1):
        A = self.A
        lik = make_lik(A, kind, params)
        rep = lambda s: [list(s)] * copies
        q = self._q(lik, R.F64, rep(y), rep(q1), rep(q2))
        yd = _y_dev(lik, rep(y), torch.float64)
        qf = self._qf(lik, rep(mu), rep(var), torch.float64)
        if which == "elt":
            return A.expected_logtilt(lik, q, yd, qf, ctx=self.ctx)
        if which == "kl":
            return A.aux_kldivergence(lik, q, yd, ctx=self.ctx)
        return A.expected_aug_loglik(lik, q, yd, qf, ctx=self.ctx)


@pytest.mark.parametrize("fmt", ["f32", "f64"])
@pytest.mark.parametrize("kind", R.KINDS)
def test_operators_point_by_point(A, ctx, kind, fmt):
    """agpl_aux_posterior and agpl_expected_potential_precision on the whole grid (one launch per parameter set): every resolved
    output within its bar of the mpmath value, every unresolved one in the model's class, integer copies bit-exact."""
    recs = R.evaluate_operators(kind, R.FMT[fmt], DeviceImpl(A, ctx))
    worst, fails, unres = R.summarize(recs)
    print(f"LIK_RULES_GPU operators {kind} {fmt}: {len(recs)} outputs, worst |device - mpmath| / bar {worst:.3f}, unresolved {unres}")
    assert not fails, "\n".join(fails)


def _same(a, b):
    return (a != a and b != b) or a == b


@pytest.mark.parametrize("kind", R.KINDS)
def test_elbo_terms_point_by_point(A, ctx, kind):
    """agpl_expected_logtilt / agpl_aux_kldivergence / agpl_expected_aug_loglik with n = 1 per grid point -- a per-point check made
    of a reduction -- and with n = 257 identical copies, which crosses a workgroup: block 0's tree gives 256 t exactly, block 1 gives
    t, and the final sum is fl(256 t + t)."""
    impl = DeviceImpl(A, ctx)
    recs = R.evaluate_elbo(kind, impl)
    worst, fails, unres = R.summarize(recs)
    print(f"LIK_RULES_GPU elbo terms {kind}: {len(recs)} terms, worst |device - mpmath| / bar {worst:.3f}, unresolved {unres}")
    assert not fails, "\n".join(fails)
    inputs = {nm: rest for nm, *rest in R.elbo_inputs(kind)}
    bad = []
    for r in recs:
        params, y, q1, q2, mu, var = inputs[r.point]
        t257 = impl.elbo_term(kind, r.out, params, y, q1, q2, mu, var, copies=257)
        with np.errstate(all="ignore"):
            want = float(np.float64(256.0) * np.float64(r.got) + np.float64(r.got))
        if not _same(t257, want):
            bad.append(f"{r.point} / {r.out}: 257 copies give {t257!r}, the fixed-order tree of 257 terms {r.got!r} gives {want!r}")
        elif not r.ref.unresolved and np.isfinite(t257) and abs(R.mpf(t257) - 257 * r.ref.v) > 257 * r.ref.bar:
            bad.append(f"{r.point} / {r.out}: 257 copies leave 257 bar")
    assert not bad, "\n".join(bad)


def _bits(t):
    return t.detach().contiguous().view(torch.int32).cpu().numpy()


# plan points per likelihood (lik_rules_reference.plan_points over the float32 grid): (finite gamma >= 0 and beta, other classes)
PLAN_POINTS = {"bernoulli": (12, 0), "negbin": (26, 0), "studentt": (25, 0), "cat": (26, 4), "catbij": (50, 0), "poisson": (32, 0),
               "laplace": (25, 0), "hetero": (30, 4)}
HAS_ELBO = ("bernoulli", "negbin", "studentt", "catbij", "poisson", "laplace")


def _operators_on(A, ctx, lik, yd, mu, var):
    """(c, gamma [L][n], beta [L][n]) of the float32 array-fed operators on marginals [L][n]."""
    L = lik._nlatent
    qf = (mu[0], var[0]) if L == 1 else (mu.t().contiguous(), var.t().contiguous())
    q = A.aux_posterior(lik, yd, qf, ctx=ctx)
    beta, gamma = A.expected_auglik_potential_and_precision(lik, q, yd, qf, ctx=ctx)
    q1 = q.inds[0][[k for k in q.inds[0].keys() if k != "y"][0]]
    return q1.reshape(-1), torch.stack(list(gamma)), torch.stack(list(beta))


def _assert_same_bits(tag, names, cavi, c, gamma, beta):
    for what, got, want in (("gamma", cavi.gamma, gamma), ("beta", cavi.beta, beta), ("c", cavi.c.reshape(-1)[: c.numel()], c)):
        g, w = _bits(got).reshape(-1), _bits(want).reshape(-1)
        d = np.nonzero(g != w)[0]
        n = len(names)
        assert d.size == 0, (tag, what, [(names[i % n] if what != "c" else int(i), int(g[i]), int(w[i])) for i in d[:5]])


def _elbo_sum_of_item_two(A, ctx, lik, yd, mu, var):
    """(sum over the points of expected_logtilt_i - aux_kldivergence_i, sum |terms|, all finite): the float64 operators with n = 1
    per point on the float64 casts of float32 marginals [L][n]."""
    f64, L, n = torch.float64, lik._nlatent, mu.shape[1]
    y64 = yd.to(f64) if lik.ykind == "real" else yd
    tot, mag, finite = 0.0, 0.0, True
    for i in range(n):
        qf = (mu[0, i:i + 1].to(f64), var[0, i:i + 1].to(f64)) if L == 1 else (mu[:, i:i + 1].t().contiguous().to(f64), var[:, i:i + 1].t().contiguous().to(f64))
        yi = y64[i:i + 1].contiguous()
        q = A.aux_posterior(lik, yi, qf, ctx=ctx)
        e, k = A.expected_logtilt(lik, q, yi, qf, ctx=ctx), A.aux_kldivergence(lik, q, yi, ctx=ctx)
        finite = finite and bool(np.isfinite(e) and np.isfinite(k))
        tot, mag = tot + (e - k), mag + abs(e) + abs(k)
    return tot, mag, finite


@pytest.mark.parametrize("kind", R.KINDS)
def test_one_statement_three_callers(A, ctx, kind):
    """The rules' three callers on the float32 grid, BITWISE: the sweep's per-point kernel (agpl_cavi_pass_plan: c_out, gamma_out,
    beta_out) and agpl_cavi_pass's element-wise kernel, each against the float32 array-fed operators applied to that route's own
    marginals (agpl_marginals_plan / agpl_marginals).  One plan per parameter set and class: N <= 64, M = 256, one feature column of
    2^-10, mu0 = the grid's mu (a fresh q(v) is N(0, I), so mu = mu0), resid = ONE var per point (the latents of a point share the
    features: lik_rules_reference.plan_points); the points whose gamma or beta the model expects negative or non-finite go into
    plans of their own (a pass alone raises nothing: the update behind it reports them, test_domain_report_names_the_point).  No
    grid point is left out: PLAN_POINTS is asserted.  Which holds: the two routes' marginals are bitwise equal to each other as well
    (asserted), so the equalities below are between all three callers on the same numbers.
    elbo_terms_out of the plan's pass (elbo_point in the per-point kernel: the one-logcosh shortcut for Bernoulli and the negative
    binomial) against the sum of the n = 1 float64 terms of the operators from the same float32 marginals, to n 2^-53 sum |term|,
    |term| = |expected_logtilt_i| + |aux_kldivergence_i|; where a term is not finite the two must be in the same class."""
    counts = [0, 0]
    for params, pts in R.groups(R.grid(kind, R.F32)):
        lik = make_lik(A, kind, params)
        L = lik._nlatent
        for cls, sub in enumerate(R.plan_points(kind, params, pts)):
            counts[cls] += len(sub)
            if not sub:
                continue
            n, names = len(sub), [p.name for p in sub]
            Phi = torch.zeros((n, 256), dtype=torch.float32, device="cuda")
            Phi[:, 0] = 2.0 ** -10
            resid = _dev([p.var[0] for p in sub], torch.float32)
            mu0 = _dev(np.asarray([p.mu for p in sub], np.float64).T, torch.float32)
            yd = _y_dev(lik, [list(p.y) for p in sub], torch.float32)
            tag = (kind, params, "finite" if cls == 0 else "other classes")
            # ---- the sweep's per-point kernel
            elbo = kind in HAS_ELBO
            pctx = ctx if cls == 0 else A.Context(0, seed=1)  # (the unreported domain flag of such a pass stays with its own context)
            cavi = A.SparseCAVI(lik, Phi, resid, yd, mu0=mu0, ctx=pctx, keep_points=True, track_elbo=elbo)
            assert cavi.plan is not None
            mu, var = cavi.marginals()
            cavi.accumulate()
            torch.cuda.synchronize()
            assert torch.equal(mu, mu0), "a fresh plan's mean is mu0"
            _assert_same_bits(tag + ("plan",), names, cavi, *_operators_on(A, pctx, lik, yd, mu, var))
            if elbo:
                got = float(cavi._elbo_terms.item())
                want, mag, finite = _elbo_sum_of_item_two(A, pctx, lik, yd, mu, var)
                if finite:
                    bound = n * 2.0 ** -53 * mag
                    print(f"LIK_RULES_GPU elbo_terms_out {kind} {params} n={n}: |pass - sum of terms| / bound = {abs(got - want) / bound:.3g}")
                    assert abs(got - want) <= bound, (tag, got, want, bound)
                else:
                    assert R.classify(got) == R.classify(want), (tag, got, want)
            # ---- agpl_cavi_pass's element-wise kernel
            flat = A.SparseCAVI(lik, Phi, resid, yd, mu0=mu0, ctx=pctx, keep_points=True, marginal_precision="f32", accumulate_precision="f32")
            assert flat.plan is None
            mu2, var2 = flat.marginals()
            flat.accumulate()  # (raises nothing, for the plans of the other classes either: this route too reports in its update)
            torch.cuda.synchronize()
            assert np.array_equal(_bits(mu2), _bits(mu)) and np.array_equal(_bits(var2), _bits(var)), (tag, "the two routes' marginals differ")
            _assert_same_bits(tag + ("element-wise",), names, flat, *_operators_on(A, pctx, lik, yd, mu2, var2))
    print(f"LIK_RULES_GPU three callers {kind}: {counts[0]} finite points, {counts[1]} of other classes")
    assert tuple(counts) == PLAN_POINTS[kind] and sum(counts) == len(R.grid(kind, R.F32))


# likelihood -> (what is put at the index, the flat index it must be reported at as a function of (N, i))
def _poison(kind, y, mu0, Phi, kd, i):
    N = Phi.shape[0]
    if kind == "negbin":  # y + r < 0: a negative precision
        y[i] = -20
        return i
    if kind == "poisson":  # y + lambda q < 0
        y[i] = -40
        return i
    if kind == "studentt":
        y[i] = float("nan")
        return i
    if kind == "laplace":  # the grid's "mu=y=0,var=0": 1 / (2 beta 0)
        Phi[i, :] = 0.0
        kd[i] = 0.0
        y[i] = 0.0
        return i
    if kind == "cat":  # the grid's "all=-17": p0 rounds to 0 in float32
        Phi[i, :] = 0.0
        kd[i] = 0.0
        mu0[:, i] = -17.0
        return (mu0.shape[0] - 1) * N + i  # every latent's precision is +inf there; the report carries the largest flat index
    if kind == "hetero":  # the grid's "y-mu=2e19": psi overflows, the count rate and the second latent's precision with it
        y[i] = 2e19
        return N + i
    mu0[:, i] = float("nan")  # Bernoulli, bijective categorical: no observation is outside the rule's domain; a mean that is no number
    return (mu0.shape[0] - 1) * N + i


@pytest.mark.parametrize("kind", R.KINDS)
def test_domain_report_names_the_point(A, kind):
    """One out-of-domain point at a known index inside typical data (N = 5000, M = 256): the pass and the update behind it raise
    DomainError naming that flat index (latent * N + point; the largest one where several latents of the point offend), and the next pass on the same context with clean data succeeds.
    The out-of-domain point is a grid point where the float32 grid has one: Laplace "mu=y=0,var=0", categorical "all=-17",
    heteroscedastic "y-mu=2e19".  The negative binomial and the Poisson rule are in domain on their whole grid (counts are >= 0),
    so a negative count stands in: the only way to a negative precision.  Bernoulli, the bijective categorical and Student-t have NO
    out-of-domain input among finite numbers in float32: c = sqrt(.) >= 0 gives 0 <= gamma <= b / 4; the bijective p0 is at least
    1 - L / (L + theta_L / 2) > 0; the Student-t w = (nu + 1) / (2 out1) is 0 once the residual overflows (the grid's 2e19) and positive
    below that.  For these three a NaN (mean or observation) is the smallest thing the report can be asked about."""
    ctx = A.Context(0, seed=5)
    params = R.grid(kind, R.F32)[0].params
    if kind == "studentt":
        params = {"nu": 3.5, "sigma": 2.0}
    if kind == "laplace":
        params = {"beta": 1.3}
    lik = make_lik(A, kind, params)
    N, M, L, i = 5000, 256, lik._nlatent, 1234
    rng = np.random.default_rng(7)
    Phi = torch.from_numpy((rng.standard_normal((N, M)) * 0.05).astype(np.float32)).cuda()
    kd = torch.ones(N, device="cuda")
    mu0 = torch.zeros((L, N), device="cuda")
    if lik.ykind == "real":
        y = torch.from_numpy(rng.standard_normal(N).astype(np.float32)).cuda()
    elif lik.ykind == "i32":
        y = torch.from_numpy(rng.poisson(4.0, N).astype(np.int32)).cuda()
    elif L > 1 and kind != "hetero":
        lab = rng.integers(0, L + 1, N)
        y = torch.from_numpy((lab[:, None] == np.arange(L)[None, :]).astype(np.uint8)).cuda()
    else:
        y = torch.from_numpy((rng.uniform(size=N) < 0.5).astype(np.uint8)).cuda()
    clean = (Phi.clone(), kd.clone(), y.clone(), mu0.clone())
    flat = _poison(kind, y, mu0, Phi, kd, i)
    cavi = A.SparseCAVI(lik, Phi, kd, y, mu0=mu0, ctx=ctx)
    assert cavi.plan is not None
    with pytest.raises(A.DomainError, match=rf"flat index {flat}\b"):
        cavi.sweep()
        cavi.sweep()
        cavi.check()
    good = A.SparseCAVI(lik, clean[0], clean[1], clean[2], mu0=clean[3], ctx=ctx)
    good.sweep()
    good.sweep()
    good.check()
