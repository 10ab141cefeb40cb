"""GPU tests of the binomial likelihood with per-point trial counts (AGPL_LIK_BINOMIAL_N = 11; run with -m gpu on an MI355X).
The kind is tied to kind 8 (one n for the data set), which tests/binomial_reference.py and the oracle already hold: with a
constant n, and at the points of each n of a mixed set, every per-point output equals kind 8's bit for bit; the sums over
points equal kind 8's on the same points.  Beyond that: the expansion into Bernoulli rows and ten sweeps against the float64
restatement tests/binomial_n_reference.py.

Bars: m, S, G, g of the expansion within the 1e-5 of max|ref| that tests/test_gpu_binomial.py asks of Bernoulli against
Binomial(1) (its NAT_TOL); natural parameters after ten sweeps within the same file's 1e-5; the two shards' G, g within the 1e-5
of tests/test_gpu_distributed.py.  Everything else is equality of bytes.

Not here: quantiles and draws of y for the kind.  agpl_predictive_quantile and agpl_sample_y have no argument for the trials
and refuse the kind (test 6); siblings that take one are left out of this change."""
import ctypes as C
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import binomial_n_reference as R  # noqa: E402

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

SEED = 20261021
N = 777
SPLIT = 401  # an odd index: the two-way split of the points
NS = (1, 2, 7, 1000)
MIXED = (1, 2, 7, 64, 65, 1000)
NAT_TOL = 1e-5


@pytest.fixture(scope="module")
def A():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import __graft_entry__ as g

    g.build()
    import agpl_amd

    return agpl_amd


def dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    return t if dtype is None else t.to(dtype)


def host(t):
    return t.detach().cpu().numpy()


def relmax(a, b):
    return np.abs(np.asarray(a) - np.asarray(b)).max() / max(np.abs(np.asarray(b)).max(), 1e-300)


def same(a, b):
    """Equality of bytes (NaN equals NaN, -inf equals -inf)."""
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def mixed_counts(rng, size, values=MIXED):
    """n_i from ``values`` and y_i uniform on 0 .. n_i, with y = 0 and y = n_i at every n (the first points)."""
    trials = rng.choice(values, size=size).astype(np.int32)
    trials[:2 * len(values)] = np.repeat(values, 2)
    y = rng.integers(0, trials + 1).astype(np.int32)
    y[:2 * len(values):2] = 0
    y[1:2 * len(values):2] = trials[1:2 * len(values):2]
    return y, trials


def obs(y, trials):
    return np.ascontiguousarray(np.stack([y, trials], axis=1).astype(np.int32))


@pytest.fixture(scope="module")
def inputs():
    """One set of latents and marginals for the elementwise tests, made once and left unchanged."""
    rng = np.random.default_rng(SEED)
    return dict(f=rng.normal(size=N) * 2.0, mu=rng.normal(size=N) * 1.5, var=rng.uniform(0.05, 2.0, size=N))


def per_point(A, lik, y, inp, offset=0, lo=0, hi=N):
    """Every per-point output of the entry points that take the descriptor, as host arrays, on points lo .. hi of ``inp``."""
    ctx = A.Context(0, seed=SEED)
    ctx.set_point_offset(offset + lo)
    f, mu, var = (dev(inp[k][lo:hi]) for k in ("f", "mu", "var"))
    yd = dev(y)
    out = {}
    Om, nuni, nterms = A.aux_sample_(A.init_aux_variables(lik, hi - lo, ctx=ctx), lik, yd, f, ctx=ctx, sweep=5, stats=True)
    out["omega"], out["nuni"], out["nterms"] = host(Om.ω), host(nuni), host(nterms)
    beta, gamma = A.auglik_potential_and_precision(lik, Om, yd, ctx=ctx)
    out["s_beta"], out["s_gamma"] = host(beta[0]), host(gamma[0])
    for dt, tag in ((torch.float64, "64"), (torch.float32, "32")):
        q = A.aux_posterior(lik, yd, (mu.to(dt), var.to(dt)), ctx=ctx)
        out["c" + tag] = host(q.inds[0]["c"])
        bt, gm = A.expected_auglik_potential_and_precision(lik, q, yd, ctx=ctx)
        out["e_beta" + tag], out["e_gamma" + tag] = host(bt[0]), host(gm[0])
    me, va, lp = A.predictive(lik, (mu, var), yd, ctx=ctx)
    out["mean"], out["var"], out["logp"] = host(me), host(va), host(lp)
    cdf, sf = A.predictive_cdf(lik, (mu, var), yd, ctx=ctx)
    out["cdf"], out["sf"] = host(cdf), host(sf)
    out["ell"] = host(A.expected_loglik(lik, mu, var, yd, ctx=ctx, per_point=True, grad=False)[2])
    ctx.synchronize()
    return out


def sums(A, lik, y, omega, inp, idx):
    """The reductions over the points ``idx``: logtilt, aug_loglik, the prior density, expected_logtilt, expected_aug_loglik, KL."""
    ctx = A.Context(0, seed=SEED)
    f, mu, var = (dev(inp[k][idx]) for k in ("f", "mu", "var"))
    yd, Om = dev(y[idx]), A.TupleVector(ω=dev(omega[idx]))
    q = A.aux_posterior(lik, yd, (mu, var), ctx=ctx)
    return [A.logtilt(lik, Om, yd, f, ctx=ctx), A.aug_loglik(lik, Om, yd, f, ctx=ctx), A.aux_prior_logpdf(lik, Om, yd, ctx=ctx),
            A.expected_logtilt(lik, q, yd, (mu, var), ctx=ctx), A.expected_aug_loglik(lik, q, yd, (mu, var), ctx=ctx),
            A.aux_kldivergence(lik, q, yd, ctx=ctx)]


def sparse_problem(M, seed=3, values=MIXED):
    rng = np.random.default_rng([seed, M])
    Phi = (rng.normal(size=(N, M)) / math.sqrt(M)).astype(np.float32)
    # one largest entry, the same in both halves of the split: the shards' images then share the scale of the whole (the reason
    # is stated in tests/test_gpu_binomial.py's sparse_problem)
    assert np.abs(Phi).max() < 0.75
    Phi[0, 0] = Phi[SPLIT, 0] = 0.75
    kd = rng.uniform(0.05, 0.3, size=N).astype(np.float32)
    y, trials = mixed_counts(rng, N, values)
    return Phi, kd, y, trials


# ------------------------------------------------------------------------------------------ 1. accepted where it was refused
def test_the_operators_accept_the_kind(A, inputs):
    """Each call raised ArgumentError (AGPL_ERR_INVALID_ARGUMENT, unknown likelihood kind 11) before the kind existed."""
    rng = np.random.default_rng(1)
    y, trials = mixed_counts(rng, N)
    lik = A.BinomialTrialsLikelihood()
    ctx = A.Context(0, seed=SEED)
    yd = A.binomial_obs(dev(y), dev(trials))
    assert same(host(yd), obs(y, trials))
    q = A.aux_posterior(lik, yd, (dev(inputs["mu"]), dev(inputs["var"])), ctx=ctx)
    beta, gamma = A.expected_auglik_potential_and_precision(lik, q, yd, ctx=ctx)
    beta, gamma = host(beta[0]), host(gamma[0])
    assert np.isfinite(beta).all() and np.isfinite(gamma).all() and (gamma > 0).all()
    assert same(beta, y - trials / 2.0)
    out = per_point(A, lik, obs(y, trials), inputs)
    assert all(np.isfinite(v).all() for v in out.values())


# ------------------------------------------------------------------------------------------ 2. constant n is kind 8
@pytest.mark.parametrize("n", NS)
def test_constant_trials_are_kind_8_bit_for_bit(A, inputs, n):
    rng = np.random.default_rng([2, n])
    y = rng.integers(0, n + 1, size=N).astype(np.int32)
    y[:2] = (0, n)
    trials = np.full(N, n, dtype=np.int32)
    l8, l11 = A.BinomialLikelihood(n), A.BinomialTrialsLikelihood()
    a, b = per_point(A, l8, y, inputs, offset=12345), per_point(A, l11, obs(y, trials), inputs, offset=12345)
    for k in a:
        assert same(a[k], b[k]), k
    idx = np.arange(N)
    assert sums(A, l8, y, a["omega"], inputs, idx) == sums(A, l11, obs(y, trials), a["omega"], inputs, idx)


@pytest.mark.parametrize("n", NS)
def test_constant_trials_sweep_as_kind_8(A, n):
    """One CAVI sweep and one Gibbs sweep on a plan: the same G, g, bit for bit."""
    Phi, kd, _, _ = sparse_problem(64)
    rng = np.random.default_rng([22, n])
    y = rng.integers(0, n + 1, size=N).astype(np.int32)
    trials = np.full(N, n, dtype=np.int32)
    res = []
    for lik, yy in ((A.BinomialLikelihood(n), y), (A.BinomialTrialsLikelihood(), obs(y, trials))):
        cavi = A.SparseCAVI(lik, dev(Phi), dev(kd), dev(yy), ctx=A.Context(0, seed=SEED), track_elbo=True)
        cavi.sweep()
        cavi.check()
        gctx = A.Context(0, seed=SEED)
        gib = A.SparseGibbs(lik, dev(Phi), dev(kd), dev(yy), ctx=gctx, keep_points=True)
        gib.sweep()
        gctx.synchronize()
        res.append([host(t) for t in (cavi.G, cavi.g, cavi.m, gib.G, gib.g, gib.omega, gib.f)])
    for u, v in zip(*res):
        assert same(u, v)


# ------------------------------------------------------------------------------------------ 3. mixed n is per-point kind 8
def test_mixed_trials_are_kind_8_at_the_points_of_each_n(A, inputs):
    rng = np.random.default_rng(3)
    y, trials = mixed_counts(rng, N)
    l11 = A.BinomialTrialsLikelihood()
    got = per_point(A, l11, obs(y, trials), inputs, offset=777)
    for n in MIXED:
        idx = np.nonzero(trials == n)[0]
        assert len(idx) > 20 and 0 in y[idx] and n in y[idx]
        l8 = A.BinomialLikelihood(n)
        ref = per_point(A, l8, np.minimum(y, n).astype(np.int32), inputs, offset=777)  # all points at this n, y clipped into range
        for k in got:
            assert same(got[k][idx], ref[k][idx]), (n, k)
        assert sums(A, l11, obs(y, trials), got["omega"], inputs, idx) == sums(A, l8, y, got["omega"], inputs, idx), n


# ------------------------------------------------------------------------------------------ 4. expansion into Bernoulli rows
def test_expansion_into_bernoulli_rows(A):
    """In exact arithmetic the two runs are the same: the rows of a point share mu and var, hence c, and n E PG(1, c) = E PG(n, c)."""
    N0, M = 300, 64
    rng = np.random.default_rng(4)
    trials = rng.integers(1, 6, size=N0).astype(np.int32)
    y = rng.integers(0, trials + 1).astype(np.int32)
    y[:2] = (0, trials[1])
    Phi = (rng.normal(size=(N0, M)) / math.sqrt(M)).astype(np.float32)
    kd = rng.uniform(0.05, 0.3, size=N0).astype(np.float32)
    y01, Phi_x, kd_x = R.expand(trials, y, Phi, kd)
    counts = A.SparseCAVI(A.BinomialTrialsLikelihood(), dev(Phi), dev(kd), dev(obs(y, trials)), ctx=A.Context(0, seed=SEED))
    rows = A.SparseCAVI(A.BernoulliLikelihood(), dev(Phi_x), dev(kd_x), dev(y01), ctx=A.Context(0, seed=SEED))
    counts.run(10)
    rows.run(10)
    for name in ("m", "S", "G", "g"):
        fig = relmax(host(getattr(counts, name)), host(getattr(rows, name)))
        print(f"BINOMIAL_N expansion: {name} relmax = {fig:.3e}")
        assert fig < NAT_TOL, (name, fig)


# ------------------------------------------------------------------------------------------ 5. ten sweeps against the restatement
@pytest.mark.parametrize("M", [64, 200])
def test_cavi_sweeps_against_the_restatement(A, M):
    Phi, kd, y, trials = sparse_problem(M)
    cavi = A.SparseCAVI(A.BinomialTrialsLikelihood(), dev(Phi), dev(kd), dev(obs(y, trials)), ctx=A.Context(0, seed=SEED), keep_points=True)
    Phi_d = host(cavi.plan.features()).astype(np.float64)  # what the plan's images hold
    ref = R.cavi_sweeps(trials, Phi_d, host(cavi.plan.resid).astype(np.float64), y, 10)
    for it in range(10):
        cavi.sweep()
        if it in (0, 9):
            fG, fg = relmax(host(cavi.G)[0], ref["G"][it]), relmax(host(cavi.g)[0], ref["g"][it])
            print(f"BINOMIAL_N sweeps M = {M}, sweep {it}: G {fG:.3e}, g {fg:.3e}")
            assert fG < NAT_TOL and fg < NAT_TOL
    cavi.check()
    assert np.isfinite(cavi.elbo())
    loo = cavi.loo()
    assert np.isfinite(loo.elpd) and loo.n_bad == 0
    me, va = cavi.loo_predict_y()  # the training trials come from the stored y
    frac = host(me) / trials
    assert ((frac > 0) & (frac < 1)).all() and (host(va) > 0).all()
    cdf, sf = cavi.loo_cdf()
    assert ((host(cdf) >= 0) & (host(cdf) <= 1)).all() and ((host(sf) >= 0) & (host(sf) <= 1)).all()


# ------------------------------------------------------------------------------------------ 6. edges
def test_edges(A, inputs):
    from agpl_amd import _ffi
    from agpl_amd import operators as ops

    rng = np.random.default_rng(6)
    y, trials = mixed_counts(rng, N)
    lik = A.BinomialTrialsLikelihood()
    base = per_point(A, lik, obs(y, trials), inputs)
    ctx = A.Context(0, seed=SEED)
    mu, var, f = (dev(inputs[k]) for k in ("mu", "var", "f"))
    # a count outside 0 .. n_i: -inf log densities at that point, no error
    for bad in (-1, int(trials[5]) + 1):
        yb = y.copy()
        yb[5] = bad
        yd = dev(obs(yb, trials))
        Om = A.TupleVector(ω=dev(base["omega"]))
        assert A.logtilt(lik, Om, yd, f, ctx=ctx) == -math.inf and A.aug_loglik(lik, Om, yd, f, ctx=ctx) == -math.inf
        lp = host(A.predictive(lik, (mu, var), yd, ctx=ctx)[2])
        assert lp[5] == -math.inf and same(np.delete(lp, 5), np.delete(base["logp"], 5))
        assert host(A.expected_loglik(lik, mu, var, yd, ctx=ctx, per_point=True, grad=False)[2])[5] == -math.inf
    # trials outside 1 <= n < 2^22: NaN at that point, its neighbours untouched, no error
    for bad in (0, 2 ** 22):
        tb = trials.copy()
        tb[7] = bad
        yd = dev(obs(y, tb))
        q = A.aux_posterior(lik, yd, (mu, var), ctx=ctx)
        bt, gm = A.expected_auglik_potential_and_precision(lik, q, yd, ctx=ctx)
        sb, sg = A.auglik_potential_and_precision(lik, A.TupleVector(ω=dev(base["omega"])), yd, ctx=ctx)
        me, va, lp = A.predictive(lik, (mu, var), yd, ctx=ctx)
        cdf, sf = A.predictive_cdf(lik, (mu, var), yd, ctx=ctx)
        ell = A.expected_loglik(lik, mu, var, yd, ctx=ctx, per_point=True, grad=False)[2]
        for got, key in ((bt[0], "e_beta64"), (gm[0], "e_gamma64"), (sb[0], "s_beta"), (me, "mean"), (va, "var"), (lp, "logp"), (cdf, "cdf"),
                         (sf, "sf"), (ell, "ell")):
            got = host(got)
            assert np.isnan(got[7]), (bad, key)
            assert same(np.delete(got, 7), np.delete(base[key], 7)), (bad, key)
    # the samplers: n_i >= 2^22 is outside the numbering of a point's draws, as any oversized b
    tb = trials.copy()
    tb[7] = 2 ** 22
    with pytest.raises(A.AGPLError) as err:
        A.aux_sample(lik, dev(obs(y, tb)), f, ctx=ctx, sweep=5)
    assert err.value.code == -3  # AGPL_ERR_UNSUPPORTED
    # n_i < 1 in a sampler: NaN at that point (the engine's answer to b < 0), no error, the neighbours' draws untouched
    tb[7] = 0
    om = host(A.aux_sample(lik, dev(obs(y, tb)), f, ctx=ctx, sweep=5).ω)
    assert np.isnan(om[7]) and same(np.delete(om, 7), np.delete(base["omega"], 7))
    # the entry points without the trials
    yd = dev(obs(y, trials))
    with pytest.raises(A.ArgumentError, match="may not be NULL"):
        A.predictive(lik, (mu, var), None, ctx=ctx)
    with pytest.raises(A.ArgumentError, match="agpl_predictive_quantile has no argument"):
        A.predictive_quantile(lik, (mu, var), (0.5,), ctx=ctx)
    with pytest.raises(A.ArgumentError, match="agpl_sample_y has no argument"):
        A.sample_y(lik, f.to(torch.float32).reshape(1, 1, N), sweep=1, ctx=ctx)
    d, h = lik.desc(), ctx.bind()  # dell_out given: refused, as for kinds 0 and 8
    sink = torch.empty(N, dtype=torch.float64, device="cuda")
    ptr = lambda t: C.c_void_p(t.data_ptr())
    rc = _ffi.likgrad_lib().agpl_expected_loglik(h, C.byref(d), C.c_int64(N), ptr(mu), ptr(var), ptr(yd), None, ptr(sink), None, None)
    with pytest.raises(A.ArgumentError, match="no learnable parameter"):
        _ffi.check(h, rc)
    # moments alone: column 0 is not read
    junk = obs(np.full(N, -12345, dtype=np.int32), trials)
    me, va, lp, _ = ops._predictive(lik, (mu, var), dev(junk), 0, None, ctx, want_logp=False)
    assert lp is None and same(host(me), base["mean"]) and same(host(va), base["var"])


# ------------------------------------------------------------------------------------------ 7. shards
def test_two_shards_reproduce_the_whole(A, inputs):
    rng = np.random.default_rng(7)
    y, trials = mixed_counts(rng, N)
    lik = A.BinomialTrialsLikelihood()
    whole = per_point(A, lik, obs(y, trials), inputs)
    for lo, hi in ((0, SPLIT), (SPLIT, N)):
        part = per_point(A, lik, obs(y[lo:hi], trials[lo:hi]), inputs, lo=lo, hi=hi)
        for k in whole:
            assert same(part[k], whole[k][lo:hi]), (lo, k)
    Phi, kd, y, trials = sparse_problem(64, seed=8)
    gib = A.SparseGibbs(lik, dev(Phi), dev(kd), dev(obs(y, trials)), ctx=A.Context(0, seed=777), keep_points=True)
    gib.sweep()
    om, f = host(gib.omega)[:, 0], host(gib.f)[:, 0]
    G, g = host(gib.G).copy(), host(gib.g).copy()
    Gs, gs = np.zeros_like(G), np.zeros_like(g)
    for lo, hi in ((0, SPLIT), (SPLIT, N)):
        part = A.SparseGibbs(lik, dev(Phi[lo:hi]), dev(kd[lo:hi]), dev(obs(y[lo:hi], trials[lo:hi])), ctx=A.Context(0, seed=777),
                             keep_points=True, point_offset=lo)
        part.sweep()
        assert same(host(part.omega)[:, 0], om[lo:hi]) and same(host(part.f)[:, 0], f[lo:hi])
        Gs += host(part.G)
        gs += host(part.g)
    assert relmax(Gs, G) < 1e-5 and relmax(gs, g) < 1e-5


# ------------------------------------------------------------------------------------------ 8. drivers
def test_drivers_from_inputs(A):
    rng = np.random.default_rng(8)
    n0, M = 500, 20  # (inducing inputs a lengthscale apart: K_ZZ stays well conditioned)
    x = np.sort(rng.uniform(-10, 10, size=n0))
    trials = rng.choice(MIXED, size=n0).astype(np.int32)
    y = rng.binomial(trials, 1 / (1 + np.exp(-2 * np.sin(0.7 * x)))).astype(np.int32)
    z = np.linspace(-10, 10, M)
    lik = A.BinomialTrialsLikelihood()
    ctx = A.Context(0, seed=SEED)
    cavi = A.SparseCAVI.from_inputs(lik, dev(x), A.binomial_obs(dev(y), dev(trials)), dev(z), 1.0, ctx=ctx, keep_points=True)
    cavi.run(10)
    xs = np.linspace(-9, 9, 101)
    ts = rng.choice(MIXED, size=101).astype(np.int32)
    ys = rng.binomial(ts, 0.5).astype(np.int32)
    mean, var, logp = cavi.predict_y(dev(xs), trials=dev(ts))
    assert logp is None
    frac = host(mean) / ts
    assert ((frac > 0) & (frac < 1)).all() and (host(var) > 0).all()
    # against the operator on the same arrays
    qf = cavi.plan._qf_at(dev(xs))
    me2, va2, lp2 = A.predictive(lik, qf, dev(obs(ys, ts)), ctx=ctx)
    assert same(host(me2), host(mean)) and same(host(va2), host(var))
    _, _, lp = cavi.predict_y(dev(xs), dev(ys), trials=dev(ts))
    assert same(host(lp), host(lp2))
    assert cavi.heldout_logp(dev(xs), dev(ys), trials=dev(ts)) == pytest.approx(host(lp2).sum(), rel=1e-12)
    cdf, sf = cavi.predict_cdf(dev(xs), dev(ys), trials=dev(ts))
    c2, s2 = A.predictive_cdf(lik, qf, dev(obs(ys, ts)), ctx=ctx)
    assert same(host(cdf), host(c2)) and same(host(sf), host(s2))
    with pytest.raises(A.ArgumentError, match="needs trials="):
        cavi.predict_y(dev(xs))
    with pytest.raises(A.ArgumentError, match="has no argument"):
        cavi.predict_quantiles(dev(xs))
    with pytest.raises(A.ArgumentError, match="has no argument"):
        cavi.sample_y(dev(xs), 2)
    ell, grad = cavi.expected_loglik()
    mu, v = cavi.marginals()
    ell2 = A.expected_loglik(lik, mu[0].to(torch.float64), v[0].to(torch.float64), cavi.y, ctx=ctx, grad=False)[0]
    assert ell == pytest.approx(ell2, rel=1e-12) and (grad is None or grad.numel() == 0)
    assert np.isfinite(cavi.loo().elpd)
    with pytest.raises(A.ArgumentError):
        A.learn_likelihood(cavi)
    other = A.SparseCAVI.from_inputs(A.BinomialLikelihood(7), dev(x), dev(np.minimum(y, 7)), dev(z), 1.0, ctx=ctx)
    with pytest.raises(A.ArgumentError, match="trials= is for"):
        other.predict_y(dev(xs), trials=dev(ts))
    gib = A.SparseGibbs.from_inputs(lik, dev(x), dev(obs(y, trials)), dev(z), 1.0, ctx=A.Context(0, seed=SEED))
    chain = gib.run(4)
    gm, gv, _ = gib.predict_y(dev(xs), chain, trials=dev(ts))
    gfrac = host(gm) / ts
    assert ((gfrac > 0) & (gfrac < 1)).all() and (host(gv) > 0).all()
    K = np.exp(-0.5 * (np.subtract.outer(np.arange(64.0), np.arange(64.0)) / 8.0) ** 2) + 1e-6 * np.eye(64)
    dg = A.DenseGibbs(lik, dev(K), dev(obs(y[:64], trials[:64])), ctx=ctx)
    dg.sweep()
    ctx.synchronize()
    assert np.isfinite(host(dg.f)).all()
