"""GPU tests of posterior-predictive draws of y (include/agpl_sample_y.h: agpl_sample_y; csrc/agpl_sample_y.hip; operators.sample_y,
Paths.sample_y, Plan.sample_y, SparseCAVI.sample_y, SparseGibbs.sample_y):

* equality with tests/sample_y_reference.py for every kind (NegBinomial r = 0.7, 15; Poisson lambda = 3, 40; Student-t nu = 1.5, 10;
  L = 3 for both categorical links) at T = 3, Ns = 257, ldf = 300, point0 = 2^32 - 100, draw0 = 65534: integer and one-hot outputs
  equal, real outputs within 1e-12 relative; a draw may differ only where the reference's margin is below 1e-9, two per case at
  most (tests/test_sample_y_reference_cpu.py: there is no such draw);
* structure, bitwise: repeatability; a point alone, a window of draws, the context's point offset against point0; another seed,
  sweep or draw; Ns = 0, 1, 63, 64, 65 and T = 0; one element more than a single pass of the grid;
* sentinels for non-finite F, neighbours unchanged;
* sample mean and variance of 4096 draws at 64 points against operators.predictive, 5 Monte Carlo standard errors, the errors from
  the quadrature moments of the reference;
* end to end on a small trained model; argument errors, after which the context still works."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import sample_y_reference as R

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "augmentedgplikelihoods.jl_amd", "csrc")


@pytest.fixture(scope="module")
def A():
    import agpl_amd

    return agpl_amd


@pytest.fixture(scope="module")
def ctx(A):
    return A.Context(0, seed=R.SEED)


def host(t):
    return t.detach().cpu().numpy()


def dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    return t if dtype is None else t.to(dtype)


def lik_of(A, c):
    return {R.BERNOULLI: lambda: A.BernoulliLikelihood(), R.NEGBINOMIAL: lambda: A.NegativeBinomialLikelihood(c.p[0]),
            R.STUDENTT: lambda: A.StudentTLikelihood(*c.p), R.POISSON: lambda: A.PoissonLikelihood(c.p[0]),
            R.LAPLACE: lambda: A.LaplaceLikelihood(c.p[0]), R.HETEROGAUSS: lambda: A.HeteroscedasticGaussianLikelihood(c.p[0]),
            R.CATEGORICAL: lambda: A.CategoricalLikelihood(np.array(c.logtheta)),
            R.CATEGORICAL_BIJ: lambda: A.CategoricalLikelihood(np.array(c.logtheta), bijective=True)}[c.kind]()


def case(cid):
    return next(c for c in R.CASES if c.id == cid)


def raw_rc(ctx, lik, T, Ns, ldf, F, point0, draw0, sweep, out):
    """The C entry point's status."""
    from agpl_amd import _ffi

    d = lik.desc()
    ptr = lambda t: C.c_void_p(0 if t is None else t.data_ptr())
    return _ffi.sample_y_lib().agpl_sample_y(ctx.bind(), C.byref(d), C.c_int32(T), C.c_int64(Ns), C.c_int64(ldf), ptr(F), C.c_int64(point0),
                                             C.c_int32(draw0), C.c_uint32(sweep), ptr(out))


@pytest.mark.parametrize("c", R.CASES, ids=lambda c: c.id)
def test_equality_with_the_reference(A, ctx, oracle, c):
    F, ref, margin = R.case_reference(oracle, c)
    Fd = dev(F)
    y = A.sample_y(lik_of(A, c), Fd[:, :, : R.NS], point0=R.POINT0, draw0=R.DRAW0, sweep=R.SWEEP, ctx=ctx)  # in place: ldf = 300
    got = host(y)
    assert got.shape == ref.shape and got.dtype == ref.dtype
    if ref.dtype == np.float64:
        err = np.abs(got - ref) / np.abs(ref)
        print(f"{c.id}: max relative difference {err.max():.3e}")
        differ = ~(err <= 1e-12)
    else:
        differ = got != ref
        if differ.ndim == 3:
            differ = differ.any(-1)
        print(f"{c.id}: {differ.sum()} draws differ")
    assert differ.sum() <= 2 and (margin[differ] < 1e-9).all(), (differ.sum(), margin[differ])
    # the contiguous copy of the same block (ldf = Ns) gives the same bytes
    assert torch.equal(A.sample_y(lik_of(A, c), Fd[:, :, : R.NS].contiguous(), point0=R.POINT0, draw0=R.DRAW0, sweep=R.SWEEP, ctx=ctx), y)


@pytest.mark.parametrize("cid", ["bernoulli", "negbinomial-r15", "studentt-nu10", "categorical-bij"])
def test_structure_is_bitwise(A, cid):
    c = case(cid)
    lik, L = lik_of(A, c), R.nlatent(c)
    ctx = A.Context(0, seed=99)
    rng = np.random.default_rng(12)
    T, Ns, k = 5, 130, 2 ** 33 + 7
    F = dev(rng.uniform(-4, 4, size=(T, L, Ns)).astype(np.float32))
    S = lambda F_, **kw: A.sample_y(lik, F_, ctx=ctx, **{"sweep": 3, **kw})
    full = S(F, point0=k)
    assert torch.equal(S(F, point0=k), full)
    # a point alone, at its global index
    assert torch.equal(S(F[:, :, 77:78], point0=k + 77), full[:, 77:78])
    # draws [d, d + 2) of the T = 5 call are a T = 2 call with draw0 = d
    assert torch.equal(S(F[1:3], point0=k, draw0=1), full[1:3])
    # the context's point offset against point0
    ctx.set_point_offset(k)
    assert torch.equal(S(F), full)
    ctx.set_point_offset(0)
    # another seed, sweep or draw: other bytes
    assert not torch.equal(S(F, point0=k, sweep=4), full)
    assert not torch.equal(S(F, point0=k, draw0=1), full)
    assert not torch.equal(S(F, point0=k + 1), full)
    other = A.Context(0, seed=100)
    assert not torch.equal(A.sample_y(lik, F, point0=k, sweep=3, ctx=other), full)
    # Ns = 0, 1, 63, 64, 65 and T = 0
    for n in (0, 1, 63, 64, 65):
        sub = S(F[:, :, :n], point0=k)
        assert tuple(sub.shape)[:2] == (T, n) and torch.equal(sub, full[:, :n])
    assert tuple(S(F[:0], point0=k).shape)[:2] == (0, Ns)


def test_one_element_beyond_a_single_grid_pass(A, oracle):
    src = open(os.path.join(CSRC, "agpl_sample_y.hip")).read()
    blocks = int(re.search(r"^\s*constexpr\s+int\s+kSampleYMaxBlocks\s*=\s*(\d+)\s*;", src, flags=re.M).group(1))
    lanes = int(re.search(r"^\s*constexpr\s+int\s+kBlock\s*=\s*(\d+)\s*;", src, flags=re.M).group(1))
    T, Ns = 3, 174763
    assert T * Ns == 524289 == blocks * lanes + 1  # plain numbers: a constant that moves fails here
    c, lik = case("bernoulli"), A.BernoulliLikelihood()
    ctx = A.Context(0, seed=R.SEED)
    F = torch.empty((T, 1, Ns), dtype=torch.float32, device="cuda").uniform_(-4, 4, generator=torch.Generator(device="cuda").manual_seed(3))
    full = A.sample_y(lik, F, point0=10, draw0=4, sweep=2, ctx=ctx)
    assert set(torch.unique(full).tolist()) == {0, 1}
    # every piece of it alone: no piece is more than one pass
    cut = 100000
    assert torch.equal(A.sample_y(lik, F[:, :, :cut], point0=10, draw0=4, sweep=2, ctx=ctx), full[:, :cut])
    assert torch.equal(A.sample_y(lik, F[:, :, cut:], point0=10 + cut, draw0=4, sweep=2, ctx=ctx), full[:, cut:])
    assert torch.equal(A.sample_y(lik, F[2:], point0=10, draw0=6, sweep=2, ctx=ctx), full[2:])
    # the lanes' second element (the last one of the call) and its neighbours against the reference
    tail = host(F[2:, :, Ns - 4:])
    ref, _ = R.sample(oracle, c, tail, R.SEED, 10 + Ns - 4, 6, 2)
    assert np.array_equal(host(full[2:, Ns - 4:]), ref)


@pytest.mark.parametrize("cid", ["bernoulli", "poisson-40", "laplace", "heterogauss", "categorical"])
def test_non_finite_function_values_give_sentinels(A, ctx, cid):
    c = case(cid)
    lik, L = lik_of(A, c), R.nlatent(c)
    rng = np.random.default_rng(4)
    T, Ns = 3, 70
    F = dev(rng.uniform(-4, 4, size=(T, L, Ns)).astype(np.float32))
    good = A.sample_y(lik, F, sweep=5, ctx=ctx)
    Fb = F.clone()
    Fb[0, 0, 5], Fb[1, L - 1, 64], Fb[2, 0, 69] = float("nan"), float("inf"), float("-inf")
    y = A.sample_y(lik, Fb, sweep=5, ctx=ctx)
    bad = torch.zeros((T, Ns), dtype=torch.bool, device="cuda")
    bad[0, 5] = bad[1, 64] = bad[2, 69] = True
    assert torch.equal(y[~bad], good[~bad])
    if y.dtype == torch.float64:
        assert torch.isnan(y[bad]).all() and not torch.isnan(good).any()
    else:
        assert (y[bad] == (255 if y.dtype == torch.uint8 else -1)).all()


PRED_CASES = ["bernoulli", "negbinomial-r15", "poisson-40", "studentt-nu10", "laplace", "heterogauss", "categorical", "categorical-bij"]


@pytest.mark.parametrize("cid", PRED_CASES)
def test_moments_against_the_shipped_predictive(A, ctx, cid):
    c = case(cid)
    lik, L = lik_of(A, c), R.nlatent(c)
    rng = np.random.default_rng(21)
    Ns, T = 64, 4096
    mu, s = rng.uniform(-2, 2, size=(L, Ns)), rng.uniform(0.1, 1, size=(L, Ns))
    F = dev((mu[None] + s[None] * rng.standard_normal((T, L, Ns))).astype(np.float32))
    y = host(A.sample_y(lik, F, sweep=8, ctx=ctx)).astype(np.float64)
    qf = (dev(mu[0]), dev(s[0] ** 2)) if L == 1 else (dev(mu.T), dev(s.T ** 2))
    if c.kind in (R.CATEGORICAL, R.CATEGORICAL_BIJ):
        nmc = 1 << 20  # the predictive's own Monte Carlo: its error adds to the bar
        pr = host(A.predictive(lik, qf, nsamples=nmc, sweep=9, ctx=ctx)[0])  # [Ns, K]
        freq = y.mean(0)
        if c.kind == R.CATEGORICAL_BIJ:
            freq = np.concatenate([freq, 1.0 - freq.sum(-1, keepdims=True)], axis=-1)
        err, bar = np.abs(freq - pr), 5 * np.sqrt(pr * (1 - pr) * (1.0 / T + 1.0 / nmc))
        print(f"{cid}: class frequencies: max err / bar {np.max(err / bar):.3f}")
        assert (err <= bar).all()
        return
    mean, var, _ = (None if t is None else host(t) for t in A.predictive(lik, qf, ctx=ctx))
    mom = np.array([R.marginal_moments(c, mu[0, i], s[0, i], mu[-1, i], s[-1, i]) for i in range(Ns)])
    # (the quadrature and the shipped predictive state the same moments)
    print(f"{cid}: quadrature against predictive: mean {np.max(np.abs(mom[:, 0] - mean)):.2e}, variance (relative) "
          f"{np.max(np.abs(mom[:, 1] / var - 1)):.2e}")
    assert np.allclose(mom[:, 0], mean, rtol=1e-4, atol=1e-6) and np.allclose(mom[:, 1], var, rtol=1e-4)
    em, bm = np.abs(y.mean(0) - mean), 5 * np.sqrt(mom[:, 1] / T)
    ev, bv = np.abs(y.var(0, ddof=1) - var), 5 * np.sqrt((mom[:, 2] - mom[:, 1] ** 2) / T)
    print(f"{cid}: mean: max err / bar {np.max(em / bm):.3f}; variance: max err / bar {np.max(ev / bv):.3f}")
    assert (em <= bm).all() and (ev <= bv).all()


def _trained(A, ctx):
    rng = np.random.default_rng(41)
    N, M = 2000, 32
    x = rng.uniform(-3, 3, size=(N, 1))
    y = (rng.uniform(size=N) < 1 / (1 + np.exp(-2 * np.sin(2 * x[:, 0])))).astype(np.uint8)
    z = np.linspace(-3, 3, M)[:, None]
    cavi = A.SparseCAVI.from_inputs(A.BernoulliLikelihood(), dev(x), dev(y), dev(z), 0.3, variance=1.5, jitter=1e-6, ctx=ctx)
    cavi.run(10)
    return cavi, x, y, z


def test_end_to_end_on_a_trained_model(A):
    ctx = A.Context(0, seed=5)
    cavi, x, y, z = _trained(A, ctx)
    lik = cavi.lik
    xs = dev(np.linspace(-2.9, 2.9, 257)[:, None] + 0.013)
    gen = lambda: torch.Generator(device="cuda").manual_seed(2024)
    for method in ("paths", "joint"):
        ys = cavi.sample_y(xs[:9], 6, method=method, nfeatures=128, generator=gen())
        assert tuple(ys.shape) == (6, 9) and ys.dtype == torch.uint8 and set(torch.unique(ys).tolist()) <= {0, 1}
    with pytest.raises(A.ArgumentError):
        cavi.sample_y(xs[:9], 6, method="exact")
    gib = A.SparseGibbs.from_inputs(lik, dev(x[:300]), dev(y[:300]), dev(z[::2]), 0.6, jitter=1e-6, ctx=ctx)
    chain = gib.run(4)
    yg = gib.sample_y(xs[:9], chain, nfeatures=100, generator=gen())
    assert tuple(yg.shape) == (4, 9) and yg.dtype == torch.uint8 and set(torch.unique(yg).tolist()) <= {0, 1}
    # Paths.sample_y over chunk seams is one sample_y call on the full block of function values
    paths = cavi.sample_paths(7, nfeatures=128, generator=gen())
    paths._Y_CHUNK = 100  # 257 points: chunks of 100, 100, 57
    chunked = paths.sample_y(lik, xs, sweep=31)
    assert tuple(chunked.shape) == (7, 257)
    assert torch.equal(chunked, A.sample_y(lik, paths(xs), sweep=31, ctx=ctx))
    del paths._Y_CHUNK
    assert torch.equal(paths.sample_y(lik, xs, sweep=31), chunked)
    # the mean of y over the paths against predict_y, 5 Monte Carlo standard errors (from predict_y's probability)
    T = 4096
    ym = host(cavi.sample_y(xs[::32], T, nfeatures=2048, generator=gen())).astype(np.float64).mean(0)
    p = host(cavi.predict_y(xs[::32])[0])
    err, bar = np.abs(ym - p), 5 * np.sqrt(p * (1 - p) / T)
    print(f"mean of y over {T} paths against predict_y: max err / bar {np.max(err / bar):.3f}")
    assert (err <= bar).all()
    # a multi-latent likelihood through a plan: one-hot rows
    lik3 = A.CategoricalLikelihood(np.array([0.3, -0.2, 0.5]))
    plan = A.Plan.from_inputs(dev(x[:500]), dev(z), 0.3, L=3, ctx=ctx)
    yc = plan.sample_y(lik3, xs[:9], 5, nfeatures=64, generator=gen())
    assert tuple(yc.shape) == (5, 9, 3) and yc.dtype == torch.uint8 and (yc.sum(-1) == 1).all()
    with pytest.raises(A.ArgumentError):
        plan.sample_y(lik, xs[:9], 5)


def test_errors_leave_the_context_usable(A, ctx):
    from agpl_amd import _ffi

    lik = A.BernoulliLikelihood()
    F = dev(np.random.default_rng(1).uniform(-4, 4, size=(2, 1, 10)).astype(np.float32))
    good = A.sample_y(lik, F, sweep=1, ctx=ctx)
    out = torch.full((2, 10), 7, dtype=torch.uint8, device="cuda")
    rc = lambda lk=lik, T=2, Ns=10, ldf=10, Fv=F, draw0=0, oo=out: raw_rc(ctx, lk, T, Ns, ldf, Fv, 0, draw0, 1, oo)
    for kw in (dict(T=-1), dict(Ns=-1), dict(ldf=9), dict(Fv=None), dict(oo=None), dict(draw0=-1), dict(draw0=2 ** 24 - 3),
               dict(lk=A.NegativeBinomialLikelihood(0.0)), dict(lk=A.StudentTLikelihood(3.0, 0.0)), dict(lk=A.PoissonLikelihood(-1.0)),
               dict(lk=A.LaplaceLikelihood(float("nan")))):
        assert rc(**kw) == _ffi.ERR_INVALID_ARGUMENT, kw
    assert rc(T=0) == _ffi.AGPL_OK and rc(Ns=0, ldf=0) == _ffi.AGPL_OK and rc(T=0, Fv=None, oo=None) == _ffi.AGPL_OK
    ctx.synchronize()
    assert (out == 7).all()
    assert rc(draw0=2 ** 24 - 4) == _ffi.AGPL_OK  # the last draw index there is
    with pytest.raises(A.ArgumentError):
        A.sample_y(lik, F[:, 0, :].reshape(2, 2, 5), ctx=ctx)
    with pytest.raises(A.ArgumentError):
        A.sample_y(lik, F, draw0=-1, ctx=ctx)
    # float64 function values (sample_f's) are cast to float32: the same draws
    assert torch.equal(A.sample_y(lik, F.to(torch.float64), sweep=1, ctx=ctx), good)
    # sweep = None takes the context's next draw counter
    s0 = ctx.sweep
    assert torch.equal(A.sample_y(lik, F, ctx=ctx), A.sample_y(lik, F, sweep=s0, ctx=ctx)) and ctx.sweep == s0 + 1
