"""GPU tests of the joint posterior at new inputs (include/agpl_joint.h: agpl_plan_predict_cov; csrc/agpl_joint.hip;
Plan.predict_cov / sample_f, SparseCAVI.predict_cov / sample_f):

* tight tier: against the float64 formula fed the device's own features (``features()`` of a second plan at the test inputs) and the
  device's own U, element-wise within the bars tests/joint_reference.py derives (tests/test_joint_reference_cpu.py shows that those
  bars tell a wrong kernel from a right one);  loose tier: against all-float64 numpy, 2e-5 of max |Cov|;
* the diagonal against ``predict``'s var; a fresh plan gives the prior covariance; the plan's own training inputs;
* the symmetric form: symmetric bit for bit, i >= j bit for bit the general call's, positive semi-definite to rounding;
* position independence: blocks, the 65536-point chunk seam on either side, calls interleaved with predict / predict_chain;
* ld, empty sets, non-finite inputs, every argument error; sample_f against numpy's Cholesky factor.

The q(v) of every case comes from agpl_plan_update on random natural parameters (U != I, different per latent).
"""
import ctypes as C

import numpy as np
import pytest

import joint_reference as R

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

CHUNK = 1 << 16


@pytest.fixture(scope="module")
def A():
    import agpl_amd

    return agpl_amd


def host(t):
    return t.detach().cpu().numpy()


def dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    return t if dtype is None else t.to(dtype)


def ptr(t):
    return C.c_void_p(0 if t is None else t.data_ptr())


def kernel_arg(kind):
    return ("rq", R.ALPHA) if kind == "rq" else kind


@pytest.fixture(scope="module")
def world(A):
    """One context; per case the plan (q(v) from agpl_plan_update on the case's natural parameters), its data and its U -- built once."""
    ctx = A.Context(0, seed=13)
    made = {}

    def setup(c, fresh=False):
        key = (c, fresh)
        if key not in made:
            d = R.case_data(c, fresh)
            plan = A.Plan.from_inputs(dev(d.x), dev(d.z), d.ell, variance=d.s2, jitter=R.JITTER, L=c.L, ctx=ctx, kernel=kernel_arg(c.kind))
            Gd, gd = dev(d.G), dev(d.g)  # named: both must outlive the call that reads them
            if not fresh:
                plan.call("agpl_plan_update", ptr(Gd), ptr(gd), C.c_void_p(0), C.c_void_p(0))
            ctx.synchronize()
            U = np.stack([np.tril(host(plan.U_colmajor)[l].T[: c.M, : c.M]) for l in range(c.L)])  # U[a][b], b <= a
            assert plan.scale_exp == R.plan_scale_exp(d.s2)
            made[key] = (plan, d, U)
        return made[key]

    def features(c, d, x):
        """The features the call uses at x: those of a second plan built at x with the same z and hyperparameters (per-point determinism)."""
        p2 = A.Plan.from_inputs(dev(x), dev(d.z), d.ell, variance=d.s2, jitter=R.JITTER, ctx=ctx, kernel=kernel_arg(c.kind))
        F = host(p2.features()).astype(np.float64)
        ctx.synchronize()
        return F

    return ctx, setup, features


def raw_cov(plan, xa, Na, xb, Nb, out, ld):
    """The C entry point itself: (status, message)."""
    from agpl_amd import _ffi

    plan.ctx.bind()
    rc = _ffi.joint_lib().agpl_plan_predict_cov(plan._h, Na, ptr(xa), Nb, ptr(xb), ptr(out), ld)
    msg = _ffi.lib().agpl_last_error(plan.ctx._h)
    return rc, (msg.decode() if msg else "")


def check_tight(tag, cov, ref, bars):
    err = np.abs(cov.astype(np.float64) - ref)
    print(f"{tag}: max err {err.max():.3e}, max err / bar {np.max(err / bars):.3f}, max |ref| {np.abs(ref).max():.3f}")
    assert (err <= bars).all(), (tag, np.max(err / bars))


@pytest.mark.parametrize("c", R.TIGHT, ids=[c.id for c in R.TIGHT])
def test_against_float64_tight_and_loose(world, c):
    ctx, setup, features = world
    plan, d, U = setup(c)
    Mp = R.plan_padded(c.M)
    xa, xb = dev(d.xa), None if c.sym else dev(d.xb)
    cov_t = plan.predict_cov(xa, xb)
    ctx.synchronize()
    assert cov_t.shape == (c.L, c.Na, c.Nb) and cov_t.dtype == torch.float32
    cov = host(cov_t)
    Fa = features(c, d, d.xa)
    Fb = Fa if c.sym else features(c, d, d.xb)
    W = R.w_of_u(U)
    r2 = R.scaled_sqdist(d.xa, d.xb, d.ell)
    K = d.s2 * R.kappa(c.kind, r2)
    ref = R.reference(Fa, Fb, W, K)
    bars = R.bars(Fa, Fb, W, c.kind, r2, d.s2, Mp, plan.scale_exp)
    assert np.abs(ref - K[None]).max() > 1e-2 * np.abs(K).max()  # a q(v) far from the prior: the quadratic term is judged
    check_tight("tight", cov, ref, bars.total)
    # loose tier: everything in float64 numpy, the features too
    Pa = R.phi_f64(c.kind, d.xa, d.z, d.ell, d.s2)
    Pb = Pa if c.sym else R.phi_f64(c.kind, d.xb, d.z, d.ell, d.s2)
    ref64 = R.reference(Pa, Pb, W, K)
    err64 = np.abs(cov - ref64).max()
    print(f"loose: max err {err64:.3e} = {err64 / np.abs(ref64).max():.2e} of max |Cov|")
    assert err64 <= 2e-5 * np.abs(ref64).max()
    if not c.sym:
        return
    # the symmetric form
    assert torch.equal(cov_t, cov_t.transpose(1, 2))
    gen = plan.predict_cov(xa, xa.clone())
    low = torch.tril(torch.ones(c.Na, c.Na, dtype=torch.bool, device="cuda"))
    assert torch.equal(cov_t[:, low], gen[:, low])
    for l in range(c.L):
        lam = np.linalg.eigvalsh(cov[l].astype(np.float64)).min()
        slack = bars.total[l].sum(1).max()
        print(f"latent {l}: smallest eigenvalue {lam:.3e}, -(largest row sum of the bars) {-slack:.3e}")
        assert lam >= -slack
    # the diagonal is predict's var
    mu, var = plan.predict(xa)
    diag = np.stack([np.diag(cov[l]) for l in range(c.L)]).astype(np.float64)
    dbar = np.stack([np.diag(bars.total[l]) for l in range(c.L)]) + R.predict_var_bar(Fa, U, d.s2, Mp)
    derr = np.abs(diag - host(var).astype(np.float64))
    print(f"diagonal against predict: max err {derr.max():.3e}, max err / bar {np.max(derr / dbar):.3f}")
    assert (derr <= dbar).all()
    # the SparseCAVI-level forwarders are the plan's methods (checked on the plan: a driver only forwards)


def test_fresh_plan_gives_the_prior_covariance(world):
    ctx, setup, features = world
    c = R.FRESH
    plan, d, U = setup(c, fresh=True)
    assert np.array_equal(U[0], np.eye(c.M))
    cov = host(plan.predict_cov(dev(d.xa), dev(d.xb)))
    r2 = R.scaled_sqdist(d.xa, d.xb, d.ell)
    K = d.s2 * R.kappa(c.kind, r2)
    kbar = R.bars(np.zeros((c.Na, c.M)), np.zeros((c.Nb, c.M)), R.w_of_u(U), c.kind, r2, d.s2, R.plan_padded(c.M), plan.scale_exp).k
    check_tight("fresh", cov[0], K, kbar)


def test_training_inputs(world):
    ctx, setup, features = world
    c = R.TIGHT[6]  # M 64, L 3, D 2
    plan, d, U = setup(c)
    n = R.N_TRAIN
    F = host(plan.features()).astype(np.float64)  # the plan's own features: those the call regenerates, bit for bit
    x = dev(d.x)
    cov = plan.predict_cov(x)
    W = R.w_of_u(U)
    r2 = R.scaled_sqdist(d.x, d.x, d.ell)
    ref = R.reference(F, F, W, d.s2 * R.kappa(c.kind, r2))
    bars = R.bars(F, F, W, c.kind, r2, d.s2, R.plan_padded(c.M), plan.scale_exp)
    assert cov.shape == (c.L, n, n)
    check_tight("training", host(cov), ref, bars.total)
    gen = plan.predict_cov(x, x.clone())
    check_tight("training, general form", host(gen), ref, bars.total)
    # the plan's own marginal variances are the diagonal
    _, var = plan.predict(x)
    dbar = np.stack([np.diag(bars.total[l]) for l in range(c.L)]) + R.predict_var_bar(F, U, d.s2, R.plan_padded(c.M))
    assert (np.abs(host(torch.diagonal(cov, dim1=1, dim2=2)).astype(np.float64) - host(var)) <= dbar).all()


def test_a_block_does_not_depend_on_the_call_it_was_computed_in(world):
    ctx, setup, features = world
    c = R.TIGHT[1]  # M 64, L 3, 127 x 129
    plan, d, U = setup(c)
    xa, xb = dev(d.xa), dev(d.xb)
    full = plan.predict_cov(xa, xb)
    for (i0, i1), (j0, j1) in (((5, 100), (17, 129)), ((126, 127), (0, 1)), ((0, 127), (128, 129))):
        part = plan.predict_cov(xa[i0:i1].contiguous(), xb[j0:j1].contiguous())
        assert torch.equal(part, full[:, i0:i1, j0:j1]), ((i0, i1), (j0, j1))
    # through ld: the same block written into a wider matrix
    wide = torch.zeros((c.L, c.Na, 200), dtype=torch.float32, device="cuda")
    rc, _ = raw_cov(plan, xa, c.Na, xb, c.Nb, wide, 200)
    assert rc == 0 and torch.equal(wide[:, :, : c.Nb], full) and not wide[:, :, c.Nb:].any()
    # interleaved with the other users of the plan's prediction scratch
    mu0, var0 = plan.predict(xb)
    V = dev(np.random.default_rng(5).standard_normal((7, c.L, c.M)))
    ch0 = plan.predict_chain(V, xa)
    again = plan.predict_cov(xa, xb)
    mu1, var1 = plan.predict(xb)
    ch1 = plan.predict_chain(V, xa)
    sym = plan.predict_cov(xb)
    again2 = plan.predict_cov(xa, xb)
    assert torch.equal(again, full) and torch.equal(again2, full)
    assert torch.equal(mu0, mu1) and torch.equal(var0, var1) and all(torch.equal(p, q) for p, q in zip(ch0, ch1))
    assert torch.equal(sym, sym.transpose(1, 2))


@pytest.mark.parametrize("long_side", ["a", "b"])
def test_the_chunk_seam(world, long_side):
    ctx, setup, features = world
    c = R.TIGHT[0]  # M 5, L 1, D 1
    plan, d, U = setup(c)
    rng = np.random.default_rng(77)
    n_long, n_short = CHUNK + 129, 129
    xl, xs = dev(rng.uniform(-10, 10, size=(n_long, 1))), dev(rng.uniform(-10, 10, size=(n_short, 1)))
    lo, hi = CHUNK - 200, n_long  # a window over the seam, not aligned to a tile
    if long_side == "a":
        full = plan.predict_cov(xl, xs)
        assert torch.equal(plan.predict_cov(xl[lo:hi].contiguous(), xs), full[:, lo:hi])
        assert torch.equal(plan.predict_cov(xl[:129].contiguous(), xs), full[:, :129])
    else:
        full = plan.predict_cov(xs, xl)
        assert torch.equal(plan.predict_cov(xs, xl[lo:hi].contiguous()), full[:, :, lo:hi])
        assert torch.equal(plan.predict_cov(xs, xl[:129].contiguous()), full[:, :, :129])
    assert torch.isfinite(full).all()


def test_the_chunk_seam_of_the_symmetric_form(world):
    """Na = 65536 + 129 with x_b = NULL: two chunks of either side, so a chunk pair on the diagonal whose a image is its own, one
    strictly below it (every entry mirrored through the second output pointer, row and column offsets that differ) and one above it
    that is skipped.  The 17 GB output is what the path needs: nothing smaller reaches it.  It is judged in strips, on the device."""
    ctx, setup, features = world
    c = R.TIGHT[0]  # M 5, L 1, D 1
    plan, d, U = setup(c)
    rng = np.random.default_rng(78)
    n = CHUNK + 129
    x = dev(rng.uniform(-10, 10, size=(n, 1)))
    lo = CHUNK - 200  # a window over the seam, not aligned to a tile
    full = plan.predict_cov(x)
    assert full.shape == (1, n, n)
    win, head = x[lo:].contiguous(), x[:129].contiguous()
    # on and below the diagonal: the general call's entries, bit for bit, in every chunk pair
    gen = plan.predict_cov(win, win.clone())
    low = torch.tril(torch.ones(n - lo, n - lo, dtype=torch.bool, device="cuda"))
    assert torch.equal(full[:, lo:, lo:][:, low], gen[:, low])
    assert torch.equal(full[:, lo:, :129], plan.predict_cov(win, head))  # rows on both sides of the seam against the first chunk
    assert torch.equal(full[:, lo:, lo:], plan.predict_cov(win))          # the same block from a one-chunk symmetric call
    # symmetric bit for bit: strips of rows against the same strips of columns, over the whole width
    for i0, i1 in ((0, 129), (lo, n), (CHUNK // 2, CHUNK // 2 + 64)):
        assert torch.equal(full[0, i0:i1, :], full[0, :, i0:i1].t()), (i0, i1)
    assert torch.isfinite(full[0, lo:, :]).all() and torch.isfinite(full[0, :129, :]).all()
    del full
    torch.cuda.empty_cache()


def test_ld_and_empty_sets_write_nothing_else(world):
    ctx, setup, features = world
    c = R.TIGHT[3]  # M 300, L 3, 129 x 128
    plan, d, U = setup(c)
    xa, xb = dev(d.xa), dev(d.xb)
    want = plan.predict_cov(xa, xb)
    ld = c.Nb + 37
    pattern = 0x7FC12345  # a NaN with a payload
    out = torch.full((c.L, c.Na, ld), pattern, dtype=torch.int32, device="cuda")
    rc, _ = raw_cov(plan, xa, c.Na, xb, c.Nb, out, ld)
    ctx.synchronize()
    assert rc == 0
    assert torch.equal(out.view(torch.float32)[:, :, : c.Nb], want)
    assert (out[:, :, c.Nb:] == pattern).all()
    # the symmetric form under ld
    outs = torch.full((c.L, c.Na, c.Na + 3), pattern, dtype=torch.int32, device="cuda")
    rc, _ = raw_cov(plan, xa, c.Na, None, c.Na, outs, c.Na + 3)
    ctx.synchronize()
    assert rc == 0 and (outs[:, :, c.Na:] == pattern).all()
    assert torch.equal(outs.view(torch.float32)[:, :, : c.Na], plan.predict_cov(xa))
    # empty sets
    for Na, Nb, b in ((0, c.Nb, xb), (c.Na, 0, xb), (0, 0, None)):
        out.fill_(pattern)
        rc, _ = raw_cov(plan, xa, Na, b, Nb, out, ld)
        ctx.synchronize()
        assert rc == 0 and (out == pattern).all()
    assert plan.predict_cov(xa[:0], xb).shape == (c.L, 0, c.Nb) and plan.predict_cov(xa, xb[:0]).shape == (c.L, c.Na, 0)


def test_non_finite_inputs_poison_their_row_or_column_only(world):
    ctx, setup, features = world
    c = R.TIGHT[1]
    plan, d, U = setup(c)
    xa, xb = dev(d.xa), dev(d.xb)
    clean = plan.predict_cov(xa, xb)
    bad_b = xb.clone()
    bad_b[3, 0], bad_b[128, 1] = float("nan"), float("inf")
    got = plan.predict_cov(xa, bad_b)
    cols = torch.zeros(c.Nb, dtype=torch.bool, device="cuda")
    cols[[3, 128]] = True
    assert torch.isnan(got[:, :, cols]).all() and torch.equal(got[:, :, ~cols], clean[:, :, ~cols])
    bad_a = xa.clone()
    bad_a[126, 0] = float("-inf")
    got = plan.predict_cov(bad_a, xb)
    rows = torch.zeros(c.Na, dtype=torch.bool, device="cuda")
    rows[126] = True
    assert torch.isnan(got[:, rows]).all() and torch.equal(got[:, ~rows], clean[:, ~rows])
    # symmetric form: row and column of the point
    s_clean = plan.predict_cov(xb)
    got = plan.predict_cov(bad_b)
    assert torch.isnan(got[:, cols]).all() and torch.isnan(got[:, :, cols]).all()
    assert torch.equal(got[:, ~cols][:, :, ~cols], s_clean[:, ~cols][:, :, ~cols])


def test_errors_leave_the_context_usable(A, world):
    from agpl_amd import _ffi

    ctx, setup, features = world
    c = R.TIGHT[1]
    plan, d, U = setup(c)
    xa, xb = dev(d.xa), dev(d.xb)
    want = plan.predict_cov(xa, xb)
    out = torch.zeros((c.L, c.Na, c.Nb), dtype=torch.float32, device="cuda")
    E = _ffi.ERR_INVALID_ARGUMENT
    for args, word in (((None, c.Na, xb, c.Nb, out, c.Nb), "null"), ((xa, c.Na, xb, c.Nb, None, c.Nb), "null"),
                       ((xa, c.Na, xb, c.Nb, out, c.Nb - 1), "ld"), ((xa, -1, xb, c.Nb, out, c.Nb), "negative"),
                       ((xa, c.Na, xb, -1, out, c.Nb), "negative"), ((xa, c.Na, None, c.Nb, out, c.Nb), "symmetric")):
        x1, Na, x2, Nb, o, ld = args
        rc, msg = raw_cov(plan, x1, Na, x2, Nb, o, ld)
        assert rc == E and word in msg, (rc, msg, word)
    assert _ffi.joint_lib().agpl_plan_predict_cov(None, 1, ptr(xa), 1, ptr(xb), ptr(out), 1) == E  # no plan: no context to report through
    # plans that cannot: one from features, one without the marginal image (what agpl_plan_predict refuses)
    Phi = plan.features().contiguous()
    flat = A.Plan(Phi, plan.resid.clone(), c.L, ctx)
    rc, msg = raw_cov(flat, xa, c.Na, xb, c.Nb, out, c.Nb)
    assert rc == E and "raw inputs" in msg
    nomarg = A.Plan.from_inputs(dev(d.x), dev(d.z), d.ell, variance=d.s2, jitter=R.JITTER, L=c.L, ctx=ctx, flags=A.Plan.NO_MARGINALS,
                                kernel=kernel_arg(c.kind))
    rc, msg = raw_cov(nomarg, xa, c.Na, xb, c.Nb, out, c.Nb)
    assert rc == E and "AGPL_PLAN_NO_MARGINALS" in msg
    assert not out.any()  # nothing was written by any refused call
    # the Python surface raises the same
    with pytest.raises(A.ArgumentError):
        flat.predict_cov(xa)
    with pytest.raises(A.ArgumentError):
        nomarg.predict_cov(xa)
    with pytest.raises(A.ArgumentError, match=r"x_b must be \[Ns, 2\]"):
        plan.predict_cov(xa, torch.zeros((4, 3), dtype=torch.float64, device="cuda"))
    with pytest.raises(A.ArgumentError, match="eps must be"):
        plan.sample_f(xa, eps=torch.zeros((2, c.L, c.Na + 1), dtype=torch.float64, device="cuda"))
    # and the context serves a correct call
    assert torch.equal(plan.predict_cov(xa, xb), want)


def test_sample_f(A, world):
    ctx, setup, features = world
    c = R.SAMPLE  # Ns 257, L 3
    plan, d, U = setup(c)
    xs = dev(d.xa)
    # two float64 factorisations that sum in different orders agree to about cond 2^-53; the case's covariance (variance 2.5) has
    # eigenvalues from 1e-4 to 44, so cond = 44 / (1e-4 + jitter s2) = 2e4 at jitter 1e-3: an agreement near 2e-12, under the 1e-10
    # asked for with room (the default jitter 1e-6 would leave cond 4e5 and a tenth of that room)
    ns, jitter = 4, 1e-3
    eps = np.random.default_rng(9).standard_normal((ns, c.L, c.Na))
    mu0 = (0.5 * np.random.default_rng(10).standard_normal((c.L, c.Na))).astype(np.float32)
    f = plan.sample_f(xs, mu0_s=dev(mu0), jitter=jitter, eps=dev(eps))
    assert f.shape == (ns, c.L, c.Na) and f.dtype == torch.float64
    cov = host(plan.predict_cov(xs)).astype(np.float64)
    mu = host(plan.predict(xs, dev(mu0))[0]).astype(np.float64)
    for l in range(c.L):
        Cl = np.linalg.cholesky(cov[l] + jitter * d.s2 * np.eye(c.Na))
        ref = mu[l][None] + eps[:, l] @ Cl.T
        err = np.abs(host(f)[:, l] - ref).max() / np.abs(ref).max()
        print(f"latent {l}: sample_f against numpy's factor, relative {err:.2e}")
        assert err <= 1e-10
    # the same seed gives the same draws; another seed does not
    g = torch.Generator(device="cuda")
    draws = []
    for seed in (123, 123, 124):
        g.manual_seed(seed)
        draws.append(plan.sample_f(xs, nsamples=2, jitter=jitter, generator=g))
    assert draws[0].shape == (2, c.L, c.Na) and torch.equal(draws[0], draws[1]) and not torch.equal(draws[0], draws[2])
    # a covariance that no jitter repairs: 128 points twice and jitter 0.  Rows i and i + 128 are equal bit for bit, so each of the
    # last 128 pivots is the rounding residue of a difference that is zero in exact arithmetic -- not all of them can come out positive.
    # The library's not-positive-definite error comes back naming the jitter, and the context then serves the first call again.
    dup = torch.cat([xs[:128], xs[:128]])
    with pytest.raises(A.PosDefException, match="jitter = 0"):
        plan.sample_f(dup, jitter=0.0)
    assert torch.equal(plan.sample_f(xs, mu0_s=dev(mu0), jitter=jitter, eps=dev(eps)), f)


def test_sparse_cavi_forwards(A):
    """SparseCAVI.predict_cov / sample_f after a few Bernoulli sweeps: the plan's methods, and the diagonal is its predict's var."""
    lik = A.BernoulliLikelihood()
    ctx = A.Context(0, seed=7)
    N, M = 4096, 64
    x, y = A.synth_xy(lik, 20240807, 0, N, ctx=ctx)
    z = np.linspace(-10, 10, M)
    cavi = A.SparseCAVI.from_inputs(lik, x, y, torch.from_numpy(z).cuda(), 1.5 * (z[1] - z[0]), ctx=ctx)
    cavi.run(3)
    cavi.check()
    xs = torch.linspace(-12, 12, 257, dtype=torch.float64, device="cuda")
    cov = cavi.predict_cov(xs)
    assert torch.equal(cov, cavi.plan.predict_cov(xs)) and torch.equal(cov, cov.transpose(1, 2))
    _, var = cavi.predict(xs)
    assert np.abs(host(torch.diagonal(cov, dim1=1, dim2=2)) - host(var)).max() <= 2e-5 * float(var.max())
    eps = torch.randn((3, 1, 257), dtype=torch.float64, device="cuda")
    assert torch.equal(cavi.sample_f(xs, eps=eps, jitter=1e-4), cavi.plan.sample_f(xs, eps=eps, jitter=1e-4))
    flat = A.SparseCAVI(lik, cavi.plan.features().contiguous(), cavi.plan.resid.clone(), y, ctx=ctx)
    with pytest.raises(A.ArgumentError):
        flat.predict_cov(xs)
    with pytest.raises(A.ArgumentError):
        flat.sample_f(xs)
