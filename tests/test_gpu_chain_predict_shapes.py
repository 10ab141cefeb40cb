"""GPU tests of agpl_plan_predict_chain (include/agpl_chain.h; csrc/agpl_chain.hip) at the latent counts, block seams, feature pads
and scales that tests/test_gpu_chain_predict.py leaves out:

* latent counts that do not divide a half block of 64 rows (3, 5, 10), vbar's block beyond 32 rows (33, 64 -- the most LDS a
  workgroup may ask for), T L on every seam of the 32-row groups and 128-row blocks, and on exact multiples of 128;
* two feature pads (M = 300 ragged and M = 512: Mp = 512);
* one scale for the whole image: a latent 2^-10 / 2^-20 below the other, a burn-in draw 2^12 / 2^20 above the rest;
* power-of-two scales of V give the same bits; constant and zero chains (the e = 0 fall-back of either scale);
* Ns = 1, 127, 128, 129 against the same points of Ns = 300, resid_out = NULL, Ns = 0;
* the prediction scratch shared with agpl_plan_predict, grown between two calls of it.

Every comparison is element-wise against tests/chain_reference.py -- float64 with the plan's own exact features, bars from the
kernel's arithmetic (derived there; tests/test_chain_reference_cpu.py shows on these very data that a correct implementation stays
within them and that six wrong ones do not).  The data tell latents and draws apart: V[t, l] ~ (1 + l) N(0, 1), mu0[l] ~ 10 (l + 1).
D = 2, N = Ns = 300 (two full 128-point tiles and a ragged one).
"""
import ctypes as C

import numpy as np
import pytest

import chain_reference as R

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

N, D = R.N, 2
JITTER = 1e-8
SENTINEL = -7.0


@pytest.fixture(scope="module")
def A():
    import agpl_amd

    return agpl_amd


def host(t):
    return t.detach().cpu().numpy()


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


@pytest.fixture(scope="module")
def world(A):
    """One context, the plans by (M, L) built once, their features in float64 (exact: hi + lo of the image), the points on the device."""
    ctx = A.Context(0, seed=11)
    plans, feats, xs = {}, {}, {}

    def points(M):
        if M not in xs:
            xs[M] = dev(R.se_inputs(M)[0])
        return xs[M]

    def plan(M, L):
        if (M, L) not in plans:
            _, z, ell = R.se_inputs(M)
            plans[M, L] = A.Plan.from_inputs(points(M), dev(z), ell, jitter=JITTER, L=L, ctx=ctx)
            assert plans[M, L].Mp == R.plan_padded(M)
        return plans[M, L]

    def features(M):
        if M not in feats:
            feats[M] = host(plan(M, 1).features()).astype(np.float64)
        return feats[M]

    return ctx, plan, features, points


def raw_chain(plan, V, x_s, mu0_s=None, Ns=None, resid=True, samples=True):
    """The C entry point on sentinel-filled outputs of x_s' size, for the first Ns points: (mean, spread, resid, F)."""
    from agpl_amd import _ffi

    T, n, L = V.shape[0], x_s.shape[0], plan.L
    Ns = n if Ns is None else Ns
    f32 = torch.float32
    mean = torch.full((L, Ns), SENTINEL, dtype=f32, device="cuda") if Ns else torch.full((L, n), SENTINEL, dtype=f32, device="cuda")
    spread = torch.full_like(mean, SENTINEL)
    res = torch.full((max(Ns, 1),), SENTINEL, dtype=f32, device="cuda") if resid else None
    F = torch.full((T, L, mean.shape[1]), SENTINEL, dtype=f32, device="cuda") if samples else None
    ptr = lambda t: C.c_void_p(0 if t is None else t.data_ptr())
    plan.call("agpl_plan_predict_chain", C.c_int32(T), ptr(V), C.c_int64(Ns), ptr(x_s), ptr(mu0_s), ptr(mean), ptr(spread), ptr(res),
              ptr(F), lib=_ffi.chain_lib())
    return mean, spread, res, F


def run(world, c):
    """A case of tests/chain_reference.py on its plan at the plan's own points: the device outputs and (V, mu0)."""
    ctx, plan, features, points = world
    V, mu0 = R.case_data(c)
    return raw_chain(plan(c.M, c.L), dev(V), points(c.M), dev(mu0)), V, mu0


def ratio(err, bar):
    with np.errstate(divide="ignore", invalid="ignore"):
        return float(np.max(np.where(bar > 0, err / bar, np.where(err > 0, np.inf, 0.0))))


def check(world, c, out, V, mu0):
    """F, mean and spread within their element-wise bars (every element), all finite; returns the reference and the bars."""
    Phi = world[2](c.M)
    mean, spread, resid, F = (host(t) for t in out)
    ref = R.reference(Phi, V, mu0)
    bars = R.bars(Phi, ref, R.plan_padded(c.M))
    errs = [np.abs(got.astype(np.float64) - want) for got, want in ((F, ref.F), (mean, ref.mean), (spread, ref.spread))]
    print(f"{c.id}: max err / bar  F {ratio(errs[0], bars.F):.3f}  mean {ratio(errs[1], bars.mean):.3f}  "
          f"spread {ratio(errs[2], bars.spread):.3f}   (max err F {errs[0].max():.3e}, mean {errs[1].max():.3e}, "
          f"spread {errs[2].max():.3e} of {ref.spread.max():.3e})")
    for got in (F, mean, spread, resid):
        assert np.isfinite(got).all()
    for name, err, bar in zip(("F", "mean", "spread"), errs, (bars.F, bars.mean, bars.spread)):
        assert (err <= bar).all(), (name, ratio(err, bar))
    assert torch.equal(out[2], world[1](c.M, c.L).resid)
    return ref, bars, errs


@pytest.mark.parametrize("c", R.SEAMS + R.PADS, ids=lambda c: c.id)
def test_seams_and_feature_pads(world, c):
    check(world, c, *run(world, c))


@pytest.mark.parametrize("c", R.SCALES, ids=lambda c: c.id)
def test_one_scale_for_the_whole_image(world, c):
    out, V, mu0 = run(world, c)
    ref, bars, errs = check(world, c, out, V, mu0)
    if c.kind == "small_latent":  # the small latent alone: its error, its bar, and how many digits of its own size it keeps
        eF, eS = errs[0][:, 1], errs[2][1]
        own = np.abs(ref.q[:, 1]).max()
        print(f"  latent 1 alone: F max err / bar {ratio(eF, bars.F[:, 1]):.3f}, max err / max |phi' (v - vbar)| {eF.max() / own:.3e}; "
              f"spread max err / bar {ratio(eS, bars.spread[1]):.3f}, max err / max spread {eS.max() / ref.spread[1].max():.3e}")
        assert (eF <= bars.F[:, 1]).all() and (eS <= bars.spread[1]).all()
    else:  # the draws after the burn-in one
        eF = errs[0][1:]
        print(f"  draws 1 ..: F max err / bar {ratio(eF, bars.F[1:]):.3f}, max err / max |F_ref| {eF.max() / np.abs(ref.F[1:]).max():.3e}")
        assert (eF <= bars.F[1:]).all()


def test_power_of_two_scales_of_the_chain_give_the_same_bits(world):
    outs = {}
    for c in R.POW2:
        out, V, mu0 = run(world, c)
        assert mu0 is None
        check(world, c, out, V, mu0)
        outs[c.arg] = out
    mean0, spread0, _, F0 = outs[0]
    for k in (20, -20):
        mean, spread, _, F = outs[k]
        assert torch.equal(F, F0 * 2.0 ** k) and torch.equal(mean, mean0 * 2.0 ** k)
        assert torch.equal(spread, spread0 * 4.0 ** k)
        assert (spread0 > 0).all()  # nothing underflowed on the way


def test_constant_and_zero_chains(world):
    four, three, zero_mu0, zero = R.DEGENERATE
    # four equal draws: vbar is exact, every centred entry 0 (the e = 0 fall-back of the centred scale)
    out, V, mu0 = run(world, four)
    check(world, four, out, V, mu0)
    mean, spread, _, F = out
    assert torch.equal(spread, torch.zeros_like(spread))
    for t in range(four.T):
        assert torch.equal(F[t], mean)
    # three equal draws: vbar may be an ulp off and the centred image holds those ulps at full scale.  The reference sums in the
    # header's order, so its centred draws are the same ulps: F and the (1e-32-sized) spread stay within their bars
    out, V, mu0 = run(world, three)
    ref, _, _ = check(world, three, out, V, mu0)
    assert np.abs(ref.cen).max() <= 2.0 ** -50 * np.abs(V).max()
    # a zero chain (the e = 0 fall-back of both scales)
    out, V, mu0 = run(world, zero_mu0)
    mean, spread, _, F = out
    m = dev(mu0)
    assert torch.equal(mean, m) and torch.equal(spread, torch.zeros_like(spread))
    for t in range(zero_mu0.T):
        assert torch.equal(F[t], m)
    out, V, mu0 = run(world, zero)
    assert mu0 is None
    for t in (out[0], out[1], out[3]):
        assert torch.equal(t, torch.zeros_like(t))


def test_prefixes_optional_outputs_and_no_points(world):
    ctx, plan, features, points = world
    c = R.NS_EDGES
    p, x = plan(c.M, c.L), points(c.M)
    V, mu0 = R.case_data(c)
    Vd, md = dev(V), dev(mu0)
    full = raw_chain(p, Vd, x, md)
    for Ns in (1, 127, 128, 129):
        mean, spread, resid, F = raw_chain(p, Vd, x[:Ns].contiguous(), md[:, :Ns].contiguous())
        assert torch.equal(mean, full[0][:, :Ns]) and torch.equal(spread, full[1][:, :Ns])
        assert torch.equal(resid, full[2][:Ns]) and torch.equal(F, full[3][:, :, :Ns])
    mean, spread, resid, F = raw_chain(p, Vd, x, md, resid=False)
    assert resid is None
    assert torch.equal(mean, full[0]) and torch.equal(spread, full[1]) and torch.equal(F, full[3])
    for t in raw_chain(p, Vd, x, md, Ns=0):  # AGPL_OK (plan.call raises otherwise) and nothing written
        assert torch.equal(t, torch.full_like(t, SENTINEL))


def test_scratch_shared_with_predict(world, A):
    ctx = world[0]
    M = 64
    x, z, ell = R.se_inputs(M)
    rng = np.random.default_rng(41)
    y = dev((rng.uniform(size=N) < 1 / (1 + np.exp(-2 * np.sin(x[:, 0])))).astype(np.uint8))
    xd, zd = dev(x), dev(z)
    cavi = A.SparseCAVI.from_inputs(A.BernoulliLikelihood(), xd, y, zd, ell, jitter=JITTER, ctx=ctx)
    cavi.run(2)
    xs = dev(rng.uniform(-12, 12, size=(N, D)))
    V_big, V_small = dev(rng.standard_normal((300, 1, M))), dev(rng.standard_normal((5, 1, M)))
    a = cavi.predict(xs)
    big = raw_chain(cavi.plan, V_big, xs)  # larger than anything before on this plan: the scratch grows
    b = cavi.predict(xs)
    small = raw_chain(cavi.plan, V_small, xs)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    fresh = A.Plan.from_inputs(xd, zd, ell, jitter=JITTER, L=1, ctx=ctx)
    for got, V in ((big, V_big), (small, V_small)):
        for u, v in zip(got, raw_chain(fresh, V, xs)):
            assert torch.isfinite(u).all() and torch.equal(u, v)
