"""agpl_predictive_cdf / agpl_predictive_quantile on the device (include/agpl_quantile.h) over the whole grid of
tests/quantile_domain.py, one launch per parameter set, against the float64 reference of tests/quantile_reference.py (route "a";
tests/test_quantile_reference_cpu.py proves it against route "b" on every point).

Bars.  cdf and sf: |device - ref| <= 1e-8 (the trapezoid rule at spacing <= 0.5 with poles at distance pi: exp(-2 pi pi / 0.5) = 7e-18;
the mass beyond +-8 s: 1.2e-15; summation over <= 4096 nodes: 1e-12; the rest for the special functions), and <= 1e-4 of the reference
wherever the reference is >= 1e-12 -- what computing each tail as such buys.  Continuous quantiles: |F_ref(q) - p| <= 2e-8 (the bar
of the distribution function plus the solve's residual 1e-10), with the REFERENCE distribution function at the device's answer.
Bernoulli: q is 0 or 1 and the reference's, except where p is within 2e-8 of the jump.  Counts: q is integer-valued,
F_ref(q) >= p - 2e-8 and (q = 0 or F_ref(q - 1) < p + 2e-8): both neighbours pass only inside that band.  No point is skipped; a
(point, prob) pair of a count kind is on the grid where the reference's quantile does not exceed the cap of 1e5."""
import numpy as np
import pytest

import quantile_domain as D
import quantile_reference as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def A():
    import agpl_amd

    return agpl_amd


@pytest.fixture(scope="module")
def ctx(A):
    return A.Context(seed=1234)


def _lik(A, kind, p):
    return {"bernoulli": lambda: A.BernoulliLikelihood(), "poisson": lambda: A.PoissonLikelihood(p[0]),
            "negbinomial": lambda: A.NegativeBinomialLikelihood(p[0]), "studentt": lambda: A.StudentTLikelihood(p[0], p[1]),
            "laplace": lambda: A.LaplaceLikelihood(p[0]), "heterogauss": lambda: A.HeteroscedasticGaussianLikelihood(p[0])}[kind]()


def _dev(a):
    import torch

    return torch.as_tensor(np.ascontiguousarray(a)).cuda()


def _ydt(kind):
    return {"bernoulli": np.uint8, "poisson": np.int32, "negbinomial": np.int32}.get(kind, np.float64)


def _flat(kind, pts):
    """(names, y, mu, var) of every (point, threshold) of one parameter set."""
    rows = [(name, y, mu, var) for name, p, mu, var in pts for y in D.thresholds(kind, p, mu, var)]
    return rows, np.array([r[1] for r in rows], dtype=_ydt(kind)), np.array([r[2] for r in rows], dtype=np.float64), np.array([r[3] for r in rows], dtype=np.float64)


@pytest.mark.parametrize("kind", D.KINDS)
def test_distribution_function_over_the_domain(A, ctx, kind):
    worst = dict(cdf=(0.0, ""), sf=(0.0, ""), cdf_rel=(0.0, ""), sf_rel=(0.0, ""))
    bad, n = [], 0
    for p, pts in D.groups(kind):
        rows, y, mu, var = _flat(kind, pts)
        cdf, sf = (o.cpu().numpy() for o in A.predictive_cdf(_lik(A, kind, p), (_dev(mu), _dev(var)), _dev(y), ctx=ctx))
        for i, (name, yi, mi, vi) in enumerate(rows):
            n += 1
            ref = R.ref_cdf(kind, p, yi, mi, vi)
            for key, got, want in (("cdf", cdf[i], ref[0]), ("sf", sf[i], ref[1])):
                figs = {key: abs(got - want) / 1e-8}
                if want >= 1e-12:
                    figs[key + "_rel"] = abs(got - want) / (1e-4 * want)
                for k, f in figs.items():
                    if not f <= worst[k][0]:
                        worst[k] = (float(f), f"{name} y={yi:g}")
                    if not f <= 1.0:
                        bad.append((name, yi, k, float(got), want))
    print(f"{kind}: {n} (point, threshold) pairs, worst in units of the bar: " + ", ".join(f"{k} {f:.3e} at {w}" for k, (f, w) in worst.items()))
    assert n == sum(len(D.thresholds(kind, *pt[1:])) for pt in D.GRID[kind]) >= 70
    assert not bad, bad


@pytest.mark.parametrize("kind", D.COUNTS)
def test_count_quantiles_over_the_domain(A, ctx, kind):
    worst, bad, n = (0.0, ""), [], 0
    probs = np.array(D.COUNT_PROBS)
    tail = lambda ref, pj: ref[0] - pj if pj <= 0.5 else (1.0 - pj) - ref[1]  # F - p on the tail p is in
    for p, pts in D.groups(kind):
        mu = np.array([pt[2] for pt in pts], dtype=np.float64)
        var = np.array([pt[3] for pt in pts], dtype=np.float64)
        lik, qf = _lik(A, kind, p), (_dev(mu), _dev(var))
        q = A.predictive_quantile(lik, qf, probs, ctx=ctx).cpu().numpy()
        for i, (name, _, mi, vi) in enumerate(pts):
            for j, pj in enumerate(probs):
                if R.ref_count_quantile(kind, p, pj, mi, vi, D.COUNT_CAP) is None:
                    continue  # (beyond the cap: not on the grid)
                n += 1
                qi = q[i, j]
                ok = np.isfinite(qi) and qi == np.floor(qi) and 0 <= qi <= D.COUNT_CAP
                if ok:
                    up = tail(R.ref_cdf(kind, p, int(qi), mi, vi), pj)
                    dn = tail(R.ref_cdf(kind, p, int(qi) - 1, mi, vi), pj) if qi > 0 else -1.0
                    f = max(-up, dn) / 2e-8  # F_ref(q) >= p - 2e-8 and F_ref(q - 1) < p + 2e-8
                    ok = up >= -2e-8 and (qi == 0 or dn < 2e-8)
                    if f > worst[0]:
                        worst = (float(f), f"{name} p={pj:g}")
                if not ok:
                    bad.append((name, pj, float(qi)))
        assert (np.diff(q, axis=1) >= 0.0).all()
    print(f"{kind}: {n} (point, prob) pairs, worst excursion into the band in units of 2e-8: {worst[0]:.3e} at {worst[1]}")
    assert n >= 60 and not bad, bad


@pytest.mark.parametrize("kind", [k for k in D.KINDS if k not in D.COUNTS])
def test_quantiles_over_the_domain(A, ctx, kind):
    import torch

    worst, bad, n = (0.0, ""), [], 0
    probs = np.array(D.PROBS)
    for p, pts in D.groups(kind):
        mu = np.array([pt[2] for pt in pts], dtype=np.float64)
        var = np.array([pt[3] for pt in pts], dtype=np.float64)
        lik, qf = _lik(A, kind, p), (_dev(mu), _dev(var))
        qd = A.predictive_quantile(lik, qf, probs, ctx=ctx)
        q = qd.cpu().numpy()
        assert q.shape == (len(pts), len(probs)) and np.isfinite(q).all()
        assert (np.diff(q, axis=1) >= 0.0).all()  # non-decreasing in probs
        for j, pj in enumerate(probs):  # round trip on the device: the distribution function at the quantile gives the prob back
            if kind == "bernoulli":
                continue
            c, s = (o.cpu().numpy() for o in A.predictive_cdf(lik, qf, qd[:, j].contiguous(), ctx=ctx))
            assert np.abs(c - pj).max() <= 2e-8 and np.abs(s - (1.0 - pj)).max() <= 2e-8, (kind, p, pj)
        for i, (name, _, mi, vi) in enumerate(pts):
            for j, pj in enumerate(probs):
                n += 1
                if kind == "bernoulli":
                    c0 = R.ref_cdf(kind, p, 0, mi, vi)[0]
                    ok = q[i, j] in (0.0, 1.0) and (q[i, j] == (0.0 if pj <= c0 else 1.0) or abs(pj - c0) <= 2e-8)
                    f = 0.0 if ok else np.inf
                else:
                    c, s = R.ref_cdf(kind, p, float(q[i, j]), mi, vi)
                    f = (abs(c - pj) if pj <= 0.5 else abs(s - (1.0 - pj))) / 2e-8
                if not f <= worst[0]:
                    worst = (float(f), f"{name} p={pj:g}")
                if not f <= 1.0:
                    bad.append((name, pj, float(q[i, j]), float(f)))
    print(f"{kind}: {n} (point, prob) pairs, worst |F_ref(q) - p| in units of 2e-8: {worst[0]:.3e} at {worst[1]}")
    assert n == len(D.GRID[kind]) * len(probs)
    assert not bad, bad
    assert torch.equal(qd, A.predictive_quantile(lik, qf, probs, ctx=ctx))  # two calls, the same bits


def test_quantile_against_the_reference_solve(A, ctx):
    """A handful of points against brentq on the reference distribution function: the device's answer is the reference's to the
    residuals' worth of y (|dF| <= 2e-8 over the density)."""
    for kind, idx in (("studentt", 2), ("laplace", 9), ("heterogauss", 5)):
        name, p, mu, var = D.GRID[kind][idx]
        q = A.predictive_quantile(_lik(A, kind, p), (_dev(np.atleast_2d(mu) if kind == "heterogauss" else [mu]),
                                                     _dev(np.atleast_2d(var) if kind == "heterogauss" else [var])), D.PROBS, ctx=ctx).cpu().numpy()[0]
        for j, pj in enumerate(D.PROBS):
            want = R.ref_quantile(kind, p, pj, mu, var, D.scale(kind, p, mu, var))
            c, s = R.ref_cdf(kind, p, float(q[j]), mu, var)
            cw, sw = R.ref_cdf(kind, p, want, mu, var)
            assert (abs(c - cw) if pj <= 0.5 else abs(s - sw)) <= 2e-8, (name, pj, q[j], want)


@pytest.mark.parametrize("n", [1, 255, 257, 3 * 256 + 7])  # kBlock = 256: the lane and workgroup seams
@pytest.mark.parametrize("nq", [1, 16])
def test_shapes(A, ctx, n, nq):
    import torch

    rng = np.random.default_rng(n + nq)
    mu, var, y = rng.normal(size=n), rng.uniform(0.0, 4.0, size=n), rng.normal(size=n) * 3.0
    probs = np.linspace(0.01, 0.99, nq) if nq > 1 else np.array([0.3])
    lik = A.StudentTLikelihood(1.5, 0.5)
    qf = (_dev(mu), _dev(var))
    c1, s1 = A.predictive_cdf(lik, qf, _dev(y), ctx=ctx)
    c2, s2 = A.predictive_cdf(lik, qf, _dev(y), ctx=ctx)
    q1, q2 = A.predictive_quantile(lik, qf, probs, ctx=ctx), A.predictive_quantile(lik, qf, probs, ctx=ctx)
    assert torch.equal(c1, c2) and torch.equal(s1, s2) and torch.equal(q1, q2)
    assert q1.shape == (n, nq) and c1.shape == (n,)
    # every point is its own lane: the values do not depend on the point's place in the launch
    pick = sorted({0, n // 2, n - 1})
    qs = A.predictive_quantile(lik, (_dev(mu[pick]), _dev(var[pick])), probs, ctx=ctx)
    cs, ss = A.predictive_cdf(lik, (_dev(mu[pick]), _dev(var[pick])), _dev(y[pick]), ctx=ctx)
    assert torch.equal(qs, q1[pick]) and torch.equal(cs, c1[pick]) and torch.equal(ss, s1[pick])
    c, s = c1.cpu().numpy(), s1.cpu().numpy()
    assert np.abs(c + s - 1.0).max() <= 1e-13 and ((c > 0) & (c < 1)).all()


def test_conventions(A, ctx):
    import ctypes as C

    import torch
    from agpl_amd import _ffi

    st, lap, het, ber = A.StudentTLikelihood(3.0, 1.0), A.LaplaceLikelihood(1.0), A.HeteroscedasticGaussianLikelihood(2.0), A.BernoulliLikelihood()
    nan, inf = np.nan, np.inf
    # a negative or non-finite var, a non-finite mu: NaN in that point's outputs, the others untouched
    mu = np.array([0.0, 0.0, nan, inf, 0.0, 0.5])
    var = np.array([1.0, -1.0, 1.0, 1.0, inf, nan])
    poi = A.PoissonLikelihood(3.0)
    for lik in (st, lap, ber, poi):
        y = np.zeros(6, dtype=np.uint8 if lik is ber else (np.int32 if lik is poi else np.float64))
        c, s = (o.cpu().numpy() for o in A.predictive_cdf(lik, (_dev(mu), _dev(var)), _dev(y), ctx=ctx))
        q = A.predictive_quantile(lik, (_dev(mu), _dev(var)), [0.1, 0.9], ctx=ctx).cpu().numpy()
        assert np.isfinite(c[0]) and np.isfinite(s[0]) and np.isfinite(q[0]).all()
        assert np.isnan(c[1:]).all() and np.isnan(s[1:]).all() and np.isnan(q[1:]).all()
    mu2, var2 = np.array([[0.0, 0.0], [0.0, nan], [0.0, 0.0]]), np.array([[1.0, 1.0], [1.0, 1.0], [1.0, -2.0]])
    c, s = (o.cpu().numpy() for o in A.predictive_cdf(het, (_dev(mu2), _dev(var2)), _dev(np.zeros(3)), ctx=ctx))
    assert abs(c[0] - 0.5) <= 1e-15 and abs(s[0] - 0.5) <= 1e-15 and np.isnan(c[1:]).all() and np.isnan(s[1:]).all()
    # a prob outside (0, 1) or NaN: NaN in that column
    one = (_dev(np.array([0.3])), _dev(np.array([0.7])))
    for lik in (st, lap, ber):
        q = A.predictive_quantile(lik, one, [0.0, 0.5, 1.0, nan, -0.1, 1.5], ctx=ctx).cpu().numpy()[0]
        assert np.isfinite(q[1]) and np.isnan(q[[0, 2, 3, 4, 5]]).all()
    # y = +-inf: 1 / 0 and 0 / 1; y = NaN: NaN
    for lik, qf in ((st, (_dev(np.full(3, 0.3)), _dev(np.full(3, 0.7)))), (lap, (_dev(np.full(3, 0.3)), _dev(np.zeros(3)))),
                    (het, (_dev(np.full((3, 2), 0.3)), _dev(np.full((3, 2), 0.7))))):
        c, s = (o.cpu().numpy() for o in A.predictive_cdf(lik, qf, _dev(np.array([inf, -inf, nan])), ctx=ctx))
        assert c[0] == 1.0 and s[0] == 0.0 and c[1] == 0.0 and s[1] == 1.0 and np.isnan(c[2]) and np.isnan(s[2])
    # Bernoulli: y = 1 is the whole mass; the quantile is 0 up to cdf(0) and 1 above
    c, s = (o.cpu().numpy() for o in A.predictive_cdf(ber, (_dev(np.zeros(2)), _dev(np.ones(2))), _dev(np.array([0, 1], dtype=np.uint8)), ctx=ctx))
    assert abs(c[0] - 0.5) <= 1e-15 and abs(s[0] - 0.5) <= 1e-15 and c[1] == 1.0 and s[1] == 0.0
    q = A.predictive_quantile(ber, (_dev(np.array([1.0])), _dev(np.array([0.0]))), [0.2, 0.3], ctx=ctx).cpu().numpy()[0]
    assert q[0] == 0.0 and q[1] == 1.0  # cdf(0) = sigma(-1) = 0.2689
    # the error codes, straight at the library
    lib, h = _ffi.quantile_lib(), ctx.bind()
    d = st.desc()
    buf = torch.zeros(8, dtype=torch.float64, device="cuda")
    P = lambda t: C.c_void_p(t.data_ptr())
    Z = C.c_void_p(0)
    cdf = lambda dd, n, m, v, y, c, s: lib.agpl_predictive_cdf(h, dd, C.c_int64(n), m, v, y, c, s)
    qt = lambda dd, n, m, v, nq, pr, q: lib.agpl_predictive_quantile(h, dd, C.c_int64(n), m, v, C.c_int32(nq), pr, q)
    b = P(buf)
    bad = _ffi.ERR_INVALID_ARGUMENT
    assert cdf(C.byref(d), 4, b, b, b, b, b) == 0 and qt(C.byref(d), 1, b, b, 2, b, b) == 0
    assert lib.agpl_predictive_cdf(Z, C.byref(d), C.c_int64(4), b, b, b, b, b) == bad
    assert lib.agpl_predictive_quantile(Z, C.byref(d), C.c_int64(1), b, b, C.c_int32(1), b, b) == bad
    assert cdf(Z, 4, b, b, b, b, b) == bad and qt(Z, 1, b, b, 1, b, b) == bad
    for args in ((Z, b, b, b, b), (b, Z, b, b, b), (b, b, Z, b, b), (b, b, b, Z, Z)):
        assert cdf(C.byref(d), 4, *args) == bad, args
    assert cdf(C.byref(d), 4, b, b, b, b, Z) == 0 and cdf(C.byref(d), 4, b, b, b, Z, b) == 0  # either output alone
    for m, v, pr, q in ((Z, b, b, b), (b, Z, b, b), (b, b, Z, b), (b, b, b, Z)):
        assert qt(C.byref(d), 1, m, v, 1, pr, q) == bad
    assert cdf(C.byref(d), -1, b, b, b, b, b) == bad and qt(C.byref(d), -1, b, b, 1, b, b) == bad
    assert qt(C.byref(d), 1, b, b, 0, b, b) == bad and qt(C.byref(d), 1, b, b, 17, b, b) == bad
    assert b"nq" in _ffi.lib().agpl_last_error(h)
    # n = 0: success, nothing written, no pointer needed
    buf.fill_(7.0)
    assert cdf(C.byref(d), 0, Z, Z, Z, b, b) == 0 and qt(C.byref(d), 0, Z, Z, 1, Z, Z) == 0
    ctx.synchronize()
    assert (buf == 7.0).all()
    # parameters outside the descriptor's domain
    for lik_bad in (A.StudentTLikelihood(3.0, 1.0), A.LaplaceLikelihood(1.0), A.HeteroscedasticGaussianLikelihood(2.0)):
        dd = lik_bad.desc()
        dd.p[0] = -1.0
        assert cdf(C.byref(dd), 4, b, b, b, b, b) == bad and qt(C.byref(dd), 1, b, b, 1, b, b) == bad
    dd = A.StudentTLikelihood(0.1, 1.0).desc()  # nu below what the rule's nodes hold: refused, not cut
    assert cdf(C.byref(dd), 4, b, b, b, b, b) == bad and qt(C.byref(dd), 1, b, b, 1, b, b) == bad
    # categorical kinds: no order; refused before any device work by the operators, and by the library
    for cat in (A.CategoricalLikelihood(3), A.CategoricalLikelihood(3, bijective=True)):
        with pytest.raises(A.ArgumentError):
            A.predictive_cdf(cat, (buf, buf), buf, ctx=ctx)
        with pytest.raises(A.ArgumentError):
            A.predictive_quantile(cat, (buf, buf), [0.5], ctx=ctx)
        dc = cat.desc()
        assert cdf(C.byref(dc), 1, b, b, b, b, b) == bad and qt(C.byref(dc), 1, b, b, 1, b, b) == bad
    # counts: y < 0 gives cdf 0, sf 1; cdf(y) - cdf(y - 1) is the mass function (agpl_predictive's log p)
    for cnt in (A.PoissonLikelihood(3.0), A.NegativeBinomialLikelihood(2.0)):
        qf = (_dev(np.array([0.3, 0.3, -1.0, 0.3])), _dev(np.array([0.7, 0.0, 2.0, 0.7])))
        y = np.array([4, 4, 2, -1], dtype=np.int32)
        c1, s1 = (o.cpu().numpy() for o in A.predictive_cdf(cnt, qf, _dev(y), ctx=ctx))
        c0, _ = (o.cpu().numpy() for o in A.predictive_cdf(cnt, qf, _dev(y - 1), ctx=ctx))
        lp = A.predictive(cnt, (qf[0][:3].contiguous(), qf[1][:3].contiguous()), _dev(y[:3]), ctx=ctx)[2].cpu().numpy()
        assert np.abs((c1 - c0)[:3] - np.exp(lp)).max() <= 2e-8
        assert c1[3] == 0.0 and s1[3] == 1.0 and np.abs(c1 + s1 - 1.0).max() <= 1e-9
        q = A.predictive_quantile(cnt, qf, [0.0, 0.5, nan], ctx=ctx).cpu().numpy()
        assert np.isnan(q[:, [0, 2]]).all() and (q[:, 1] == np.floor(q[:, 1])).all() and (q[:, 1] >= 0).all()


@pytest.fixture(scope="module")
def models(A):
    """One tiny SparseCAVI.from_inputs model per regression likelihood (N = 2000, M = 32, D = 1, three sweeps) and 257 new inputs."""
    import torch

    out = {}
    for name, lik in (("studentt", A.StudentTLikelihood(1.5, 0.5)), ("laplace", A.LaplaceLikelihood(0.5)),
                      ("heterogauss", A.HeteroscedasticGaussianLikelihood(2.0))):
        c = A.Context(seed=11)
        if name != "studentt":  # (no synthetic workload of their own: the Student-t inputs, a sine with noise that grows with x)
            x, _ = A.synth_xy(A.StudentTLikelihood(1.5, 0.5), seed=3, i0=0, n=2000, ctx=c)
            noise = torch.randn(x.shape, dtype=torch.float64, generator=torch.Generator().manual_seed(5)).to(x.device)
            y = (torch.sin(x) + (0.2 + 0.05 * (x + 10.0)) * noise).reshape(-1)
        else:
            x, y = A.synth_xy(lik, seed=3, i0=0, n=2000, ctx=c)
        z = torch.linspace(-10, 10, 32, dtype=torch.float64, device=x.device)
        cavi = A.SparseCAVI.from_inputs(lik, x, y, z, lengthscale=1.5 * 20.0 / 31, ctx=c)
        cavi.run(3)
        out[name] = (lik, c, cavi, torch.linspace(-10, 10, 257, dtype=torch.float64, device=x.device))
    return out


@pytest.mark.parametrize("name", ["studentt", "laplace", "heterogauss"])
def test_on_the_plan(A, models, name):
    import torch

    lik, c, cavi, x_s = models[name]
    mu, var = cavi.predict(x_s)
    qf = (mu[0].to(torch.float64), var[0].to(torch.float64)) if mu.shape[0] == 1 else (mu.t().contiguous().to(torch.float64), var.t().contiguous().to(torch.float64))
    probs = (0.025, 0.5, 0.975)
    got = cavi.predict_quantiles(x_s)
    assert got.shape == (257, 3) and torch.equal(got, A.predictive_quantile(lik, qf, probs, ctx=c))
    assert torch.equal(got, cavi.plan.predict_quantiles(lik, x_s, probs))
    y_s = got[:, 1].contiguous()
    cdf, sf = cavi.predict_cdf(x_s, y_s)
    want = A.predictive_cdf(lik, qf, y_s, ctx=c)
    assert torch.equal(cdf, want[0]) and torch.equal(sf, want[1])
    assert (cdf - 0.5).abs().max().item() <= 2e-8  # the median's distribution function
    assert torch.isfinite(got).all() and (got[:, 0] < got[:, 1]).all() and (got[:, 1] < got[:, 2]).all()
    if name == "studentt":  # nu = 1.5: the 95 % band is finite where the predictive's variance is not
        _, vy, _ = cavi.predict_y(x_s)
        assert torch.isinf(vy).all()
    assert not hasattr(A.SparseGibbs, "predict_quantiles")  # (a chain has sample_y)
