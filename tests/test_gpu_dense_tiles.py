"""The float64 tile kernels of the dense Gibbs route (csrc/agpl_dense.hip) on matrices that reach every tile of the factor.

The other dense tests above the blocking threshold use sorted squared-exponential matrices whose factor is banded: over 90 % of the
128 x 128 tiles the update kernel runs subtract exact zeros there (tests/test_dense_reference_cpu.py measures it), so a wrong tile
index, a wrong start of the second launch, a dropped 16-column stage or a panel row tile that reads the wrong U_k would pass.  Here the
prior is `exp_perm` or `wishart` (tests/dense_reference.py): O(1) entries at every index distance, every tile's contribution above
the bar.  Shapes: the smallest that reach the routes (N = 8192 is the threshold), the ragged and the odd block counts.

Bars: derived in tests/dense_reference.py -- (a) entry-wise backward error of the factor, formed from np.linalg.cholesky(K);
(b) forward error of f from the reference's own B, K and s, capped at the existing dense-step tests' flat 1e-6 max(1, max|f|):
the derived bound is a worst-case norm bound and came out above the flat bar in every case here (1.4e-4 .. 2.6e-4 for wishart
Student-t, 9e-6 for Poisson, 0.31 for exp_perm), so the flat bar is what binds.  Measured on an MI355X:
    look-ahead factor |K - LL'| / bar (a):  exp_perm 4.4e-5 (N = 8192), 5.2e-5 (9193); wishart 4.7e-4, 4.6e-4
                                            (c = 63, 48, 22, 20: almost all of it the allowance for the explicit inverses)
    dense step max|f - ref| / bar:          wishart Student-t 2.6e-8 (8192), 3.3e-8 (9216), 4.1e-8 (8492, look-ahead step);
                                            wishart Poisson 1.2e-8; exp_perm 1.0e-6     (max|f - ref| itself: 5e-14 .. 1e-12)
Wall time of the module on one MI355X: 93 s (13 s of it the first numpy Cholesky; each step case 7 to 13 s, most of it the oracle's
two numpy Cholesky factorisations of B).
"""
import ctypes as C
import time

import numpy as np
import pytest

import dense_reference as R

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

BL = R.Blocking.from_source()


@pytest.fixture(scope="module")
def A():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import __graft_entry__ as g

    g.build()
    import agpl_amd

    return agpl_amd


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    return t.detach().cpu().numpy()


def extreme_eigs(Md, Cd, iters=60):
    """(smallest, largest) eigenvalue of the SPD matrix Md with lower factor Cd, by power iteration on Md and on Md^-1.  Rayleigh
    quotients: the largest is approached from below and the smallest from above, so cond_2 is never overstated (the bar never
    widened)."""
    g = torch.Generator(device="cuda").manual_seed(1)
    v = torch.randn(Md.shape[0], 1, dtype=torch.float64, device="cuda", generator=g)
    w = v.clone()
    for _ in range(iters):
        v = Md @ v
        v /= v.norm()
        w = torch.cholesky_solve(w, Cd)
        w /= w.norm()
    return float((w.T @ Md @ w).item()), float((v.T @ Md @ v).item())


def abs_factor_norm(Cd, iters=60):
    """|| |C| |C|' ||_2 by power iteration (from below: see extreme_eigs)"""
    Ca = Cd.abs()
    a = torch.ones(Cd.shape[0], 1, dtype=torch.float64, device="cuda")
    for _ in range(iters):
        a = Ca @ (Ca.T @ a)
        a /= a.norm()
    return float((Ca.T @ a).norm() ** 2)


_refs = {}


@pytest.fixture(scope="module")
def ref():
    """(family, N) -> dict(K, Lref = np.linalg.cholesky(K), c of bar (a), extreme eigenvalues of K), computed once"""

    def get(family, N):
        if (family, N) not in _refs:
            K = R.FAMILIES[family](N)
            Lref = np.linalg.cholesky(K)
            c, parts = R.factor_margin(Lref, BL)
            _refs[(family, N)] = dict(K=K, Lref=Lref, c=c, c_parts=parts, eig=extreme_eigs(dev(K), dev(Lref)))
        return _refs[(family, N)]

    yield get
    _refs.clear()


def lower_of(Lk):
    return torch.triu(Lk).T.contiguous()  # LAPACK-lower of the column-major view = upper triangle of the row-major tensor


def check_factor(ref, got, what):
    """bar (a) on the device's factor `got` (lower, on the device) by dense_reference.check_factor, the function the CPU module's
    fault injections are rejected by; returns the worst ratio"""
    Lr = dev(ref["Lref"]).abs()
    absLL = Lr @ Lr.T
    del Lr
    Rm = dev(ref["K"]) - got @ got.T
    ok, worst, msg = R.check_factor(Rm, absLL, ref["c"], BL, xp=torch)
    print("%s: %s, c = %.4g %s" % (what, msg, ref["c"], ref["c_parts"]))
    assert ok, (what, msg)
    return worst


@pytest.mark.parametrize("family", ["exp_perm", "wishart"])
@pytest.mark.parametrize("N", [8192, 8192 + 1001])
def test_lookahead_factor_meets_the_backward_bound_on_every_tile(A, ref, family, N):
    """agpl_dense_cholesky (the look-ahead route; N = 8192: four whole panels, N = 9193: ragged last block, last update tile with
    rmax < 128, odd order): |K - L L'| <= c gamma_{n+1} |Lref| |Lref|' entry by entry, and the factor is bit-identical on a
    second call."""
    t0 = time.time()
    rf = ref(family, N)
    ctx = A.Context(0, seed=3)
    Kd = dev(rf["K"])
    L1, L2 = torch.empty_like(Kd), torch.empty_like(Kd)
    ctx.call("agpl_dense_cholesky", C.c_int64(N), C.c_void_p(Kd.data_ptr()), C.c_void_p(L1.data_ptr()))
    ctx.call("agpl_dense_cholesky", C.c_int64(N), C.c_void_p(Kd.data_ptr()), C.c_void_p(L2.data_ptr()))
    assert torch.equal(torch.triu(L1), torch.triu(L2)), "the factor differs between two calls"
    del L2, Kd
    got = lower_of(L1)
    del L1
    check_factor(rf, got, "look-ahead factor %s N = %d" % (family, N))
    print("wall %.1f s" % (time.time() - t0))


def _step_case(A, O, ref, family, N, likname, seed, sweeps=2):
    t0 = time.time()
    rf = ref(family, N)
    K = rf["K"]
    if likname == "studentt":
        lik, olik = A.StudentTLikelihood(3.5, 2.0), O.studentt(3.5, 2.0)
        y = np.random.default_rng(seed).normal(size=N)
    else:
        lik, olik = A.PoissonLikelihood(3.0), O.poisson(3.0)
        y = np.random.default_rng(seed).poisson(0.4, size=N).astype(np.int32)
    mu0 = 0.5 + 0.25 * np.cos(np.arange(N))
    dg = A.DenseGibbs(lik, dev(K), dev(y), mu0=dev(mu0), ctx=A.Context(0, seed=seed))
    # the device draws f0 with its own factor of K: check that factor against bar (a), then give it to the oracle
    got = lower_of(dg.Lk)
    check_factor(rf, got, "factor of the prior, %s N = %d" % (family, N))
    Lk = host(got)
    del got
    Kd = dev(K)
    f = np.zeros(N)
    worst, saw_zero = 0.0, False
    for sweep in range(sweeps):
        dg.sweep()
        f, d = O.dense_gibbs_step(olik, K, Lk, y, f, seed=seed, sweep=sweep, mu0=mu0)
        assert np.allclose(host(dg.omega), d["omega"], rtol=1e-6), (likname, sweep)
        if d.get("n") is not None:
            assert np.array_equal(host(dg.n), d["n"])
        # the reference's own B, r, s (float64 on the device for the O(N^3) parts: they enter the bar only through norms)
        beta, gamma = O.potential_precision(olik, y, d["omega"], d.get("n"))
        beta, gamma = beta[0], gamma[0]
        saw_zero |= bool((gamma == 0).any())
        z = O.randn(seed, 0, (sweep | 0x80000000) & 0xFFFFFFFF, 2 * N)
        sg = np.sqrt(gamma)
        f0 = Lk @ z[:N] + mu0
        with np.errstate(divide="ignore", invalid="ignore"):
            r = np.where(sg > 0, beta / sg, 0.0) - sg * f0 - z[N:]
        sgd = dev(sg)
        Bd = sgd[:, None] * Kd * sgd[None, :]
        Bd.diagonal().add_(1.0)
        Cd = torch.linalg.cholesky(Bd)
        eig_B = extreme_eigs(Bd, Cd)
        acc = abs_factor_norm(Cd)
        s = host(torch.cholesky_solve(dev(r)[:, None], Cd)[:, 0])
        nb = N - N % BL.db
        c_inv_blocks = 3.0 * 2.0 * BL.db * R.cond_of_blocks(host(Cd[:nb, :nb]), BL.db) / N
        del Bd, Cd
        bar, parts = R.step_bar(K, Lk, (rf["eig"][1], 1.0 / rf["eig"][0]), eig_B[1] / eig_B[0], acc, eig_B[1], gamma, z[:N], s,
                                c_inv_blocks, BL, f)
        err = float(np.abs(host(dg.f) - f).max())
        worst = max(worst, err / bar)
        print("%s %s N = %d sweep %d: max|f - ref| = %.3g, bar = %.3g %s, ratio %.3g, cond(B) = %.3g, derived bar: %.3g"
              % (family, likname, N, sweep, err, bar, parts, err / bar, eig_B[1] / eig_B[0], sum(parts[:3])))
        assert err <= bar, (family, likname, N, sweep, err, bar, parts)
    if likname == "poisson":
        assert saw_zero  # rows with gamma_i = 0 were among the dense rows
    print("wall %.1f s" % (time.time() - t0))
    return worst


@pytest.mark.parametrize("N", [8192, 9216])
def test_inverse_block_step_on_a_dense_prior(A, oracle, ref, N):
    """DenseGibbs.sweep() for N % 1024 == 0 (eight blocks; nine, an odd count): Student-t, wishart prior, nonzero mu0, two sweeps
    against the numpy chain on the same streams; omega at 1e-6 relative, f under bar (b)."""
    _step_case(A, oracle, ref, "wishart", N, "studentt", seed=123)


def test_inverse_block_step_on_the_exp_perm_prior(A, oracle, ref):
    """The same with exp_perm as the prior: a larger cond_2(B), hence a larger bar; the point is that every tile is reached."""
    _step_case(A, oracle, ref, "exp_perm", 8192, "studentt", seed=321)


def test_inverse_block_step_with_zero_precision_rows(A, oracle, ref):
    """Poisson with y_i = 0 points: gamma_i = 0 rows of B are rows of a dense matrix here."""
    _step_case(A, oracle, ref, "wishart", 8192, "poisson", seed=606)


def test_lookahead_step_on_a_dense_prior(A, oracle, ref):
    """The step's fallback for N % 1024 != 0 (blocked_potrf + blocked_potrs_vec), N = 8192 + 300."""
    _step_case(A, oracle, ref, "wishart", 8192 + 300, "studentt", seed=99)
