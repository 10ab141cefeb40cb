"""GPU tests of the greedy conditional-variance inducing inputs (include/agpl_greedy.h; csrc/agpl_greedy.hip;
agpl_amd.select_inducing_greedy) against tests/greedy_reference.py: one step per entry under a derived bar, byte-identity over splits,
grids and calls, exact ties, whole runs (exact indices where the reference's residual gaps allow it, a float64 replay of the device's
own pivots everywhere), the ends, errors, the 2-rank path and one end-to-end fit."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

import greedy_reference as G
import inducing_reference as R

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 20250920
EPS = 2.0 ** -52
NONE = np.iinfo(np.int64).max
KINDS = {"se": 0, "matern12": 1, "matern32": 2, "matern52": 3}
FIVE = ["se", "matern12", "matern32", "matern52", ("rq", 1.5)]


def constant(name):
    src = open(os.path.join(ROOT, "augmentedgplikelihoods.jl_amd", "csrc", "agpl_greedy.hip")).read()
    return int(re.search(r"^\s*constexpr\s+int\s+" + name + r"\s*=\s*(\d+)\s*;", src, flags=re.M).group(1))


TILE, UNROLL, PARTIALS = constant("kGvTile"), constant("kGvUnroll"), constant("kGvPartials")
STEP_N = [1, TILE - 1, TILE + 1, 3 * TILE + 17]
STEP_J = [0, 1, UNROLL - 1, UNROLL, UNROLL + 1, 37]


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
    return A.Context(0, seed=SEED)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def kind_of(kernel):
    return (KINDS[kernel], 0.0) if isinstance(kernel, str) else (4, float(kernel[1]))


def nbytes(A, n, Mmax):
    b = C.c_int64()
    assert A._ffi.greedy_lib().agpl_greedy_bytes(n, Mmax, C.byref(b)) == 0
    return b.value


class Range:
    """The work area of a range of points, its regions as the header lays them out."""

    def __init__(self, A, x_local, Mmax):
        self.n, self.Mmax = int(x_local.shape[0]), Mmax
        self.bytes = nbytes(A, self.n, Mmax)
        self.work = torch.zeros(self.bytes // 8, dtype=torch.int64, device="cuda")
        f = self.work.view(torch.float64)
        self.cols = f[:Mmax * self.n].view(Mmax, self.n)
        self.d = f[Mmax * self.n:(Mmax + 1) * self.n]
        self.x = dev(x_local) if self.n else None

    def xp(self):
        return self.x.data_ptr() if self.n else None


def run_step(A, ctx, rng_, N_total, i0, kernel, ell, variance, j, p, pivot, trace=None):
    """agpl_greedy_step of the range `rng_` (its cols[:j] and d already set): (column j, new d, candidate record, trace tensor)."""
    lib, h = A._ffi.greedy_lib(), ctx.bind()
    D = len(ell)
    kind, param = kind_of(kernel)
    ellh = np.ascontiguousarray(ell, dtype=np.float64)
    index, rec = dev(np.array([p], dtype=np.int64)), dev(np.asarray(pivot, dtype=np.float64))
    cand = torch.full((2,), -5, dtype=torch.int64, device="cuda")
    if trace is None:
        trace = torch.zeros(rng_.Mmax, dtype=torch.int64, device="cuda")
    A._ffi.check(h, lib.agpl_greedy_step(h, N_total, i0, rng_.n, rng_.Mmax, D, kind, param, j, rng_.xp(), ellh.ctypes.data_as(C.c_void_p),
                                         variance, index.data_ptr(), rec.data_ptr(), rng_.work.data_ptr(), rng_.bytes, cand.data_ptr(),
                                         trace.data_ptr()))
    return rng_.cols[j].cpu().numpy(), rng_.d.cpu().numpy(), cand.cpu().numpy(), trace


# ---- 1: one step against the reference ------------------------------------------------------------------------------------------------

STEP_ELL = {1: (0.35,), 3: (3.0, 6.0, 1.5), 16: tuple(2.0 + 0.25 * k for k in range(16))}
_WORLDS = {}


def step_world(D, kernel):
    """Per (D, kind), computed once: 3 kGvTile + 17 points, the reference's first 38 picks, the state before each."""
    key = (D, str(kernel))
    if key not in _WORLDS:
        c = G.Case("step", STEP_N[-1], 38, D, kernel, 1.7, STEP_ELL[D], 1e-6)
        x, ell = G.data(c), G.ell_of(c)
        r = G.run(x, ell, kernel, c.variance, c.M, c.threshold)
        before, cols, _ = G.replay(x, ell, kernel, c.variance, r["indices"])
        _WORLDS[key] = dict(c=c, x=x, ell=ell, idx=r["indices"], before=before, cols=cols)
    return _WORLDS[key]


@pytest.mark.parametrize("kernel", FIVE, ids=[str(k) for k in FIVE])
@pytest.mark.parametrize("D", [1, 3, 16])
def test_one_step_against_the_reference(A, ctx, D, kernel):
    """Column j and the new d, per entry.  The column's bar (j + 32) 2^-52 (|k| + sum_t |cols[t][i] cols[t][p]|) / sqrt(d_p) is
    derived: one rounding per fused multiply-add plus the rule's few operations.  d' = d - c^2 carries it as 2 |c| bar + bar^2, plus
    two roundings of its own, 2^-51 (d + c^2).  Measured worst ratio to the bar on one MI355X: column 0.98 (squared exponential, D = 16, j = 0: far points, where exp turns the
    rounding of r^2 into r^2 / 2 times as much in k, in the device and in the float64 yardstick alike; 0.53 at most elsewhere), d 0.45."""
    w = step_world(D, kernel)
    c, x, ell, N = w["c"], w["x"], w["ell"], STEP_N[-1]
    assert len(w["idx"]) == 38
    worst_c = worst_d = 0.0
    for j in STEP_J:
        p, d_old = int(w["idx"][j]), w["before"][j]
        assert d_old[p] >= 1e-3 * c.variance  # (the reference's own pivot: the bar's 1 / sqrt(d_p) stays moderate)
        col, dn, mag = G.step(x, ell, kernel, c.variance, w["cols"][:j], d_old, p)
        pivot = np.concatenate([x[p], [d_old[p]], w["cols"][:j, p]])
        for n in STEP_N:  # the first n points as a range of the N: the pivot may lie outside it
            rg = Range(A, x[:n], 40)
            rg.cols[:j] = dev(w["cols"][:j, :n])
            rg.d.copy_(dev(d_old[:n]))
            got_c, got_d, cand, trace = run_step(A, ctx, rg, N, 0, kernel, ell, c.variance, j, p, pivot)
            bar_c = (j + 32) * EPS * mag[:n] / np.sqrt(d_old[p])
            bar_d = 2.0 * np.abs(col[:n]) * bar_c + bar_c ** 2 + 2.0 * EPS * (d_old[:n] + col[:n] ** 2)
            rc, rd = np.abs(got_c - col[:n]) / bar_c, np.abs(got_d - dn[:n]) / bar_d
            worst_c, worst_d = max(worst_c, rc.max()), max(worst_d, rd.max())
            assert (rc <= 1.0).all() and (rd <= 1.0).all(), (j, n, rc.max(), rd.max())
            if p < n:
                assert got_d[p] == 0.0
            # the candidate record and the trace are those of the device's own d
            assert cand[0] == got_d.view(np.int64).max() and cand[1] == int(np.argmax(got_d))
            assert int(trace[j].item()) == G.trace_word(got_d, c.variance, N) and int(trace.abs().sum().item()) == abs(int(trace[j].item()))
    print(f"D={D} {kernel}: worst |column - ref| / bar = {worst_c:.3e}, worst |d - ref| / bar = {worst_d:.3e}")


# ---- 2: split independence ------------------------------------------------------------------------------------------------------------

def synthetic_state(n, D, j, seed):
    """A state for byte-identity checks: any finite numbers do (nothing is compared with a reference)."""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((n, D))
    cols = 0.2 * rng.standard_normal((j, n))
    d = rng.uniform(0.5, 1.5, size=n)
    return x, cols, d


def split_step(A, ctx, x, cols, d, cuts, kernel, ell, variance, j, p, order=None):
    """The step over the ranges [cuts[k], cuts[k + 1]): (column, d, combined candidate record, trace word)."""
    N = x.shape[0]
    pivot = np.concatenate([x[p], [d[p]], cols[:j, p]])
    trace = torch.zeros(j + 1, dtype=torch.int64, device="cuda")
    col, dn, cands = np.zeros(N), np.zeros(N), []
    for k in (order or range(len(cuts) - 1)):
        lo, hi = cuts[k], cuts[k + 1]
        rg = Range(A, x[lo:hi], j + 1)
        if hi > lo:
            rg.cols[:j] = dev(cols[:, lo:hi])
            rg.d.copy_(dev(d[lo:hi]))
        col[lo:hi], dn[lo:hi], cand, _ = run_step(A, ctx, rg, N, lo, kernel, ell, variance, j, p, pivot, trace=trace)
        if hi == lo:
            assert tuple(cand) == (-1, NONE)
        cands.append(cand)
    top = max(c[0] for c in cands)
    return col, dn, (top, min(c[1] for c in cands if c[0] == top)), int(trace[j].item())


def test_the_step_does_not_depend_on_the_split_or_the_call(A, ctx):
    n, D, j = 3 * TILE + 17, 3, UNROLL + 3
    x, cols, d = synthetic_state(n, D, j, 5)
    ell, p = np.array([1.0, 2.0, 0.5]), TILE + 5
    one = split_step(A, ctx, x, cols, d, [0, n], "matern52", ell, 1.5, j, p)
    again = split_step(A, ctx, x, cols, d, [0, n], "matern52", ell, 1.5, j, p)
    cut = split_step(A, ctx, x, cols, d, [0, 1, TILE - 1, TILE + 1, TILE + 1, n], "matern52", ell, 1.5, j, p, order=[4, 0, 3, 2, 1])
    for other in (again, cut):
        assert one[0].tobytes() == other[0].tobytes() and one[1].tobytes() == other[1].tobytes()
        assert one[2] == other[2] and one[3] == other[3]
    assert one[1][p] == 0.0 and one[2] == (one[1].view(np.int64).max(), int(np.argmax(one[1])))


def test_more_tiles_than_one_stride_of_the_grid(A, ctx):
    n, D, j = (PARTIALS + 3) * TILE + 5, 1, UNROLL + 1
    x, cols, d = synthetic_state(n, D, j, 6)
    ell, p = np.array([0.7]), n - 3
    one = split_step(A, ctx, x, cols, d, [0, n], "se", ell, 1.0, j, p)
    two = split_step(A, ctx, x, cols, d, [0, PARTIALS * TILE // 2 + 7, n], "se", ell, 1.0, j, p)  # each inside one stride
    assert one[0].tobytes() == two[0].tobytes() and one[1].tobytes() == two[1].tobytes() and one[2:] == two[2:]
    assert one[2] == (one[1].view(np.int64).max(), int(np.argmax(one[1])))
    assert one[3] == G.trace_word(one[1], 1.0, n)


# ---- 3: exact ties --------------------------------------------------------------------------------------------------------------------

def test_exact_ties_take_the_lowest_index(A, ctx):
    c = G.BY_ID["m32-n2049-m120-d3"]
    x, ell = G.data(c).copy(), G.ell_of(c)
    lows = [0, 27, 38, TILE - 7, TILE - 4, 1500]  # i and i + 7: two pairs across the tile edge
    for i in lows:
        x[i + 7] = x[i]
    z, info = A.select_inducing_greedy(dev(x), c.M, lengthscale=ell, variance=c.variance, kernel=c.kernel, threshold=c.threshold,
                                       ctx=ctx, return_info=True)
    idx = info["indices"].tolist()
    assert len(set(idx)) == len(idx) == c.M
    assert idx[0] == 0  # every d is the variance: the lowest index
    picked = [i for i in lows if i in idx]
    print("twins whose lower index was picked:", picked)
    assert 0 in picked and len(picked) >= 3
    for i in lows:  # a twin's d equals the other's bit for bit until that one is picked, and is rounding residue afterwards
        assert i + 7 not in idx
    # the candidate record: two equal maxima in different tiles, the lower index reported
    n, D, j = 2 * TILE + 9, 2, 3
    xs, cols, d = synthetic_state(n, D, j, 8)
    for lo, hi in ((TILE - 2, TILE + 5), (40, 47)):
        xs[hi], cols[:, hi], d[hi] = xs[lo], cols[:, lo], d[lo]
    d[[TILE - 2, TILE + 5]] = 3.0
    out = split_step(A, ctx, xs, cols, d, [0, n], "se", np.ones(D), 1.0, j, 11)
    assert out[1][TILE - 2] == out[1][TILE + 5] == out[1].max() and out[2][1] == TILE - 2
    assert out[1][40] == out[1][47]


# ---- 4, 5: whole runs -----------------------------------------------------------------------------------------------------------------

BIG = G.Case("m12-n3000-m2048-d1", 3000, 2048, 1, "matern12", 1.3, (0.05,), 1e-6)  # the largest M


def device_run(A, ctx, c):
    return A.select_inducing_greedy(dev(G.data(c)), c.M, lengthscale=G.ell_of(c), variance=c.variance, kernel=c.kernel,
                                    threshold=c.threshold, ctx=ctx, return_info=True)


QUALIFYING = [c for c in G.CASES if c.kernel in ("matern12", "matern32", "matern52")]


@pytest.mark.parametrize("c", QUALIFYING, ids=[c.id for c in QUALIFYING])
def test_whole_runs_pick_the_reference_indices(A, ctx, c):
    r = G.run_case(c)
    assert G.qualifies(r)  # (tests/test_greedy_reference_cpu.py: at least three such cases over three kinds)
    z, info = device_run(A, ctx, c)
    assert info["selected"] == len(r["indices"]) and np.array_equal(info["indices"], r["indices"])
    assert np.array_equal(z.cpu().numpy(), G.data(c)[r["indices"]])
    quantum = 2.0 ** -G.trace_shift(c.N)
    em = np.abs(info["max_residual"] - r["max_residual"]) / r["max_residual"]
    et = np.abs(info["trace"] - r["trace"]) - 0.5 * c.N * quantum
    print(f"{c.id}: max rel error of max_residual {em.max():.3e}, of the trace {(np.abs(info['trace'] - r['trace']) / r['trace']).max():.3e}")
    assert (em <= 1e-10).all() and (et <= 1e-10 * r["trace"]).all()


@pytest.mark.parametrize("c", G.CASES + [BIG], ids=[c.id for c in G.CASES + [BIG]])
def test_whole_runs_follow_a_float64_replay_of_their_own_pivots(A, ctx, c):
    """At every step the device's pivot holds the replay's maximum to 1e-10 variance and the device's max_residual is the replay's d
    there to 1e-10; it stopped exactly where the replay's maximum falls to the threshold.  The 1e-10 is derived: the column's error
    (j + 32) 2^-52 scale / sqrt(d_p) at d_p >= 1e-6 variance and j <= 300 gives about 2e-13 variance in d, taken with a margin of 500.
    Measured worst on one MI355X: no shortfall of the device's pivot at all (0.0 in all eight cases) and 3.2e-15 (max_residual)."""
    x, ell = G.data(c), G.ell_of(c)
    z, info = device_run(A, ctx, c)
    idx, m = info["indices"], info["selected"]
    assert 1 <= m <= c.M and len(set(idx.tolist())) == m and np.array_equal(z.cpu().numpy(), x[idx])
    before, _, last = G.replay(x, ell, c.kernel, c.variance, idx)
    at = before[np.arange(m), idx]
    short = (before.max(axis=1) - at) / c.variance
    err = np.abs(info["max_residual"] - at / c.variance)
    print(f"{c.id}: m = {m}; worst shortfall of the device's pivot {short.max():.3e} variance; worst |max_residual - replay| {err.max():.3e}")
    assert (short <= 1e-10).all() and (err <= 1e-10).all()
    assert (np.diff(info["max_residual"]) <= 0).all() and (np.diff(info["trace"]) < 0).all()
    assert (at > c.threshold * c.variance).all()
    if m < c.M:
        assert last.max() <= c.threshold * c.variance
    quantum = 2.0 ** -G.trace_shift(c.N)
    assert abs(info["trace"][-1] - last.sum() / c.variance) <= 0.5 * c.N * quantum + 1e-10 * info["trace"][-1] + 1e-10 * c.N


# ---- 6: ends --------------------------------------------------------------------------------------------------------------------------

def raw_select(A, ctx, x, M, kernel, ell, variance, threshold, work_bytes=None, D=None, kind=None, param=None):
    """agpl_select_inducing_greedy itself: (status, z [M, D], idx [M], info [1 + 2 M])."""
    lib, h = A._ffi.greedy_lib(), ctx.bind()
    N, Dx = x.shape
    k, pr = kind_of(kernel)
    ellh = np.ascontiguousarray(ell, dtype=np.float64)
    nb = nbytes(A, N, min(max(M, 1), 2048))
    work = torch.zeros(nb // 8, dtype=torch.int64, device="cuda")
    Mz = min(max(M, 1), 4096)
    z = torch.full((Mz, Dx), np.nan, dtype=torch.float64, device="cuda")
    idx = torch.full((Mz,), -3, dtype=torch.int64, device="cuda")
    info = torch.full((1 + 2 * Mz,), np.nan, dtype=torch.float64, device="cuda")
    rc = lib.agpl_select_inducing_greedy(h, N, M, Dx if D is None else D, k if kind is None else kind, pr if param is None else param,
                                         dev(x).data_ptr(), ellh.ctypes.data_as(C.c_void_p), variance, threshold, work.data_ptr(),
                                         nb if work_bytes is None else work_bytes, z.data_ptr(), idx.data_ptr(), info.data_ptr())
    return rc, z.cpu().numpy(), idx.cpu().numpy(), info.cpu().numpy()


def test_ends(A, ctx):
    # M > N: every point once
    N, M = 50, 64
    x = (np.arange(N, dtype=np.float64) * 1.25)[:, None]
    z, info = A.select_inducing_greedy(dev(x), M, lengthscale=1.0, variance=2.0, kernel="matern12", ctx=ctx, return_info=True)
    assert info["selected"] == N and sorted(info["indices"].tolist()) == list(range(N)) and tuple(z.shape) == (N, 1)
    assert info["trace"][-1] == 0.0
    # a threshold of 0.5 stops early; rows beyond m are zero
    c = G.BY_ID["m32-n2049-m120-d3"]
    xc = G.data(c)
    rc, z, idx, info = raw_select(A, ctx, xc, c.M, c.kernel, G.ell_of(c), c.variance, 0.5)
    m = int(info[0])
    ref = G.run(xc, G.ell_of(c), c.kernel, c.variance, c.M, 0.5)
    assert rc == 0 and 1 <= m < c.M and m == len(ref["indices"]) and np.array_equal(idx[:m], ref["indices"])
    assert np.array_equal(z[:m], xc[idx[:m]]) and not z[m:].any() and not idx[m:].any()
    assert not info[1 + m:1 + c.M].any() and not info[1 + c.M + m:].any() and (info[1:1 + m] > 0.5).all()
    assert ref["last"] <= 0.5 - 1e-9  # (the margin of the stop, in the reference)


# ---- 7: errors ------------------------------------------------------------------------------------------------------------------------

def test_errors_leave_the_context_usable(A, ctx):
    c = G.CASES[0]
    x, ell = G.data(c), G.ell_of(c)
    E = A._ffi.ERR_INVALID_ARGUMENT
    bad = x.copy()
    bad[123, 0] = np.nan
    with pytest.raises(A.DomainError, match=r"x\[123\]"):
        A.select_inducing_greedy(dev(bad), c.M, lengthscale=ell, kernel=c.kernel, ctx=ctx)
    ok = lambda: raw_select(A, ctx, x, c.M, c.kernel, ell, c.variance, c.threshold)
    assert ok()[0] == 0
    for kw in (dict(threshold=0.0), dict(threshold=1.0), dict(kind=7), dict(kind=4, param=0.0), dict(kind=4, param=-1.0), dict(D=17),
               dict(M=2049), dict(M=0), dict(work_bytes=nbytes(A, c.N, c.M) - 8), dict(variance=0.0)):
        a = dict(M=c.M, variance=c.variance, threshold=c.threshold)
        a.update({k: v for k, v in kw.items() if k in a})
        rest = {k: v for k, v in kw.items() if k not in a}
        assert raw_select(A, ctx, x, a["M"], c.kernel, ell, a["variance"], a["threshold"], **rest)[0] == E, kw
        rc, _, idx, info = ok()  # the next call succeeds
        assert rc == 0 and int(info[0]) == c.M and idx[0] == 0
    rc = raw_select(A, ctx, x, c.M, c.kernel, ell, c.variance, c.threshold, work_bytes=16)[0]
    assert rc == E
    xd = dev(x)
    for kw in (dict(M=0), dict(M=2049), dict(M=4, threshold=0.0), dict(M=4, kernel="cubic"), dict(M=4, kernel=("rq", -1.0)),
               dict(M=4, variance=-1.0), dict(M=4, lengthscale=[1.0, 2.0])):
        with pytest.raises(A.ArgumentError):
            A.select_inducing_greedy(xd, ctx=ctx, **kw)
    with pytest.raises(A.ArgumentError):
        A.select_inducing_greedy(torch.zeros((10, 17), dtype=torch.float64, device="cuda"), 2, ctx=ctx)
    z = A.select_inducing_greedy(xd, c.M, lengthscale=ell, variance=c.variance, kernel=c.kernel, ctx=ctx)
    assert np.array_equal(z.cpu().numpy(), x[G.run_case(c)["indices"]])


# ---- 8: two ranks ---------------------------------------------------------------------------------------------------------------------

TWO_RANK = "rq-n1500-m100-d1"  # ends by the threshold: the stop is shared too


def _worker(rank, world, port, q):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    import torch
    import torch.distributed as dist

    import agpl_amd as A
    import greedy_reference as G

    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        c = G.BY_ID[TWO_RANK]
        ctx = A.Context(0, seed=SEED)
        i0, i1 = A.shard_range(c.N, rank, world)
        x = torch.from_numpy(G.data(c)[i0:i1].copy()).cuda()
        z, info = A.select_inducing_greedy(x, c.M, lengthscale=G.ell_of(c), variance=c.variance, kernel=c.kernel, threshold=c.threshold,
                                           ctx=ctx, group=dist.group.WORLD, return_info=True)
        torch.cuda.synchronize()
        q.put((rank, z.cpu().numpy(), info))
    finally:
        dist.destroy_process_group()


@pytest.mark.timeout(300)
def test_two_ranks_end_with_the_bits_of_one_process(A, ctx):
    import torch.multiprocessing as mp

    c = G.BY_ID[TWO_RANK]
    world = 2
    port = 29800 + (os.getpid() % 1000)
    mpctx = mp.get_context("spawn")
    q = mpctx.Queue()
    procs = [mpctx.Process(target=_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = sorted([q.get(timeout=240) for _ in range(world)], key=lambda t: t[0])
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    z, info = device_run(A, ctx, c)
    assert info["selected"] < c.M
    for r in res:
        assert r[1].tobytes() == z.cpu().numpy().tobytes()
        assert r[2]["selected"] == info["selected"]
        for k in ("indices", "max_residual", "trace"):
            assert r[2][k].dtype == info[k].dtype and r[2][k].tobytes() == info[k].tobytes(), k


# ---- 9: end to end --------------------------------------------------------------------------------------------------------------------

def test_end_to_end_fit_on_the_chosen_inputs(A, ctx):
    c = R.CASES[3]
    x, ell = R.data(c), R.ell_of(c)
    xd = dev(x)
    z_gv, info = A.select_inducing_greedy(xd, c.M, lengthscale=ell, ctx=ctx, return_info=True)
    assert info["selected"] == c.M
    z_km = A.select_inducing(xd, c.M, lengthscale=ell, niter=10, ctx=ctx)
    z_seed = A.select_inducing(xd, c.M, lengthscale=ell, niter=0, ctx=ctx)
    zs = (("greedy", z_gv), ("kmeans", z_km), ("start", z_seed))
    # the ordering is the reference's first (float64 numpy on the same inputs, at the plans' jitter)
    ref = {name: float(G.nystrom_residual(x, z.cpu().numpy(), ell, "se", 1.0, jitter=1e-8).max()) for name, z in zs}
    print("largest Nystrom residual, float64:", ref)
    assert ref["greedy"] < ref["kmeans"] and ref["greedy"] < ref["start"]
    assert ref["greedy"] <= info["max_residual"][-1] + 1e-6  # (the residual after the last pick is below the one before it)
    resid = {}
    for name, z in zs:
        Phi = A.Plan.from_inputs(xd, z, ell, ctx=ctx).features().to(torch.float64)
        resid[name] = float((1.0 - (Phi * Phi).sum(dim=1)).max().item())
    print("largest Nystrom residual, plans:", resid)
    assert resid["greedy"] < resid["kmeans"] and resid["greedy"] < resid["start"]
    rng = np.random.default_rng(5)
    y = dev((np.sin(x[:, 0]) + 0.3 * rng.standard_normal(c.N) > 0).astype(np.uint8))
    cavi = A.SparseCAVI.from_inputs(A.BernoulliLikelihood(), xd, y, z_gv, ell, ctx=ctx)
    cavi.run(3)
    mu, var = cavi.predict(xd[:500])
    assert torch.isfinite(mu).all() and torch.isfinite(var).all() and (var > 0).all()
