"""GPU tests of the k-means inducing inputs (include/agpl_inducing.h; csrc/agpl_inducing.hip; agpl_amd.select_inducing) against
tests/inducing_reference.py: assignment (near ties left out, at most 1e-3 of the points; exact ties exactly), the integer
accumulators against the stated fixed-point rule, their independence of the split, centres and cost over six iterations, the
stratified start, empty centres, errors, the 2-rank path and one end-to-end fit."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

import inducing_reference as R

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 20250611


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


def _lib(A):
    return A._ffi.inducing_lib()


def _ell(ell):
    ell = np.ascontiguousarray(ell, dtype=np.float64)
    return ell, ell.ctypes.data_as(C.c_void_p)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def seed(A, ctx, xd, N_total, i0, M):
    n, D = xd.shape
    z = torch.full((M, D), np.nan, dtype=torch.float64, device="cuda")
    idx = torch.full((M,), -1, dtype=torch.int64, device="cuda")
    h = ctx.bind()
    A._ffi.check(h, _lib(A).agpl_kmeans_seed(h, N_total, i0, n, M, D, xd.data_ptr() if n else None, z.data_ptr(), idx.data_ptr()))
    return z.cpu().numpy(), idx.cpu().numpy()


def step(A, ctx, xd, zd, ell, bound, N_total, acc=None, want_assign=True):
    """One agpl_kmeans_step of the points xd (device) into acc (a fresh zero one unless given): (acc tensor, assignment)."""
    n, D = xd.shape
    M = zd.shape[0]
    if acc is None:
        acc = torch.zeros((M, D + 2), dtype=torch.int64, device="cuda")
    a = torch.full((max(n, 1),), -7, dtype=torch.int32, device="cuda") if want_assign else None
    ellk, ellp = _ell(ell)
    h = ctx.bind()
    A._ffi.check(h, _lib(A).agpl_kmeans_step(h, N_total, n, M, D, xd.data_ptr() if n else None, ellp, zd.data_ptr(), bound,
                                             acc.data_ptr(), a.data_ptr() if want_assign else None))
    return acc, (a.cpu().numpy()[:n] if want_assign else None)


def centres(A, ctx, acc, zd, ell, bound, N_total):
    M, D = zd.shape
    info = torch.full((3,), np.nan, dtype=torch.float64, device="cuda")
    ellk, ellp = _ell(ell)
    h = ctx.bind()
    A._ffi.check(h, _lib(A).agpl_kmeans_centres(h, N_total, M, D, ellp, bound, acc.data_ptr(), zd.data_ptr(), info.data_ptr()))
    return info.cpu().numpy()


@pytest.fixture(scope="module")
def worlds(A, ctx):
    """Per step case, computed once: x, ell, bound, the device's own start z0 (so that the reference follows the same run), the
    reference distances' assignment."""
    out = {}
    for c in R.STEP_CASES:
        x, ell = R.data(c), R.ell_of(c)
        z0, idx = seed(A, ctx, dev(x), c.N, 0, c.M)
        a, dmin, near = R.assignment(R.sqdist(x, z0, ell))
        out[c.id] = dict(x=x, ell=ell, bound=R.bound_of(x, ell), z0=z0, idx=idx, a=a, dmin=dmin, near=near,
                         fused=R.fused_r2(x, z0, ell, a))
    return out


def _fused(w, a, n=None):
    """The fused distances of the first n points to the centres a the device chose: the shared ones, recomputed where a differs
    from the reference's choice (near ties only)."""
    n = len(a) if n is None else n
    f = w["fused"][:n].copy()
    diff = np.nonzero(a != w["a"][:n])[0]
    if len(diff):
        f[diff] = R.fused_r2(w["x"][diff], w["z0"], w["ell"], a[diff])
    return f


# ---- 1, 3: assignment and accumulators ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("c", R.STEP_CASES, ids=[c.id for c in R.STEP_CASES])
def test_assignment_and_accumulators(A, ctx, worlds, c):
    w = worlds[c.id]
    acc, a = step(A, ctx, dev(w["x"]), dev(w["z0"]), w["ell"], w["bound"], c.N)
    acc = acc.cpu().numpy()
    keep = ~w["near"]
    print(f"{c.id}: near ties left out {int(w['near'].sum())} of {c.N}")
    assert w["near"].sum() <= R.TIE_CAP * c.N
    assert np.array_equal(a[keep], w["a"][keep])
    # the accumulators are the integer sums of the stated rule under the DEVICE's own assignment, the distances fused as the header
    # states them
    want = R.accumulate(w["x"], w["ell"], a, _fused(w, a), w["bound"], c.N, c.M)
    assert acc[:, 0].sum() == c.N
    assert np.array_equal(acc, want)


def test_exact_ties_take_the_lowest_index(A, ctx):
    c = R.CASES[1]
    x = R.data(c, quarter=True)
    ell = np.ones(c.D)
    z0, _ = seed(A, ctx, dev(x), c.N, 0, c.M)
    r2 = R.sqdist(x, z0, ell)
    two = np.partition(r2, 1, axis=1)[:, :2]
    print("points with an exact tie:", int((two[:, 0] == two[:, 1]).sum()))
    acc, a = step(A, ctx, dev(x), dev(z0), ell, R.bound_of(x, ell), c.N)
    assert np.array_equal(a, np.argmin(r2, axis=1))
    # every distance is exact here, fused or not: the whole accumulator is the rule's, bit for bit
    want = R.accumulate(x, ell, a, r2[np.arange(c.N), a], R.bound_of(x, ell), c.N, c.M)
    assert np.array_equal(acc.cpu().numpy(), want)


# ---- 4: split invariance --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("c", [R.CASES[1], R.CASES[2], R.GLOBAL_ACC], ids=lambda c: c.id)
def test_accumulators_do_not_depend_on_the_split(A, ctx, worlds, c):
    w = worlds[c.id]
    xd, zd = dev(w["x"]), dev(w["z0"])
    one, a_one = step(A, ctx, xd, zd, w["ell"], w["bound"], c.N)
    tile = R.tile_points(c.D)
    cuts = [0, 1, tile + 37, c.N]  # a cut at 1, one off the tile, the end
    acc = torch.zeros_like(one)
    parts = {}
    for k in (2, 0, 1):  # in another order than the points'
        lo, hi = cuts[k], cuts[k + 1]
        _, parts[k] = step(A, ctx, xd[lo:hi].contiguous(), zd, w["ell"], w["bound"], c.N, acc=acc)
    assert np.array_equal(acc.cpu().numpy(), one.cpu().numpy())
    assert np.array_equal(np.concatenate([parts[0], parts[1], parts[2]]), a_one)


def test_tile_edges_and_empty_range(A, ctx, worlds):
    """n = 1, 255, 256, 257, one point around a workgroup's tile (1024 at D = 16, 2048 at D = 2) and n = 0: the step of the first n
    points equals the rule applied to them."""
    for c in (R.CASES[1], R.CASES[2]):
        w = worlds[c.id]
        tile = R.tile_points(c.D)
        zd = dev(w["z0"])
        for n in (0, 1, 255, 256, 257, 511, 512, 513, tile - 1, tile, tile + 1):
            acc, a = step(A, ctx, dev(w["x"][:n]), zd, w["ell"], w["bound"], c.N)
            acc = acc.cpu().numpy()
            if n == 0:
                assert not acc.any()
                continue
            keep = ~w["near"][:n]
            assert np.array_equal(a[keep], w["a"][:n][keep])
            want = R.accumulate(w["x"][:n], w["ell"], a, _fused(w, a, n), w["bound"], c.N, c.M)
            assert acc[:, 0].sum() == n and np.array_equal(acc, want), (c.id, n)


# ---- 5: centres and cost --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("c", R.LLOYD, ids=[c.id for c in R.LLOYD])
def test_centres_and_cost_follow_the_reference_run(A, ctx, worlds, c):
    w = worlds[c.id]
    x, ell, bound = w["x"], w["ell"], w["bound"]
    xd, zd = dev(x), dev(w["z0"])
    zref, costs, cref = w["z0"], [], []
    for it in range(R.NITER):
        acc, _ = step(A, ctx, xd, zd, ell, bound, c.N, want_assign=False)
        info = centres(A, ctx, acc, zd, ell, bound, c.N)
        zref, _, cost, near, empty = R.lloyd_step(x, zref, ell)
        assert near.sum() == 0 and empty == 0  # (tests/test_inducing_reference_cpu.py shows this for its own start)
        costs.append(info[2])
        cref.append(cost)
        assert info[0] == 0
    z = zd.cpu().numpy()
    print(f"{c.id}: max |z - ref| / (bound ell) = {np.max(np.abs(z - zref) / (bound * ell)):.3e}; "
          f"max rel cost error = {max(abs(a - b) / b for a, b in zip(costs, cref)):.3e}")
    assert (np.abs(z - zref) <= 1e-10 * bound * ell).all()
    assert all(b <= a for a, b in zip(costs, costs[1:])), costs
    assert all(abs(a - b) <= 1e-9 * b for a, b in zip(costs, cref))
    # the convenience call is the same run, bit for bit
    z1, info1 = A.select_inducing(dev(x), c.M, lengthscale=ell, niter=R.NITER, ctx=ctx, return_info=True)
    assert np.array_equal(z1.cpu().numpy(), z)
    assert info1["empty"] == 0 and info1["cost"] <= costs[-1] and info1["movement"] >= 0.0
    z_start = A.select_inducing(dev(x), c.M, lengthscale=ell, niter=0, ctx=ctx)
    assert np.array_equal(z_start.cpu().numpy(), w["z0"])


def test_every_point_its_own_centre(A, ctx, worlds):
    """N = M: the first step costs exactly 0 and the update returns the start rows -- to half a quantum of the fixed point, which is
    all a sum kept as rint(u 2^sx) can return (bit equality holds for niter = 0, asserted in the test above)."""
    c = R.OWN_CENTRE
    w = worlds[c.id]
    assert sorted(w["idx"]) == list(range(c.N))
    zd = dev(w["z0"])
    acc, a = step(A, ctx, dev(w["x"]), zd, w["ell"], w["bound"], c.N)
    assert np.array_equal(a, np.arange(c.N)) and np.array_equal(acc[:, 0].cpu().numpy(), np.ones(c.M, dtype=np.int64))
    info = centres(A, ctx, acc, zd, w["ell"], w["bound"], c.N)
    assert info[2] == 0.0 and info[0] == 0
    sx = R.quanta(w["bound"], c.N, c.D)[0]
    assert (np.abs(zd.cpu().numpy() - w["z0"]) <= 2.0 ** -(sx + 1) * w["ell"]).all()


# ---- 6: the start ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("c", [R.CASES[0], R.CASES[3], R.BIG_M], ids=lambda c: c.id)
def test_stratified_start(A, ctx, worlds, c):
    w = worlds[c.id]
    x, idx = w["x"], w["idx"]
    j = np.arange(c.M)
    assert np.array_equal(w["z0"], x[idx])
    assert (idx >= j * c.N // c.M).all() and (idx < (j + 1) * c.N // c.M).all()
    z_again, idx_again = seed(A, ctx, dev(x), c.N, 0, c.M)
    assert np.array_equal(idx_again, idx) and np.array_equal(z_again, w["z0"])
    other = A.Context(0, seed=SEED + 1)
    _, idx_other = seed(A, other, dev(x), c.N, 0, c.M)
    assert not np.array_equal(idx_other, idx) or c.N == c.M
    cuts = [0, 1, c.N // 2 + 3, c.N]
    total = np.zeros_like(w["z0"])
    for k in (1, 2, 0):
        zk, idxk = seed(A, ctx, dev(x[cuts[k]:cuts[k + 1]]), c.N, cuts[k], c.M)
        assert np.array_equal(idxk, idx)
        total += zk
    assert np.array_equal(total, w["z0"])


# ---- 7: an empty centre ---------------------------------------------------------------------------------------------------------------

def test_an_empty_centre_keeps_its_value(A, ctx, worlds):
    c = R.CASES[1]
    w = worlds[c.id]
    z0 = w["z0"].copy()
    z0[17] = 1.0e3
    z, info = A.select_inducing(dev(w["x"]), c.M, lengthscale=w["ell"], niter=3, z0=dev(z0), ctx=ctx, return_info=True)
    z = z.cpu().numpy()
    assert np.array_equal(z[17], z0[17]) and info["empty"] == 1
    assert not np.array_equal(z[16], z0[16])


# ---- 8: errors ------------------------------------------------------------------------------------------------------------------------

def test_errors_leave_the_context_usable(A, ctx, worlds):
    c = R.CASES[1]
    w = worlds[c.id]
    x = w["x"].copy()
    x[1234, 1] = np.nan
    with pytest.raises(A.DomainError, match=r"x\[1234\]"):
        A.select_inducing(dev(x), c.M, ctx=ctx)
    with pytest.raises(A.DomainError, match=r"x\[1234\]"):
        step(A, ctx, dev(x), dev(w["z0"]), w["ell"], w["bound"], c.N)
    zbad = w["z0"].copy()
    zbad[5, 0] = np.inf
    with pytest.raises(A.DomainError, match=r"z\[5\]"):
        step(A, ctx, dev(w["x"]), dev(zbad), w["ell"], w["bound"], c.N)
    far = w["x"].copy()
    far[77, 0] = 4.0 * w["bound"]
    with pytest.raises(A.DomainError, match=r"x\[77\].*bound"):
        step(A, ctx, dev(far), dev(w["z0"]), w["ell"], w["bound"], c.N)
    xd, zd = dev(w["x"]), dev(w["z0"])
    for bound in (0.0, -1.0, np.inf, np.nan):
        with pytest.raises(A.ArgumentError):
            step(A, ctx, xd, zd, w["ell"], bound, c.N)
    with pytest.raises(A.ArgumentError):
        step(A, ctx, xd, zd, [1.0, 0.0], w["bound"], c.N)
    with pytest.raises(A.ArgumentError):
        step(A, ctx, xd, zd, w["ell"], w["bound"], c.M - 1)  # M > N_total
    h = ctx.bind()
    ellk, ellp = _ell(w["ell"])
    acc = torch.zeros((c.M, c.D + 2), dtype=torch.int64, device="cuda")
    E = A._ffi.ERR_INVALID_ARGUMENT
    assert _lib(A).agpl_kmeans_step(h, c.N, c.N, c.M, c.D, None, ellp, zd.data_ptr(), w["bound"], acc.data_ptr(), None) == E
    assert _lib(A).agpl_kmeans_step(h, c.N, c.N, c.M, 17, xd.data_ptr(), ellp, zd.data_ptr(), w["bound"], acc.data_ptr(), None) == E
    assert _lib(A).agpl_kmeans_step(h, c.N, c.N, 2049, c.D, xd.data_ptr(), ellp, zd.data_ptr(), w["bound"], acc.data_ptr(), None) == E
    assert _lib(A).agpl_kmeans_seed(h, c.N, 10, c.N, c.M, c.D, xd.data_ptr(), zd.data_ptr(), None) == E  # range beyond N_total
    for kw in (dict(M=0), dict(M=c.N + 1), dict(M=c.M, lengthscale=-1.0), dict(M=c.M, lengthscale=[1.0, 2.0, 3.0]),
               dict(M=c.M, niter=-1), dict(M=c.M, z0=zd[:3])):
        with pytest.raises(A.ArgumentError):
            A.select_inducing(xd, ctx=ctx, **kw)
    with pytest.raises(A.ArgumentError):
        A.select_inducing(torch.zeros((10, 17), dtype=torch.float64, device="cuda"), 2, ctx=ctx)
    # the context works afterwards
    acc2, a = step(A, ctx, xd, zd, w["ell"], w["bound"], c.N)
    assert acc2[:, 0].sum().item() == c.N
    z = A.select_inducing(xd, c.M, niter=1, ctx=ctx)
    assert torch.isfinite(z).all()


# ---- 9: two ranks ---------------------------------------------------------------------------------------------------------------------

def _worker(rank, world, port, q):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    import torch
    import torch.distributed as dist

    import agpl_amd as A
    import inducing_reference as R

    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        c = R.CASES[3]
        ctx = A.Context(0, seed=SEED)
        i0, i1 = A.shard_range(c.N, rank, world)
        x = torch.from_numpy(R.data(c)[i0:i1].copy()).cuda()
        z, info = A.select_inducing(x, c.M, lengthscale=R.ell_of(c), niter=R.NITER, ctx=ctx, group=dist.group.WORLD, return_info=True)
        torch.cuda.synchronize()
        q.put((rank, z.cpu().numpy(), info))
    finally:
        dist.destroy_process_group()


@pytest.mark.timeout(300)
def test_two_ranks_end_with_the_bits_of_one_process(A, ctx, worlds):
    import torch.multiprocessing as mp

    c = R.CASES[3]
    world = 2
    port = 29700 + (os.getpid() % 1000)
    mpctx = mp.get_context("spawn")
    q = mpctx.Queue()
    procs = [mpctx.Process(target=_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = sorted([q.get(timeout=240) for _ in range(world)], key=lambda t: t[0])
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    w = worlds[c.id]
    z, info = A.select_inducing(dev(w["x"]), c.M, lengthscale=w["ell"], niter=R.NITER, ctx=ctx, return_info=True)
    for r in res:
        assert np.array_equal(r[1], z.cpu().numpy())
        assert r[2] == info


# ---- 10: end to end -------------------------------------------------------------------------------------------------------------------

def test_end_to_end_fit_on_the_chosen_inputs(A, ctx, worlds):
    c = R.CASES[3]
    w = worlds[c.id]
    x, ell = w["x"], w["ell"]
    xd = dev(x)
    z_km = A.select_inducing(xd, c.M, lengthscale=ell, niter=10, ctx=ctx)
    z_seed = A.select_inducing(xd, c.M, lengthscale=ell, niter=0, ctx=ctx)
    # the ordering is the reference's first (float64 numpy on the same inputs)
    ref_km, ref_seed = R.nystrom_residual_mean(x, z_km.cpu().numpy(), ell), R.nystrom_residual_mean(x, z_seed.cpu().numpy(), ell)
    print(f"mean Nystrom residual, float64: k-means {ref_km:.4f}, start {ref_seed:.4f}")
    assert ref_km < ref_seed
    rng = np.random.default_rng(5)
    y = dev((np.sin(x[:, 0]) + 0.3 * rng.standard_normal(c.N) > 0).astype(np.uint8))
    lik = A.BernoulliLikelihood()
    resid = {}
    for name, z in (("kmeans", z_km), ("start", z_seed)):
        plan = A.Plan.from_inputs(xd, z, ell, ctx=ctx)
        Phi = plan.features().to(torch.float64)
        resid[name] = float((1.0 - (Phi * Phi).sum(dim=1)).mean().item())
    print("mean Nystrom residual, plans:", resid)
    assert resid["kmeans"] < resid["start"]
    cavi = A.SparseCAVI.from_inputs(lik, xd, y, z_km, ell, ctx=ctx)
    cavi.run(3)
    mu, var = cavi.predict(xd[:500])
    assert torch.isfinite(mu).all() and torch.isfinite(var).all() and (var > 0).all()
