"""SparseCAVI.hyper_grad(inducing=True) over a process group, in the pattern of tests/test_gpu_hyper_grad_ranks.py: two ranks on ONE
GPU (gloo exchange), each with its shard of the points and a prior mean, run three sweeps and one gradient (rank 0 adds the K_ZZ
part from the exchanged G, g; every rank its own -m h' term; one all-reduce of the D + 1 + M D numbers).  Both ranks end with the
same bits.  Against the one-process gradient: the two runs differ in how the sweep's accumulation groups the points, so their G, g
and q(v) differ at the accumulation's stated precision, 2^-22 relative (the same q(v) on two half shards agrees to 1e-10:
tests/test_gpu_zgrad.py).  The D + 1 hyperparameter derivatives keep tests/test_gpu_hyper_grad_ranks.py's bound, 2^-22 of their scale.
A component of the z gradient is a sum over one row a only and sees the K_ZZ part through L^-1 at jitter 1e-6; each run's gradient
differs from one process's by 8.427e-7 of its scale, measured on an MI355X; the bound is 4 x that (the margin covers another draw
of the data)."""
import os
import sys

import numpy as np
import pytest

import kernels_reference as K

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASE, SEED = (K.SE, 1000, 40, 3, 1, True), 3
Z_RANKS_BAR = 4 * 8.427e-07  # of the reference's scale, worst over (a, d); measured: 8.427e-7


def _flat(gr):
    return np.concatenate([gr["log_lengthscale"].numpy(), [gr["log_variance"]], gr["z"].numpy().reshape(-1)])


def _worker(rank, world, port, q):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    import torch
    import torch.distributed as dist

    import agpl_amd as A
    import test_gpu_hyper_grad as T

    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        ctx = A.Context(0, seed=17)
        lik, y, inp = T.problem(A, CASE, SEED)
        i0, i1 = A.shard_range(CASE[1], rank, world)
        cavi = T.build(A, ctx, lik, y, inp, i0, i1, group=dist.group.WORLD)
        cavi.run(3)
        q.put((rank, _flat(cavi.hyper_grad(inducing=True))))
    finally:
        dist.destroy_process_group()


@pytest.mark.timeout(300)
def test_two_ranks_give_the_one_process_gradient():
    import torch.multiprocessing as mp

    import agpl_amd as A
    import hyper_reference as HR
    import test_gpu_hyper_grad as T
    import zgrad_reference as ZR

    world, port = 2, 30800 + (os.getpid() % 1000)
    mpctx = mp.get_context("spawn")
    q = mpctx.Queue()
    procs = [mpctx.Process(target=_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = sorted([q.get(timeout=240) for _ in range(world)], key=lambda t: t[0])
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    ctx = A.Context(0, seed=17)
    lik, y, inp = T.problem(A, CASE, SEED)
    cavi = T.build(A, ctx, lik, y, inp)
    cavi.run(3)
    one = _flat(cavi.hyper_grad(inducing=True))
    cavi.accumulate()
    q_ = dict(m=T.host(cavi.m), S=T.host(cavi.S), beta=T.host(cavi.beta).astype(np.float64), gamma=T.host(cavi.gamma).astype(np.float64))
    scale = np.concatenate([HR.gradient(**q_, **inp)["scale"], ZR.gradient_z(**q_, **inp)["scale"].reshape(-1)])
    for rank, got in res:
        err = np.abs(got - one) / scale
        print("ZGRAD_RANKS", rank, err[: CASE[3] + 1], err[CASE[3] + 1:].max())
        bound = np.concatenate([np.full(CASE[3] + 1, 2.0 ** -22), np.full(CASE[2] * CASE[3], Z_RANKS_BAR)])
        assert np.all(np.abs(got - one) <= bound * scale)
    assert np.array_equal(res[0][1], res[1][1])
