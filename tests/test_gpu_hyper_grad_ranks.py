"""SparseCAVI.hyper_grad over a process group: two ranks on ONE GPU (gloo exchange, as tests/test_gpu_distributed.py), each with its
shard of the points and a prior mean, run three sweeps and one hyper_grad (rank 0 adds the K_ZZ part from the exchanged G, g; every rank its own -m h' term; one
all-reduce).  Both ranks end with the same bits, and with the one-process gradient to 2^-22 of the reference's scale: the two runs
differ in how the sweep's accumulation groups the points into float32 partial sums of split-float16 products, whose stated
precision (include/agpl.h) is 2^-22 relative, so their G, g and q(v) -- in which the gradient is smooth -- differ at that level
and no lower (the same q(v) on two half shards agrees to 1e-10: tests/test_gpu_hyper_grad.py)."""
import os
import sys

import numpy as np
import pytest

import kernels_reference as K

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASE, SEED = (K.SE, 1000, 40, 3, 1, True), 3


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
        gr = cavi.hyper_grad()
        q.put((rank, np.concatenate([gr["log_lengthscale"].numpy(), [gr["log_variance"]]])))
    finally:
        dist.destroy_process_group()


@pytest.mark.timeout(300)
def test_two_ranks_give_the_one_process_gradient():
    import torch.multiprocessing as mp

    import agpl_amd as A
    import test_gpu_hyper_grad as T

    world, port = 2, 29800 + (os.getpid() % 1000)
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
    gr = cavi.hyper_grad()
    one = np.concatenate([gr["log_lengthscale"].numpy(), [gr["log_variance"]]])
    cavi.accumulate()
    scale = T.reference(cavi, inp)["scale"]
    for rank, got in res:
        print("HYPER_RANKS", rank, np.abs(got - one) / scale)
        assert np.all(np.abs(got - one) <= 2.0 ** -22 * scale)
    assert np.array_equal(res[0][1], res[1][1])
