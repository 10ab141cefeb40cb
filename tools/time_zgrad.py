#!/usr/bin/env python3
"""Times agpl_plan_inducing_grad (Plan.inducing_grad) next to agpl_plan_hyper_grad (Plan.hyper_grad): what the combined call, which
returns the hyperparameter derivatives and the inducing-input gradient from one pass over the points, costs against one and two
gradient passes.

    python tools/time_zgrad.py [--N 1048576] [--M 512] [--D 2] [--reps 11] [--warmup 3] [--limit 300] [--parent-lib PATH]

Bernoulli data from synth_xy (further input dimensions uniform on [-10, 10]), squared-exponential kernel, z on a regular grid over
the inputs' box with the lengthscale 0.7 grid steps, q(v) after two sweeps, G and g given.  Times are device time between two events
around a call, medians of `reps` after `warmup` calls.  `--parent-lib`: a libagpl_hyper.so built from another commit, placed in the
package directory (it resolves libagpl.so next to itself); its agpl_plan_hyper_grad is timed on the same plan.  Under
`rocprofv3 --kernel-trace --stats -- python tools/time_zgrad.py` the per-kernel times separate the points kernel with and without
its second phase.  One process; every step runs under an alarm of `--limit` seconds whose default action ends the process, so
nothing is started on the device after a step that hangs.  Prints one JSON line."""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import agpl_amd as A  # noqa: E402
from agpl_amd import _ffi  # noqa: E402
from time_hyper_grad import step, timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--N", type=int, default=1 << 20)
    ap.add_argument("--M", type=int, default=512)
    ap.add_argument("--D", type=int, default=2)
    ap.add_argument("--reps", type=int, default=11)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--limit", type=int, default=300, help="seconds per step")
    ap.add_argument("--parent-lib", default=None)
    a = ap.parse_args()
    torch.cuda.set_device(0)
    ctx = A.Context(0, seed=1)
    N, M, D = a.N, a.M, a.D
    lik = A.BernoulliLikelihood()
    with step(a.limit):
        x1, y = A.synth_xy(lik, 5, 0, N, ctx=ctx)
        x = x1.to(torch.float64).reshape(N, 1)
        if D > 1:
            g = torch.Generator(device="cuda").manual_seed(7)
            x = torch.cat([x, -10 + 20 * torch.rand(N, D - 1, dtype=torch.float64, device="cuda", generator=g)], 1).contiguous()
        side = int(np.ceil(M ** (1.0 / D)))
        axis = torch.linspace(-10, 10, side, dtype=torch.float64, device="cuda")
        z = torch.cartesian_prod(*([axis] * D)).reshape(-1, D)[:M].contiguous()
        ell = 0.7 * 20.0 / (side - 1)
        cavi = A.SparseCAVI.from_inputs(lik, x, y, z, ell, jitter=1e-6, ctx=ctx, keep_points=True, keep_inputs=True)
        cavi.run(2)
        cavi.accumulate()
        cavi.check()
    p = cavi.plan
    args = (x, cavi.beta, cavi.gamma, None, cavi.G, cavi.g)
    out = {"N": N, "M": M, "Mp": p.Mp, "D": D, "reps": a.reps, "warmup": a.warmup, "lengthscale": ell}
    with step(a.limit):
        out["hyper_grad_ms"] = timed(lambda: p.hyper_grad(*args), a.reps, a.warmup)
        out["inducing_grad_with_theta_ms"] = timed(lambda: p.inducing_grad(*args, with_theta=True), a.reps, a.warmup)
        out["inducing_grad_ms"] = timed(lambda: p.inducing_grad(*args), a.reps, a.warmup)
    if a.parent_lib:
        lib = C.CDLL(os.path.abspath(a.parent_lib))
        lib.agpl_plan_hyper_grad.restype = C.c_int32
        lib.agpl_plan_hyper_grad.argtypes = [C.c_void_p, C.c_int64] + [C.c_void_p] * 7
        grad = torch.empty(D + 1, dtype=torch.float64, device="cuda")

        def parent():
            ctx.bind()
            _ffi.check(ctx._h, lib.agpl_plan_hyper_grad(p._h, N, x.data_ptr(), None, cavi.beta.data_ptr(), cavi.gamma.data_ptr(),
                                                         cavi.G.data_ptr(), cavi.g.data_ptr(), grad.data_ptr()))

        with step(a.limit):
            out["parent_hyper_grad_ms"] = timed(parent, a.reps, a.warmup)
            out["parent_equals_hyper_grad"] = bool(torch.equal(grad, p.hyper_grad(*args)))
    out["ratio_to_hyper_grad"] = out["inducing_grad_with_theta_ms"][0] / out["hyper_grad_ms"][0]
    print(json.dumps(out))


if __name__ == "__main__":
    main()
