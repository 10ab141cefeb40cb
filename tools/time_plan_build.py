"""Build time and peak device memory of a plan from raw inputs (Plan.from_inputs: one fused pass) against the four-step build
(se_features -> whiten_features -> nystrom_residual -> Plan) on the bench workload (z = linspace(-10, 10, M), ell = 1.5 spacing,
jitter 1e-8).  Kernel times: run it alone under `rocprofv3 --kernel-trace --stats -- python tools/time_plan_build.py ...`.

    python tools/time_plan_build.py --n 10000000 --m 512 [--kernel matern32 | --kernel rq:2.0] [--two-step] [--sweeps 10]

``--kernel`` times the fused build of another stationary kernel (include/agpl_kernels.h); the four-step comparison of ``--two-step``
is the squared exponential's only.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import agpl_amd as A  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=10_000_000)
    ap.add_argument("--m", type=int, default=512)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--two-step", action="store_true", help="also time the four-step build and compare ten sweeps' G")
    ap.add_argument("--sweeps", type=int, default=10)
    ap.add_argument("--kernel", default="se", help='se, matern12 (exponential), matern32, matern52 or rq:ALPHA')
    a = ap.parse_args()
    kernel = ("rq", float(a.kernel[3:])) if a.kernel.startswith("rq:") else a.kernel
    if a.two_step and kernel != "se":
        ap.error("--two-step compares the squared-exponential builds only")
    ctx = A.Context(0, seed=1)
    lik = A.BernoulliLikelihood()
    x, y = A.synth_xy(lik, 20240807, 0, a.n, ctx=ctx)
    z = np.linspace(-10, 10, a.m)
    ell = 1.5 * (z[1] - z[0])
    zt = torch.from_numpy(z).cuda()
    torch.cuda.synchronize()
    out = {"N": a.n, "M": a.m, "kernel": a.kernel}
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    times = []
    for _ in range(a.reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        plan = A.Plan.from_inputs(x, zt, ell, ctx=ctx, kernel=kernel)
        e1.record()
        torch.cuda.synchronize()
        times.append(e0.elapsed_time(e1))
        out["plan_bytes"] = plan.nbytes
        del plan
    out["from_inputs_ms"] = times
    out["from_inputs_peak_over_inputs_bytes"] = torch.cuda.max_memory_allocated() - base
    if a.two_step:
        torch.cuda.reset_peak_memory_stats()
        times = []
        for _ in range(a.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            _, Linv = A.sparse.whitening_matrix(np.exp(-0.5 * ((z[:, None] - z[None, :]) / ell) ** 2), 1e-8)
            Phi = A.whiten_features(A.se_features(x, zt, ell, ctx=ctx), Linv, ctx=ctx)[:, : a.m].contiguous()
            kd = A.sparse.nystrom_residual(Phi, torch.ones(a.n, device="cuda"), ctx=ctx)
            plan = A.sparse.Plan(Phi, kd, 1, ctx)
            e1.record()
            torch.cuda.synchronize()
            times.append(e0.elapsed_time(e1))
            del plan, Phi, kd
        out["two_step_ms"] = times
        out["two_step_peak_over_inputs_bytes"] = torch.cuda.max_memory_allocated() - base
        if a.sweeps:
            new = A.SparseCAVI.from_inputs(lik, x, y, zt, ell, ctx=ctx)
            new.run(a.sweeps)
            new.check()
            G_new = new.G.clone()
            del new
            _, Linv = A.sparse.whitening_matrix(np.exp(-0.5 * ((z[:, None] - z[None, :]) / ell) ** 2), 1e-8)
            Phi = A.whiten_features(A.se_features(x, zt, ell, ctx=ctx), Linv, ctx=ctx)[:, : a.m].contiguous()
            kd = A.sparse.nystrom_residual(Phi, torch.ones(a.n, device="cuda"), ctx=ctx)
            ref = A.SparseCAVI(lik, Phi, kd, y, ctx=ctx)
            del Phi
            ref.run(a.sweeps)
            ref.check()
            out["sweeps"] = a.sweeps
            out["G_rel_diff_vs_two_step"] = float(((G_new - ref.G).abs().max() / ref.G.abs().max()).item())
    print(json.dumps(out))


if __name__ == "__main__":
    main()
