"""Build time and peak device memory of a plan from raw inputs (Plan.from_inputs: one fused pass) against the four-step build
(se_features -> whiten_features -> nystrom_residual -> Plan) on the bench workload (z = linspace(-10, 10, M), ell = 1.5 spacing,
jitter 1e-8).  Kernel times: run it alone under `rocprofv3 --kernel-trace --stats -- python tools/time_plan_build.py ...`.

    python tools/time_plan_build.py --n 10000000 --m 512 [--kernel matern32 | --kernel rq:2.0] [--two-step] [--sweeps 10]
    python tools/time_plan_build.py --n 10000000 --m 512 --d 16 --kernel additive_se --jitter 1e-2
    python tools/time_plan_build.py --n 10000000 --m 512 --d 16 --kernel additive2_se:0.5 --jitter 1e-2
    python tools/time_plan_build.py --n 10000000 --m 512 --d 4 --kernel matern52_product --jitter 1e-2
    python tools/time_plan_build.py --n 10000000 --m 512 --d 16 --kernel anova_se:0.3 --jitter 1e-2
    python tools/time_plan_build.py --n 10000000 --m 512 --d 16 --kernel se_categorical:8 --jitter 1e-2

``--d D`` (D > 1) times a D-input build: x is the bench input and D - 1 fixed shuffles of it, z is uniform in the same box, the
lengthscales are 5 (1 + d / D); ``se_categorical:C`` turns the last C columns of x and z into the codes floor(.) mod 8 and gives them
lengthscale 1.  ``--jitter`` is the plan's: K_ZZ of the additive kernel has far fewer than M significant
eigenvalues, so its plans need more than the default 1e-8; the build time does not depend on it.

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
    ap.add_argument("--kernel", default="se", help='se, matern12 (exponential), matern32, matern52, additive_se, additive2_se:W, matern32_product, matern52_product, se_matern32, se_matern52, anova_se:ETA, se_categorical:C or rq:ALPHA')
    ap.add_argument("--d", type=int, default=1, help="input dimensions (1 ... 16)")
    ap.add_argument("--jitter", type=float, default=1e-8)
    a = ap.parse_args()
    name, _, par = a.kernel.partition(":")
    kernel = (name, float(par)) if par else a.kernel  # (rq:ALPHA, additive2_se:W, anova_se:ETA, se_categorical:C)
    if a.two_step and (kernel != "se" or a.d != 1):
        ap.error("--two-step compares the squared-exponential builds at D = 1 only")
    ctx = A.Context(0, seed=1)
    lik = A.BernoulliLikelihood()
    x, y = A.synth_xy(lik, 20240807, 0, a.n, ctx=ctx)
    z = np.linspace(-10, 10, a.m)
    ell = 1.5 * (z[1] - z[0])
    zt = torch.from_numpy(z).cuda()
    if a.d > 1:
        gen = torch.Generator(device="cuda").manual_seed(7)
        x = torch.stack([x] + [x[torch.randperm(a.n, device="cuda", generator=gen)] for _ in range(a.d - 1)], 1).contiguous()
        zt = torch.from_numpy(np.random.default_rng(7).uniform(-10, 10, size=(a.m, a.d))).cuda()
        ell = 5.0 * (1.0 + np.arange(a.d) / a.d)
    if name == "se_categorical":  # the last C columns hold eight category codes each, lengthscale 1 (rho = exp(-1/2))
        ncat = int(float(par))
        x, zt, ell = x.reshape(a.n, a.d).clone(), zt.reshape(a.m, a.d).clone(), np.broadcast_to(ell, (a.d,)).copy()
        x[:, a.d - ncat:] = torch.remainder(torch.floor(x[:, a.d - ncat:]), 8)
        zt[:, a.d - ncat:] = torch.remainder(torch.floor(zt[:, a.d - ncat:]), 8)
        ell[a.d - ncat:] = 1.0
    torch.cuda.synchronize()
    out = {"N": a.n, "M": a.m, "D": a.d, "kernel": a.kernel}
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    times = []
    for _ in range(a.reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        plan = A.Plan.from_inputs(x, zt, ell, jitter=a.jitter, ctx=ctx, kernel=kernel)
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
