#!/usr/bin/env python3
"""Times agpl_select_inducing_kmeans (agpl_amd.select_inducing, niter = 1: the max pass, the start, two steps and one update) and
the only route a user could write before it: one Lloyd iteration in torch float64 -- chunked cdist + argmin + index_add_, then the
assignment pass for the final cost -- on the same device in the same process.

    python tools/time_inducing.py [--N 10000000] [--M 512] [--D 1 4 16] [--reps 10] [--warmup 3] [--limit 300]

Medians of `reps` calls between device events after `warmup` calls.  `step_ms` = the niter = 1 call minus the niter = 0 call (the max pass, the start and
one step): the cost of ONE step and one update; `fma_fraction` = N M D float64 fused multiply-adds per step over
`--peak-tfma` (the vector-float64 rate in 10^12 FMA/s; default 39.3 = 78.6 TFLOP/s, the MI355X's).  One process; every stage runs
under an alarm whose default action ends the process, so nothing is started on the device after a stage that hangs.  Prints one JSON
line."""
import argparse
import json
import os
import signal
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import agpl_amd as A  # noqa: E402


def timed(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return float(np.median(ms)), float(min(ms)), float(max(ms))


def torch_lloyd(x, z, ell, chunk):
    """One Lloyd iteration and the final cost, float64, N x M distances never held beyond `chunk` points."""
    u, M, D = x / ell, z.shape[0], x.shape[1]
    for last in (False, True):
        zs = z / ell
        s = torch.zeros((M, D), dtype=torch.float64, device=x.device)
        cnt = torch.zeros(M, dtype=torch.float64, device=x.device)
        cost = torch.zeros((), dtype=torch.float64, device=x.device)
        for i in range(0, x.shape[0], chunk):
            d = torch.cdist(u[i:i + chunk], zs)
            dmin, a = d.min(dim=1)
            cost += (dmin * dmin).sum()
            if not last:
                s.index_add_(0, a, u[i:i + chunk])
                cnt.index_add_(0, a, torch.ones_like(dmin))
        if not last:
            z = torch.where(cnt[:, None] > 0, ell * s / cnt.clamp(min=1)[:, None], z)
    return z, cost


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--N", type=int, default=10_000_000)
    ap.add_argument("--M", type=int, default=512)
    ap.add_argument("--D", type=int, nargs="+", default=[1, 4, 16])
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--chunk", type=int, default=1 << 18)
    ap.add_argument("--limit", type=int, default=300, help="seconds per stage")
    ap.add_argument("--peak-tfma", type=float, default=39.3)
    a = ap.parse_args()
    torch.cuda.set_device(0)
    ctx = A.Context(0, seed=1)
    g = torch.Generator(device="cuda").manual_seed(11)
    out = {"N": a.N, "M": a.M, "reps": a.reps, "warmup": a.warmup, "peak_tfma": a.peak_tfma, "cases": []}
    for D in a.D:
        signal.alarm(a.limit)
        shifts = 12.0 * torch.rand(4, D, dtype=torch.float64, device="cuda", generator=g) - 6.0
        k = torch.randint(0, 4, (a.N,), device="cuda", generator=g)
        x = shifts[k] + torch.randn(a.N, D, dtype=torch.float64, device="cuda", generator=g)
        ell = torch.ones(D, dtype=torch.float64, device="cuda")
        r = {"D": D}
        z1, info = A.select_inducing(x, a.M, niter=1, ctx=ctx, return_info=True)
        z0 = A.select_inducing(x, a.M, niter=0, ctx=ctx)
        r["select_niter1_ms"] = timed(lambda: A.select_inducing(x, a.M, niter=1, ctx=ctx), a.reps, a.warmup)
        r["select_niter0_ms"] = timed(lambda: A.select_inducing(x, a.M, niter=0, ctx=ctx), a.reps, a.warmup)
        r["step_ms"] = r["select_niter1_ms"][0] - r["select_niter0_ms"][0]
        r["fma_fraction"] = a.N * a.M * D / (r["step_ms"] * 1e-3) / (a.peak_tfma * 1e12)
        signal.alarm(a.limit)
        zt, cost = torch_lloyd(x, z0, ell, a.chunk)
        r["max_abs_z_diff_vs_torch"] = float((zt - z1).abs().max())
        r["rel_cost_diff_vs_torch"] = float(abs(cost.item() - info["cost"]) / info["cost"])
        r["torch_lloyd_ms"] = timed(lambda: torch_lloyd(x, z0, ell, a.chunk), a.reps, a.warmup)
        signal.alarm(0)
        out["cases"].append(r)
        del x, k
        torch.cuda.empty_cache()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
