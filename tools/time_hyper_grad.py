#!/usr/bin/env python3
"""Times agpl_plan_hyper_grad (Plan.hyper_grad) next to the two things a hyperparameter loop already pays for: one CAVI sweep and
one Plan.from_inputs build.

    python tools/time_hyper_grad.py [--N 10000000] [--M 512] [--D 1] [--reps 5] [--warmup 2] [--limit 300]

Bernoulli data from synth_xy, squared-exponential kernel, z on a grid, q(v) after two sweeps.  Wall times are medians of `reps`
calls between device events after `warmup` calls.  From the code the gradient costs about one plan build (the features are
regenerated) plus one N Mp^2 split-float16 product per latent (the accumulation's order of cost).  One process; every step runs
under an alarm of `--limit` seconds whose default action ends the process, so nothing is started on the device after a step that
hangs.  Prints one JSON line."""
import argparse
import json
import os
import signal
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import agpl_amd as A  # noqa: E402


class step:
    """A step under a time limit: SIGALRM's default action ends the process."""

    def __init__(self, seconds):
        self.seconds = seconds

    def __enter__(self):
        signal.alarm(self.seconds)

    def __exit__(self, *exc):
        signal.alarm(0)
        return False


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--N", type=int, default=10_000_000)
    ap.add_argument("--M", type=int, default=512)
    ap.add_argument("--D", type=int, default=1)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--limit", type=int, default=300, help="seconds per step")
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
        lo, hi = float(x[:, 0].min()), float(x[:, 0].max())
        if D == 1:
            z, ell = torch.linspace(lo, hi, M, dtype=torch.float64, device="cuda"), 1.5 * (hi - lo) / (M - 1)
        else:
            z, ell = x[torch.randperm(N, device="cuda")[:M]].clone(), 3.0
        cavi = A.SparseCAVI.from_inputs(lik, x, y, z, ell, jitter=1e-6, ctx=ctx, keep_points=True, keep_inputs=True)
        cavi.run(2)
        cavi.accumulate()
        cavi.check()
    out = {"N": N, "M": M, "Mp": cavi.plan.Mp, "D": D, "reps": a.reps, "warmup": a.warmup}
    with step(a.limit):
        out["hyper_grad_ms"] = timed(lambda: cavi.plan.hyper_grad(x, cavi.beta, cavi.gamma, None, cavi.G, cavi.g), a.reps, a.warmup)
        out["hyper_grad_points_only_ms"] = timed(lambda: cavi.plan.hyper_grad(x, cavi.beta, cavi.gamma), a.reps, a.warmup)
    with step(a.limit):
        def sweep():
            cavi.sweep()
            cavi.check()
        out["cavi_sweep_ms"] = timed(sweep, a.reps, a.warmup)
    with step(a.limit):
        mem = torch.empty(cavi.plan.nbytes, dtype=torch.uint8, device="cuda")
        out["from_inputs_build_ms"] = timed(lambda: A.Plan.from_inputs(x, z, ell, jitter=1e-6, ctx=ctx, storage=mem).close(), a.reps,
                                            a.warmup)
    out["split_f16_mfma_flop"] = 3 * 2 * ((N + 127) // 128) * 128 * cavi.plan.Mp * ((M + 127) // 128) * 128
    print(json.dumps(out))


if __name__ == "__main__":
    main()
