#!/usr/bin/env python3
"""Times agpl_plan_predict_chain (Plan.predict_chain) at the plan's own inputs, and the one thing the library offered before it at
those points: plan.features() followed by a float32 torch.matmul of the same shape.

    python tools/time_chain_predict.py [--N 1000000] [--M 512] [--T 256] [--L 1] [--reps 10] [--warmup 3] [--samples] [--profile]

Wall times are medians of `reps` calls between device events after `warmup` calls.  --profile: warm-up plus three calls and nothing
else -- the run to put under `rocprofv3 --kernel-trace --stats` for the kernel times of the pack, build and projection launches.
Prints one JSON line."""
import argparse
import json
import os
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--N", type=int, default=1_000_000)
    ap.add_argument("--M", type=int, default=512)
    ap.add_argument("--T", type=int, default=256)
    ap.add_argument("--L", type=int, default=1)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--samples", action="store_true", help="also write F [T, L, N]")
    ap.add_argument("--profile", action="store_true")
    a = ap.parse_args()
    torch.cuda.set_device(0)
    ctx = A.Context(0, seed=1)
    g = torch.Generator(device="cuda").manual_seed(7)
    x = -10 + 20 * torch.rand(a.N, dtype=torch.float64, device="cuda", generator=g)
    z = torch.linspace(-10, 10, a.M, dtype=torch.float64, device="cuda")
    ell = 1.5 * 20 / (a.M - 1)
    plan = A.Plan.from_inputs(x, z, ell, L=a.L, ctx=ctx, flags=A.Plan.NO_MARGINALS)
    V = torch.randn(a.T, a.L, a.M, dtype=torch.float64, device="cuda", generator=g)
    call = lambda: plan.predict_chain(V, x, samples=a.samples)
    if a.profile:
        for _ in range(a.warmup + 3):
            call()
        torch.cuda.synchronize()
        print(json.dumps({"profile_calls": a.warmup + 3}))
        return
    out = {"N": a.N, "M": a.M, "T": a.T, "L": a.L, "samples": a.samples, "reps": a.reps, "warmup": a.warmup}
    out["predict_chain_ms"] = timed(call, a.reps, a.warmup)
    # executed float16 MFMA work of the projection: three products per sub-product, Mp features, whole 32-row groups of draws
    Mp, TL = plan.Mp, a.T * a.L
    rows = 32 * ((min(a.L, 128) + 31) // 32) + 128 * (TL // 128) + 32 * ((TL % 128 + 31) // 32)
    out["projection_mfma_flop"] = 3 * 2 * ((a.N + 127) // 128 * 128) * rows * Mp
    # what the parent offers at these points: the decoded features and a float32 matmul (one latent's draws)
    V32 = V[:, 0].to(torch.float32).t().contiguous()
    feats = {}

    def decode():
        feats["F"] = plan.features()

    out["features_ms"] = timed(decode, a.reps, a.warmup)
    out["matmul_f32_ms"] = timed(lambda: torch.matmul(feats["F"], V32), a.reps, a.warmup)
    F = torch.matmul(feats["F"], V32)
    mean, var, resid, Fs = plan.predict_chain(V, x[:4096], samples=True)
    out["max_abs_diff_vs_matmul"] = float((Fs[:, 0].t() - F[:4096]).abs().max())
    print(json.dumps(out))


if __name__ == "__main__":
    main()
