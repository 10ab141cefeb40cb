#!/usr/bin/env python3
"""Times agpl_plan_sample_paths (a Paths object evaluated at the plan's own inputs) at the shape of tools/time_chain_predict.py, next
to agpl_plan_predict_chain with samples at the same shape.

    python tools/time_pathwise.py [--N 1000000] [--M 512] [--T 256] [--L 1] [--F 2048] [--reps 10] [--warmup 3] [--profile]

Wall times are medians of `reps` calls between device events after `warmup` calls.  --profile: warm-up plus three calls and nothing
else -- the run to put under `rocprofv3 --kernel-trace --stats` for the kernel times of the set-up, the two feature builds and the
projection.  Prints one JSON line."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import agpl_amd as A  # noqa: E402
from tools.time_chain_predict import timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--N", type=int, default=1_000_000)
    ap.add_argument("--M", type=int, default=512)
    ap.add_argument("--T", type=int, default=256)
    ap.add_argument("--L", type=int, default=1)
    ap.add_argument("--F", type=int, default=2048)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
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
    paths = plan.sample_paths(V=V, nfeatures=a.F, generator=g)
    call = lambda: paths(x)
    if a.profile:
        for _ in range(a.warmup + 3):
            call()
        torch.cuda.synchronize()
        print(json.dumps({"profile_calls": a.warmup + 3}))
        return
    out = {"N": a.N, "M": a.M, "T": a.T, "L": a.L, "F": a.F, "reps": a.reps, "warmup": a.warmup}
    out["sample_paths_ms"] = timed(call, a.reps, a.warmup)
    out["sample_paths_small_ms"] = timed(lambda: paths(x[:128]), a.reps, a.warmup)  # the set-up and the call's wait, almost alone
    out["predict_chain_samples_ms"] = timed(lambda: plan.predict_chain(V, x, samples=True), a.reps, a.warmup)
    out["predict_chain_ms"] = timed(lambda: plan.predict_chain(V, x), a.reps, a.warmup)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
