#!/usr/bin/env python3
"""Times agpl_plan_predict_grad (Plan.predict_grad) next to agpl_plan_predict at the same new inputs: the gradient repeats the
generation, the whitening and the marginal pass once per input dimension, so the expectation is about D x one predict.

    python tools/time_predict_grad.py [--Ns 1000000] [--M 512] [--D 3] [--L 1] [--kernel se] [--reps 10] [--warmup 3]

Wall times are (median, min, max) of `reps` calls between device events after `warmup` calls.  Prints one JSON line."""
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
    ap.add_argument("--Ns", type=int, default=1_000_000)
    ap.add_argument("--N", type=int, default=4096)  # the plan's own points: they only carry the plan
    ap.add_argument("--M", type=int, default=512)
    ap.add_argument("--D", type=int, default=3)
    ap.add_argument("--L", type=int, default=1)
    ap.add_argument("--kernel", default="se")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    torch.cuda.set_device(0)
    ctx = A.Context(0, seed=1)
    g = torch.Generator(device="cuda").manual_seed(7)
    uni = lambda n: -10 + 20 * torch.rand(n, a.D, dtype=torch.float64, device="cuda", generator=g)
    x, z, xs = uni(a.N), uni(a.M), uni(a.Ns)
    kernel = ("rq", 2.0) if a.kernel == "rq" else a.kernel
    plan = A.Plan.from_inputs(x, z, 4.0, L=a.L, ctx=ctx, kernel=kernel, jitter=1e-6)
    out = {"Ns": a.Ns, "M": a.M, "D": a.D, "L": a.L, "kernel": a.kernel, "reps": a.reps, "warmup": a.warmup}
    out["predict_ms"] = timed(lambda: plan.predict(xs), a.reps, a.warmup)
    out["predict_grad_ms"] = timed(lambda: plan.predict_grad(xs), a.reps, a.warmup)
    out["D_x_predict_ms"] = a.D * out["predict_ms"][0]
    out["ratio_to_D_x_predict"] = out["predict_grad_ms"][0] / out["D_x_predict_ms"]
    print(json.dumps(out))


if __name__ == "__main__":
    main()
