#!/usr/bin/env python3
"""Times agpl_plan_predict_cov (Plan.predict_cov) and the only route the library offered before it: a second plan at the test inputs ->
plan.features() (float32 Phi), S - I = U'U - I from the plan's state, two float32 torch.matmul and the kernel in torch.

    python tools/time_predict_cov.py [--M 512] [--L 1] [--reps 10] [--warmup 3] [--limit 120] [--profile sym|rect]

Two shapes: a symmetric 16384 x 16384 block and a 65536 x 4096 rectangle (D = 1, squared-exponential kernel, q(v) from one update on
random natural parameters).  Wall times are medians of `reps` calls between device events after `warmup` calls; device memory is
what hipMemGetInfo reports in use beyond the state before the step (it sees the library's own scratch, which torch's counters do
not), torch's peak counter for the torch route.  One process; every step runs under an alarm of `--limit` seconds whose default
action ends the process, so nothing is started on the device after a step that hangs.
--profile sym|rect: warm-up plus three calls of that shape and nothing else -- the run to put under
`rocprofv3 --kernel-trace --stats` for the per-kernel times (joint_w_kernel, se_build_kernel, joint_t_kernel, joint_cov_kernel).
Prints one JSON line."""
import argparse
import ctypes as C
import json
import os
import signal
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import agpl_amd as A  # noqa: E402

SHAPES = {"sym": (16384, 16384, True), "rect": (65536, 4096, False)}


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


def in_use():
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    free, total = torch.cuda.mem_get_info()
    return total - free


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--M", type=int, default=512)
    ap.add_argument("--L", type=int, default=1)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--limit", type=int, default=120, help="seconds per step")
    ap.add_argument("--profile", choices=sorted(SHAPES))
    a = ap.parse_args()
    torch.cuda.set_device(0)
    ctx = A.Context(0, seed=1)
    g = torch.Generator(device="cuda").manual_seed(7)
    M, L = a.M, a.L
    z = torch.linspace(-10, 10, M, dtype=torch.float64, device="cuda")
    ell = 1.5 * 20 / (M - 1)
    with step(a.limit):
        xt = -10 + 20 * torch.rand(4096, dtype=torch.float64, device="cuda", generator=g)
        plan = A.Plan.from_inputs(xt, z, ell, L=L, ctx=ctx)
        B = torch.randn(L, M, M // 2, dtype=torch.float64, device="cuda", generator=g)
        G, gg = B @ B.transpose(1, 2), torch.randn(L, M, dtype=torch.float64, device="cuda", generator=g)
        plan.call("agpl_plan_update", C.c_void_p(G.data_ptr()), C.c_void_p(gg.data_ptr()), C.c_void_p(0), C.c_void_p(0))
        ctx.synchronize()
    inputs = {k: (-10 + 20 * torch.rand(na, dtype=torch.float64, device="cuda", generator=g),
                  None if sym else -10 + 20 * torch.rand(nb, dtype=torch.float64, device="cuda", generator=g))
              for k, (na, nb, sym) in SHAPES.items()}
    if a.profile:
        with step(a.limit):
            xa, xb = inputs[a.profile]
            for _ in range(a.warmup + 3):
                plan.predict_cov(xa, xb)
            torch.cuda.synchronize()
        print(json.dumps({"profile": a.profile, "profile_calls": a.warmup + 3}))
        return
    out = {"M": M, "Mp": plan.Mp, "L": L, "reps": a.reps, "warmup": a.warmup}
    for name, (na, nb, sym) in SHAPES.items():
        xa, xb = inputs[name]
        r = {"Na": na, "Nb": nb, "symmetric": sym}
        with step(a.limit):
            base = in_use()
            cov = plan.predict_cov(xa, xb)
            r["predict_cov_device_bytes"] = in_use() - base  # the output and the library's scratch
            r["predict_cov_output_bytes"] = cov.numel() * 4
            r["predict_cov_ms"] = timed(lambda: plan.predict_cov(xa, xb), a.reps, a.warmup)
        # executed float16 MFMA work of the product kernel: three products per tile pair that is computed, Mp features
        ta, tb = (na + 127) // 128, (nb + 127) // 128
        tiles = ta * (ta + 1) // 2 if sym else ta * tb
        r["product_mfma_flop"] = 3 * 2 * tiles * 128 * 128 * plan.Mp * L
        r["t_mfma_flop"] = 3 * 2 * tb * 128 * plan.Mp * plan.Mp * L

        # the route of the parent commit
        def torch_route():
            pa = A.Plan.from_inputs(xa, z, ell, ctx=ctx)
            Fa = pa.features()
            Fb = Fa if sym else A.Plan.from_inputs(xb, z, ell, ctx=ctx).features()
            res = []
            for l in range(L):
                U = torch.tril(plan.U_colmajor[l].t()[:M, :M])
                W = (U.t() @ U - torch.eye(M, dtype=torch.float64, device="cuda")).to(torch.float32)
                b = xa if sym else xb
                k = torch.exp(-0.5 * ((xa[:, None] - b[None, :]) / ell) ** 2).to(torch.float32)
                res.append(k.addmm_(Fa @ W, Fb.t()))
            return res

        with step(a.limit):
            torch.cuda.synchronize()
            torch.cuda.empty_cache()
            torch.cuda.reset_peak_memory_stats()
            m0 = torch.cuda.memory_allocated()
            ref = torch_route()
            torch.cuda.synchronize()
            r["torch_route_peak_bytes"] = torch.cuda.max_memory_allocated() - m0
            r["max_abs_diff_vs_torch_route"] = float((cov[0] - ref[0]).abs().max())
            del ref
            r["torch_route_ms"] = timed(torch_route, a.reps, a.warmup)
        del cov
        out[name] = r
    print(json.dumps(out))


if __name__ == "__main__":
    main()
