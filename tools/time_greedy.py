#!/usr/bin/env python3
"""Times agpl_select_inducing_greedy (agpl_amd.select_inducing_greedy: begin, then M x (pick + pivot record, step), one wait) and its
hot path, agpl_greedy_step, against the streaming rate the step is bound by; agpl_select_inducing_kmeans (niter = 10) on the same
inputs for context.

    python tools/time_greedy.py [--N 1000000 10000000] [--M 512] [--D 1 4 16] [--reps 5] [--warmup 2] [--limit 300]

Medians of `reps` calls between device events after `warmup` calls.  `step_ms[j]` = one agpl_greedy_step (the pass over the points and
the one-workgroup reduction of its partials) on a state of j columns; `stream_fraction[j]` = 8 n j bytes / `--stream-tbs` (default
6.3 TB/s, the MI355X's measured streaming rate) over that time.  `fixed_ms` = the step at j = 0: the read of x, kappa, the update of d,
the partials and the launches, with no column to stream; `fixed_share` = M fixed_ms over the whole call.  `steps_ms` = the steps of
the whole call summed by linear interpolation between the measured j; `rest_ms` = the whole call minus that: the pick kernels' pivot
gathers, the begin pass, the clears, the host's enqueueing where it is not hidden.  Nothing finer is separated.  One process; every
stage runs under an alarm whose default action ends the process, so nothing is started on the device after a stage that hangs.
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
from agpl_amd import _ffi  # noqa: E402


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
    ap.add_argument("--N", type=int, nargs="+", default=[1_000_000, 10_000_000])
    ap.add_argument("--M", type=int, default=512)
    ap.add_argument("--D", type=int, nargs="+", default=[1, 4, 16])
    ap.add_argument("--J", type=int, nargs="+", default=[64, 256, 511])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--kernel", default="matern32")
    ap.add_argument("--limit", type=int, default=300, help="seconds per stage")
    ap.add_argument("--stream-tbs", type=float, default=6.3)
    ap.add_argument("--no-kmeans", action="store_true")
    a = ap.parse_args()
    torch.cuda.set_device(0)
    ctx = A.Context(0, seed=1)
    lib = _ffi.greedy_lib()
    g = torch.Generator(device="cuda").manual_seed(11)
    kind, param = A.sparse.kernel_kind(a.kernel)
    M = a.M
    out = {"M": M, "kernel": a.kernel, "reps": a.reps, "warmup": a.warmup, "stream_tbs": a.stream_tbs, "cases": []}
    for N in a.N:
        for D in a.D:
            signal.alarm(a.limit)
            shifts = 12.0 * torch.rand(4, D, dtype=torch.float64, device="cuda", generator=g) - 6.0
            k = torch.randint(0, 4, (N,), device="cuda", generator=g)
            x = shifts[k] + torch.randn(N, D, dtype=torch.float64, device="cuda", generator=g)
            del k
            r = {"N": N, "D": D}
            # threshold at its floor: all M steps run
            sel = lambda: A.select_inducing_greedy(x, M, kernel=a.kernel, threshold=1e-12, ctx=ctx, return_info=True)
            z, info = sel()
            r["selected"], r["max_residual_last"], r["trace_last_over_N"] = info["selected"], float(info["max_residual"][-1]), float(info["trace"][-1]) / N
            r["whole_ms"] = timed(sel, a.reps, a.warmup)
            # the step alone, on a state of j columns (any finite numbers stream as fast as a run's own)
            signal.alarm(a.limit)
            nb = C.c_int64()
            assert lib.agpl_greedy_bytes(N, M, C.byref(nb)) == 0
            work = torch.empty(nb.value // 8, dtype=torch.int64, device="cuda")
            f = work.view(torch.float64)
            f[:M * N].normal_(0.0, 0.03, generator=g)
            ell = np.ones(D)
            index = torch.tensor([N // 2], dtype=torch.int64, device="cuda")
            pivot = torch.cat([x[N // 2], torch.ones(1, dtype=torch.float64, device="cuda"), f[N // 2:M * N:N][:M - 1].clone()])
            cand = torch.zeros(2, dtype=torch.int64, device="cuda")
            trace = torch.zeros(M, dtype=torch.int64, device="cuda")
            h = ctx.bind()

            def step(j):
                f[M * N:(M + 1) * N].fill_(1.0)
                _ffi.check(h, lib.agpl_greedy_step(h, N, 0, N, M, D, kind, param, j, x.data_ptr(), ell.ctypes.data_as(C.c_void_p), 1.0,
                                                   index.data_ptr(), pivot.data_ptr(), work.data_ptr(), nb.value, cand.data_ptr(),
                                                   trace.data_ptr()))

            fill_ms = timed(lambda: f[M * N:(M + 1) * N].fill_(1.0), a.reps, a.warmup)[0]
            js = [0] + [j for j in a.J if 0 < j < M]
            r["step_ms"], r["stream_fraction"] = {}, {}
            for j in js:
                ms = timed(lambda: step(j), a.reps, a.warmup)[0] - fill_ms
                r["step_ms"][j] = ms
                if j:
                    r["stream_fraction"][j] = 8.0 * N * j / (a.stream_tbs * 1e12) / (ms * 1e-3)
            r["fixed_ms"] = r["step_ms"][0]
            r["fixed_share"] = M * r["fixed_ms"] / r["whole_ms"][0]
            r["steps_ms"] = float(np.interp(np.arange(M), js, [r["step_ms"][j] for j in js]).sum())
            r["rest_ms"] = r["whole_ms"][0] - r["steps_ms"]
            del work, f
            torch.cuda.empty_cache()
            if not a.no_kmeans:
                signal.alarm(a.limit)
                r["kmeans_niter10_ms"] = timed(lambda: A.select_inducing(x, M, niter=10, ctx=ctx), a.reps, a.warmup)
            signal.alarm(0)
            out["cases"].append(r)
            del x
            torch.cuda.empty_cache()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
