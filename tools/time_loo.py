"""Times agpl_plan_loo (include/agpl_loo.h) against agpl_marginals_plan alone on the same plan, on one GPU: device events, medians of 5
after 2 warm-ups.  The difference is the streaming kernel (with its two clears and the one-workgroup sums); it is printed beside the
kernel's bytes / 6.3 TB/s.  Bytes per (point, latent): 16 read (mu, var, gamma, beta; float32) + 24 written (mean, variance, leverage;
float64), + 4 per point for the residual; mu0 is NULL here.

    python tools/time_loo.py [--n 1000000 10000000] [--m 512] [--l 1 4] [--out profiles/loo_mi355x.md]

The plan is built from raw inputs (no float32 feature matrix is held), q(v) by one update from random sites."""
import argparse
import ctypes as C
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HBM = 6.3e12  # bytes / s, the streaming rate the kernels of DESIGN.md 4 are held against


def median_ms(fn, torch, warm=2, reps=5):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        out.append(e0.elapsed_time(e1))
    return statistics.median(out), min(out), max(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, nargs="+", default=[1_000_000, 10_000_000])
    ap.add_argument("--m", type=int, default=512)
    ap.add_argument("--l", type=int, nargs="+", default=[1, 4])
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch

    import agpl_amd as A
    from agpl_amd import _ffi

    ctx = A.Context(0, seed=1)
    lib = _ffi.loo_lib()
    p = lambda t: C.c_void_p(0 if t is None else t.data_ptr())
    rows = []
    for N in a.n:
        for L in a.l:
            gen = torch.Generator(device="cuda").manual_seed(N + L)
            x = torch.rand(N, dtype=torch.float64, device="cuda", generator=gen) * 20 - 10
            z = torch.linspace(-10, 10, a.m, dtype=torch.float64, device="cuda")
            plan = A.Plan.from_inputs(x, z, 20.0 / a.m * 1.5, 1.0, 1e-6, L=L, ctx=ctx)
            gamma = torch.rand((L, N), device="cuda", generator=gen) * 0.25
            beta = torch.randn((L, N), device="cuda", generator=gen)
            # q(v) of these sites: G, g through one float64 pass over chunks of the plan's own features
            G = torch.zeros((L, a.m, a.m), dtype=torch.float64, device="cuda")
            g = torch.zeros((L, a.m), dtype=torch.float64, device="cuda")
            step = 1 << 18
            for i0 in range(0, N, step):
                P = plan.features(i0, min(step, N - i0)).double()
                for l in range(L):
                    G[l] += (P.t() * gamma[l, i0:i0 + P.shape[0]].double()[None]) @ P
                    g[l] += beta[l, i0:i0 + P.shape[0]].double() @ P
                del P
            plan.call("agpl_plan_update", p(G), p(g), C.c_void_p(0), C.c_void_p(0))
            ctx.synchronize()
            nb = lib.agpl_plan_loo_bytes(N, L)
            work = torch.empty(nb, dtype=torch.uint8, device="cuda")
            mu32 = torch.empty((L, N), dtype=torch.float32, device="cuda")
            var32 = torch.empty_like(mu32)
            mu, var, lev = (torch.empty((N, L), dtype=torch.float64, device="cuda") for _ in range(3))
            lev_sum = torch.empty(L, dtype=torch.float64, device="cuda")
            info = torch.empty(2, dtype=torch.int64, device="cuda")
            marg = lambda: plan.call("agpl_marginals_plan", C.c_void_p(0), p(mu32), p(var32))
            loo = lambda: plan.call("agpl_plan_loo", C.c_void_p(0), p(gamma), p(beta), p(work), nb, p(mu), p(var), p(lev), p(lev_sum),
                                    p(info), lib=lib)
            t_m, t_l = median_ms(marg, torch), median_ms(loo, torch)
            bad = info.cpu().tolist()
            nbytes = N * L * (16 + 24) + 4 * N
            ideal = nbytes / HBM * 1e3
            diff = t_l[0] - t_m[0]
            rows.append((N, a.m, L, t_m, t_l, diff, ideal, float(lev_sum[0]), bad[0]))
            print(f"N={N} M={a.m} L={L}: marginals {t_m[0]:.3f} ms [{t_m[1]:.3f}, {t_m[2]:.3f}], loo {t_l[0]:.3f} ms [{t_l[1]:.3f}, {t_l[2]:.3f}], "
                  f"difference {diff:.3f} ms, bytes / 6.3 TB/s {ideal:.3f} ms, ratio {ideal / diff if diff > 0 else float('nan'):.2f}; "
                  f"p_eff[0] {float(lev_sum[0]):.3f}, pairs without a cavity {bad[0]}", flush=True)
            del plan, work, mu, var, lev, gamma, beta, mu32, var32, x
            torch.cuda.empty_cache()
    if a.out:
        with open(a.out, "w") as f:
            f.write("# agpl_plan_loo against agpl_marginals_plan alone (one MI355X)\n\n"
                    "`python tools/time_loo.py`: device events, medians of 5 after 2 warm-ups [min, max]; mu0 NULL; all three outputs, `lev_sum` and `info` asked for.\n"
                    "The difference is the streaming kernel with its two clears and the one-workgroup sums; bytes = N·L·(16 read + 24 written) + 4·N.\n\n"
                    "| N | M | L | marginals ms | loo ms | difference ms | bytes ÷ 6.3 TB/s ms | ratio |\n|---|---|---|---|---|---|---|---|\n")
            for N, M, L, t_m, t_l, diff, ideal, _, _ in rows:
                f.write(f"| {N} | {M} | {L} | {t_m[0]:.3f} [{t_m[1]:.3f}, {t_m[2]:.3f}] | {t_l[0]:.3f} [{t_l[1]:.3f}, {t_l[2]:.3f}] | {diff:.3f} | {ideal:.3f} | "
                        f"{ideal / diff if diff > 0 else float('nan'):.2f} |\n")


if __name__ == "__main__":
    main()
