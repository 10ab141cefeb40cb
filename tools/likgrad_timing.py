#!/usr/bin/env python3
"""Times agpl_expected_loglik (value, gradient and both sums; no per-point output) for Student-t, NegBinomial and Laplace on resident
marginals, with no plan.

    python tools/likgrad_timing.py [--n 10000000] [--reps 10] [--warmup 3] [--lib PATH]

x, y come from synth_xy of the likelihood itself (Laplace, for which it defines no data: its inputs and latent plus Laplace noise);
the marginals are stand-ins for a fit's: mu = 2 sin(x / 2), s = 0.1 + 0.4 u with u = frac(x * 7.3) (so s / (sigma sqrt(nu)) <= 0.5 for the Student-t and the rule takes its 32 nodes a side; the counts' rule is
spaced by min(s / 4, pi / 4)).  `studentt_wide` is the same call at sigma = 1e-3: s / (sigma sqrt(nu)) in [50, 250], the sinh rule
above 64 (s >= 0.128) and the trapezoid rule at up to 2048 nodes a side below it; `studentt_sinh` at nu = 1, sigma = 1e-3 has
s / (sigma sqrt(nu)) in [100, 500] and y = mu + 3 s (2 frac(3.1 x) - 1): the sinh rule alone.  --lib times another build of
libagpl_likgrad.so (it must lie beside libagpl.so).  Device times are medians (with min and max) of `reps` calls between device events after `warmup`
calls; the output buffers are reused, so a timed call allocates nothing.  Prints one JSON line."""
import argparse
import ctypes as C
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import agpl_amd as A  # noqa: E402
from agpl_amd import _ffi  # noqa: E402
from tools.time_chain_predict import timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=10_000_000)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--lib", default=None)
    a = ap.parse_args()
    if a.lib:
        _ffi.LG_LIB_PATH = os.path.abspath(a.lib)
    torch.cuda.set_device(0)
    ctx = A.Context(0, seed=1)
    out = {"n": a.n, "reps": a.reps, "warmup": a.warmup}
    for name, lik in (("studentt", A.StudentTLikelihood(4.0, 0.5)), ("studentt_wide", A.StudentTLikelihood(4.0, 1e-3)),
                      ("studentt_sinh", A.StudentTLikelihood(1.0, 1e-3)),
                      ("negbinomial", A.NegativeBinomialLikelihood(15.0)), ("laplace", A.LaplaceLikelihood(0.5))):
        if name == "laplace":  # the synthetic workload defines no Laplace data: its inputs, its latent and Laplace noise by inversion
            x, _ = A.synth_xy(A.StudentTLikelihood(), 7, 0, a.n, ctx=ctx)
            u = torch.rand(a.n, dtype=torch.float64, device="cuda", generator=torch.Generator(device="cuda").manual_seed(7)) - 0.5
            y = 2.0 * torch.sin(0.7 * x) + torch.cos(0.23 * x) - lik.beta * torch.sign(u) * torch.log1p(-2.0 * u.abs())
        else:
            x, y = A.synth_xy(lik, 7, 0, a.n, ctx=ctx)
        mu = 2.0 * torch.sin(0.5 * x)
        var = (0.1 + 0.4 * torch.frac(x * 7.3).abs()) ** 2
        y = y.to(torch.float64) if lik.ykind == "real" else y
        if name == "studentt_sinh":  # y within mu +- 3 s: every point takes the sinh rule
            y = mu + 3.0 * var.sqrt() * (2.0 * torch.frac(x * 3.1).abs() - 1.0)
        sums = torch.empty(3, dtype=torch.float64, device="cuda")
        d = lik.desc()
        P = len(lik._param_names)
        ptr = lambda t: C.c_void_p(t.data_ptr())

        def call():
            h = ctx.bind()
            _ffi.check(h, _ffi.likgrad_lib().agpl_expected_loglik(h, C.byref(d), C.c_int64(a.n), ptr(mu), ptr(var), ptr(y), C.c_void_p(0),
                                                                  C.c_void_p(0), ptr(sums[:1]), ptr(sums[1:1 + P])))

        med, lo, hi = timed(call, a.reps, a.warmup)
        out[name] = {"ms": [med, lo, hi], "ell_sum": float(sums[0]), "grad_sum": sums[1:1 + P].tolist()}
        del x, y, mu, var
    print(json.dumps(out))


if __name__ == "__main__":
    main()
