#!/usr/bin/env python3
"""Times agpl_sample_y (operators.sample_y on a resident block of function draws) for Bernoulli, NegBinomial (r = 15) and Student-t,
next to the same draws by plain torch on the same F.

    python tools/time_sample_y.py [--T 256] [--Ns 1000000] [--reps 10] [--warmup 3]

Device times are medians (with min and max) of `reps` calls between device events after `warmup` calls.  F is float32 [T, 1, Ns],
standard normal.  `bytes` is what the call must move (4 bytes of F in, 1 / 4 / 8 bytes of y out per draw), `gb_per_s` that over the
median.  The torch lines: Bernoulli `torch.rand_like(F) < torch.sigmoid(F)`; NegBinomial `torch.poisson(Gamma(r, 1).sample() * exp(F))`
(the Gamma-Poisson mixture); Student-t `F + sigma * StudentT(nu).sample()` -- each allocates its temporaries, as a user's line would.
Prints one JSON line."""
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
    ap.add_argument("--T", type=int, default=256)
    ap.add_argument("--Ns", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    torch.cuda.set_device(0)
    ctx = A.Context(0, seed=1)
    g = torch.Generator(device="cuda").manual_seed(7)
    F = torch.randn((a.T, 1, a.Ns), dtype=torch.float32, device="cuda", generator=g)
    n = a.T * a.Ns
    r, nu, sigma = 15.0, 4.0, 0.5
    gamma = torch.distributions.Gamma(torch.tensor(r, device="cuda"), torch.tensor(1.0, device="cuda"))
    student = torch.distributions.StudentT(torch.tensor(nu, device="cuda"))
    cases = [
        ("bernoulli", A.BernoulliLikelihood(), 1, lambda: torch.rand_like(F) < torch.sigmoid(F)),
        ("negbinomial", A.NegativeBinomialLikelihood(r), 4, lambda: torch.poisson(gamma.sample(F.shape) * torch.exp(F))),
        ("studentt", A.StudentTLikelihood(nu, sigma), 8, lambda: F + sigma * student.sample(F.shape)),
    ]
    out = {"T": a.T, "Ns": a.Ns, "reps": a.reps, "warmup": a.warmup}
    for name, lik, ybytes, plain in cases:
        y = A.sample_y(lik, F, sweep=0, ctx=ctx)  # the output block, reused: the timed call allocates nothing
        med, lo, hi = timed(lambda: A.sample_y(lik, F, sweep=1, ctx=ctx, out=y), a.reps, a.warmup)
        tmed, tlo, thi = timed(plain, a.reps, a.warmup)
        nbytes = n * (4 + ybytes)
        out[name] = {"sample_y_ms": [med, lo, hi], "torch_ms": [tmed, tlo, thi], "bytes": nbytes, "gb_per_s": nbytes / med * 1e-6}
        del y
    print(json.dumps(out))


if __name__ == "__main__":
    main()
