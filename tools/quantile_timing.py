"""The cost table of DESIGN.md 4.25: predictive_quantile (three probs), predictive_cdf (both tails) and predictive (with log p) on the
same n marginals per kind, timed with device events (the median of three runs after one).  n = 1e6, and 1e5 for the count kinds near
the cap (their rows are scaled to a million points in the table).  Usage: python tools/quantile_timing.py [out.json]"""
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import agpl_amd as A  # noqa: E402

ctx = A.Context(seed=1)
n = 1_000_000
nc = 100_000
rng = np.random.default_rng(0)
mu = torch.as_tensor(rng.normal(size=n)).cuda()
var = torch.as_tensor(rng.uniform(0.01, 1.0, size=n)).cuda()
mu2 = torch.stack([mu, 0.3 * mu], 1).contiguous()
var2 = torch.stack([var, 0.5 * var], 1).contiguous()
y = (mu + torch.as_tensor(rng.normal(size=n)).cuda()).contiguous()
yb = (y > 0).to(torch.uint8)
probs = (0.025, 0.5, 0.975)
ycap = torch.full((nc,), 90000, dtype=torch.int32, device="cuda")
ysm = torch.full((nc,), 3, dtype=torch.int32, device="cuda")
hi = (torch.full((nc,), 3.0, dtype=torch.float64, device="cuda"), var[:nc].contiguous())
lo = (mu[:nc].contiguous(), var[:nc].contiguous())
out = {}
for name, lik, qf, yy in (("poisson_lam3_n1e5", A.PoissonLikelihood(3.0), lo, ysm), ("poisson_lam1e5_n1e5", A.PoissonLikelihood(1e5), hi, ycap),
                          ("negbinomial_r15_n1e5", A.NegativeBinomialLikelihood(15.0), lo, ysm), ("negbinomial_r1e3_n1e5", A.NegativeBinomialLikelihood(1e3), (torch.full((nc,), 4.5, dtype=torch.float64, device="cuda"), var[:nc].contiguous()), ycap),
                          ("bernoulli", A.BernoulliLikelihood(), (mu, var), yb), ("studentt_nu4", A.StudentTLikelihood(4.0, 0.5), (mu, var), y),
                          ("studentt_nu0.5", A.StudentTLikelihood(0.5, 0.5), (mu, var), y), ("laplace", A.LaplaceLikelihood(0.5), (mu, var), y),
                          ("heterogauss", A.HeteroscedasticGaussianLikelihood(2.0), (mu2, var2), y)):
    res = {}
    for what, fn in (("quantile3", lambda: A.predictive_quantile(lik, qf, probs, ctx=ctx)), ("cdf", lambda: A.predictive_cdf(lik, qf, yy, ctx=ctx)),
                     ("predictive", lambda: A.predictive(lik, qf, yy, ctx=ctx))):
        fn()
        torch.cuda.synchronize()
        ts = []
        for _ in range(3):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            ts.append(e0.elapsed_time(e1))
        res[what] = sorted(ts)[1]
    out[name] = res
    print(name, json.dumps(res), flush=True)
if len(sys.argv) > 1:
    json.dump(out, open(sys.argv[1], "w"), indent=1)
