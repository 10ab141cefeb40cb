"""agpl_expected_loglik on the device over its whole supported domain (tests/likgrad_domain.py): every grid point,
ell and every derivative, one launch per parameter set, nothing excluded beyond likgrad_domain.REMOVED.

Device against the reference (tests/likgrad_domain_reference.py): 1e-6 max(1, |ref|) + 4 e^{-8 pi} T_q + 64 eps T_c -- the project's
own line for a defective rule; four times the trapezoid rule's stated design error on the terms that pass through it (T_q: the sum of
|coefficient x expectation| over them); what float64 lgamma and psi can hold of the closed-form terms (T_c: the sum of their
magnitudes).  The classes -- NaN, -inf, finite -- must be the reference's.

Device against the numpy twin of the kernel's rules (tools/likgrad_twin.py), derived and not tuned: both run the same rule in
float64 without contraction, sums of n = 2 nh + 1 (the sinh rule: its node count) products of one sign added in another order, each
with the ulps of exp / log1p behind it, so (2 n + 8) eps times the magnitude sums T_q the twin reports, plus 64 eps T_c for the
device's lgamma, psi, erf and log against scipy's."""
import math
import os
import sys

import numpy as np
import pytest

import likgrad_domain as D
import likgrad_domain_reference as Q

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import likgrad_twin as T  # noqa: E402

pytestmark = pytest.mark.gpu
EPS = np.finfo(np.float64).eps
TERMS = ("1e-6 max(1, |ref|)", "4 e^-8pi T_q", "64 eps T_c")


@pytest.fixture(scope="module")
def A():
    import agpl_amd

    return agpl_amd


@pytest.fixture(scope="module")
def ctx(A):
    return A.Context(seed=1234)


def _lik(A, kind, p):
    return {"bernoulli": lambda: A.BernoulliLikelihood(), "negbinomial": lambda: A.NegativeBinomialLikelihood(p[0]),
            "studentt": lambda: A.StudentTLikelihood(p[0], p[1]), "poisson": lambda: A.PoissonLikelihood(p[0]),
            "laplace": lambda: A.LaplaceLikelihood(p[0]), "heterogauss": lambda: A.HeteroscedasticGaussianLikelihood(p[0])}[kind]()


def _dev(a):
    import torch

    return torch.as_tensor(np.ascontiguousarray(a)).cuda()


def _cls(x):
    return "nan" if math.isnan(x) else ("+inf" if x == math.inf else ("-inf" if x == -math.inf else "finite"))


@pytest.mark.parametrize("kind", D.KINDS)
def test_whole_domain(A, ctx, kind):
    ydt = {"bernoulli": np.uint8, "negbinomial": np.int32, "poisson": np.int32}.get(kind, np.float64)
    P = Q.NPARAMS[kind]
    worst_ref, worst_twin = (0.0, "", 0, 0), (0.0, "", 0)
    bad, n = [], 0
    for p, pts in D.groups(kind):
        y = np.array([pt[2] for pt in pts], dtype=ydt)
        mu = np.array([pt[3] for pt in pts], dtype=np.float64)
        var = np.array([pt[4] for pt in pts], dtype=np.float64)
        _, _, ell, dell = A.expected_loglik(_lik(A, kind, p), _dev(mu), _dev(var), _dev(y), ctx=ctx, per_point=True)
        ell = ell.cpu().numpy()
        dell = dell.cpu().numpy().reshape(len(pts), P) if P else np.empty((len(pts), 0))
        for i, (name, _, yi, mi, vi) in enumerate(pts):
            n += 1
            ref = Q.reference(kind, p, yi, mi, vi)
            ell_t, dell_t, tq_t = T.twin(kind, p, yi, mi, vi)
            nodes = T.EVALS
            got = [float(ell[i])] + [float(v) for v in dell[i]]
            for k, (g, r, t, bar) in enumerate(zip(got, ref.values, [ell_t] + list(dell_t), Q.bars(ref))):
                assert ref.err[k] <= 1e-9 * max(1.0, abs(r)), (name, k, ref.err[k])  # (the CPU module proves this for every kept point)
                if _cls(g) != _cls(r) or _cls(g) != _cls(t):
                    bad.append((name, k, "class", g, r, t))
                    continue
                if not math.isfinite(r):
                    continue
                f = abs(g - r) / bar
                terms = Q.bar_terms(ref, k)
                if f > worst_ref[0]:
                    worst_ref = (f, name, k, int(np.argmax(terms)))
                tbar = (2 * nodes + 8) * EPS * tq_t[k] + 64 * EPS * ref.tc[k]
                ft = abs(g - t) / tbar if tbar > 0.0 else (0.0 if g == t else math.inf)
                if ft > worst_twin[0]:
                    worst_twin = (ft, name, k)
                if not f <= 1.0:
                    bad.append((name, k, "reference", f, g, r))
                if not ft <= 1.0:
                    bad.append((name, k, "twin", ft, g, t))
    print(f"LIKGRAD DOMAIN {kind}: {n} points; against the reference the worst is {worst_ref[0]:.3e} of the bar at {worst_ref[1]} (output {worst_ref[2]}; "
          f"the bar's largest term there: {TERMS[worst_ref[3]]}); against the twin {worst_twin[0]:.3e} of its bar at {worst_twin[1]} (output {worst_twin[2]})")
    assert n == len(D.points(kind)) >= 40
    assert not bad, bad


def test_non_finite_y_of_the_real_valued_kinds(A, ctx):
    """ell = -inf and NaN derivatives for y = +-inf, NaN throughout for y = NaN, at that point only -- the convention of a count y < 0
    -- and on either rule of the Student-t kind (s / a = 0.4 and 1e3)."""
    for kind, p, mu, var in (("studentt", (3.0, 0.5), 0.2, 0.3), ("studentt", (1.0, 1e-3), 0.2, 1.0), ("laplace", (0.5,), 0.2, 0.3),
                             ("heterogauss", (2.0,), (0.2, -1.0), (0.3, 0.5))):
        ys = np.array([0.7, np.inf, -np.inf, np.nan, -0.4])
        m, v = np.array([mu] * len(ys), dtype=np.float64), np.array([var] * len(ys), dtype=np.float64)
        _, _, ell, dell = A.expected_loglik(_lik(A, kind, p), _dev(m), _dev(v), _dev(ys), ctx=ctx, per_point=True)
        ell, dell = ell.cpu().numpy(), dell.cpu().numpy().reshape(len(ys), -1)
        assert ell[1] == -np.inf and ell[2] == -np.inf and np.isnan(ell[3]) and np.isnan(dell[1:4]).all(), (kind, ell, dell)
        assert np.isfinite(ell[[0, 4]]).all() and np.isfinite(dell[[0, 4]]).all(), kind
        for i in (0, 4):
            ref = Q.reference(kind, p, float(ys[i]), mu, var)
            assert abs(ell[i] - ref.values[0]) <= Q.bars(ref)[0], (kind, i)
