"""tests/sample_y_reference.py held against what it claims, without a GPU, on the exact inputs of the equality cases of
tests/test_gpu_sample_y.py (T = 3 draws of 257 points, f in [-4, 4]):

* its draws have the moments of p(y | f): sum (y - E[y|f]) and sum ((y - E)^2 - Var) lie within 5 standard errors, the errors from
  the closed forms (Var and the fourth central moment of y | f; direct sums over the probabilities for the counts), never from the
  draws.  Student-t with nu = 1.5 has neither mean nor variance: there the sign of y - f and the event |y - f| <= sigma are
  counted instead (probabilities 1/2 and the integral of the density).  The categorical kinds: every class's frequency.
* no draw has a comparison margin below 1e-9 (expected number at double precision: about 1e-4), so the GPU test needs no
  exemption; and no real draw is a cancellation (|y| >= 1e-3 (|f| + |y - f|)), so the few-ulp differences of a device libm in
  the noise term stay below the GPU test's 1e-12 relative;
* five wrong samplers each differ from the reference on at least 1 % of the draws."""
import math

import numpy as np
import pytest

import sample_y_reference as R


@pytest.mark.parametrize("c", R.CASES, ids=lambda c: c.id)
def test_reference_has_the_moments_of_the_likelihood(oracle, c):
    F, y, _ = R.case_reference(oracle, c)
    f = F[:, :, : R.NS].astype(np.float64)
    n = R.T * R.NS
    stats = []  # (name, statistic, its standard deviation)
    if c.kind in (R.CATEGORICAL, R.CATEGORICAL_BIJ):
        L = f.shape[1]
        theta = np.exp(np.asarray(c.logtheta))
        w = theta[:L, None, None] * (1.0 / (1.0 + np.exp(-f.transpose(1, 0, 2))))  # [L, T, NS]
        const = 0.5 * theta[L] if c.kind == R.CATEGORICAL_BIJ else 0.0
        pr = w / (w.sum(0) + const)
        assert set(np.unique(y)) <= {0, 1} and (y.sum(-1) <= 1).all()
        if c.kind == R.CATEGORICAL:
            assert (y.sum(-1) == 1).all()
        for k in range(L):
            stats.append((f"class {k}", (y[:, :, k] - pr[k]).sum(), math.sqrt((pr[k] * (1 - pr[k])).sum())))
        if const:
            p_last = 1.0 - pr.sum(0)
            stats.append((f"class {L}", ((y.sum(-1) == 0) - p_last).sum(), math.sqrt((p_last * (1 - p_last)).sum())))
    elif c.kind == R.STUDENTT and c.p[0] <= 4.0:
        r = y - f[:, 0]
        pm = R.studentt_central_mass(c.p[0])
        stats.append(("sign", np.sign(r).sum(), math.sqrt(n)))
        stats.append(("central mass", ((np.abs(r) <= c.p[1]) - pm).sum(), math.sqrt(n * pm * (1 - pm))))
    else:
        m, v, m4 = np.empty((R.T, R.NS)), np.empty((R.T, R.NS)), np.empty((R.T, R.NS))
        for t in range(R.T):
            for i in range(R.NS):
                x = f[t, 0, i]
                if c.kind == R.BERNOULLI:
                    s = R.sigma(x)
                    mv = s, s * (1 - s), s * (1 - s) * (1 - 3 * s * (1 - s))
                elif c.kind in (R.POISSON, R.NEGBINOMIAL):
                    mv = R.count_moments(c, x)
                elif c.kind == R.STUDENTT:
                    nu, sg = c.p
                    mv = x, sg * sg * nu / (nu - 2), 3 * sg ** 4 * nu * nu / ((nu - 2) * (nu - 4))
                elif c.kind == R.LAPLACE:
                    mv = x, 2 * c.p[0] ** 2, 24 * c.p[0] ** 4
                else:
                    vv = 1.0 / (c.p[0] * R.sigma(f[t, 1, i]))
                    mv = x, vv, 3 * vv * vv
                m[t, i], v[t, i], m4[t, i] = mv
        r = y.astype(np.float64) - m
        stats.append(("mean", r.sum(), math.sqrt(v.sum())))
        stats.append(("variance", (r * r - v).sum(), math.sqrt((m4 - v * v).sum())))
    for name, s, sd in stats:
        print(f"{c.id}: {name}: statistic / standard error = {s / sd:+.2f}")
        assert abs(s) <= 5 * sd, (name, s, sd)


def test_no_draw_of_the_gpu_cases_is_near_a_decision_or_a_cancellation(oracle):
    for c in R.CASES:
        F, y, margin = R.case_reference(oracle, c)
        print(f"{c.id}: smallest margin {margin.min():.2e}, margins below 1e-9: {(margin < 1e-9).sum()}")
        assert (margin < 1e-9).sum() == 0, c.id
        if y.dtype == np.float64:
            f = F[:, 0, : R.NS].astype(np.float64)
            cond = np.abs(y) / (np.abs(f) + np.abs(y - f))
            print(f"{c.id}: smallest |y| / (|f| + |y - f|) {cond.min():.2e}")
            assert (cond >= 1e-3).all(), c.id


@pytest.mark.parametrize("variant,case_id", [("neg_f", "bernoulli"), ("no_draw", "bernoulli"), ("no_point", "bernoulli"),
                                             ("swap_normal", "studentt-nu10"), ("nb_sigma", "negbinomial-r15")])
def test_a_wrong_sampler_differs_on_at_least_one_percent_of_draws(oracle, variant, case_id):
    c = next(c for c in R.CASES if c.id == case_id)
    F, y, _ = R.case_reference(oracle, c)
    wrong, _ = R.sample(oracle, c, F, R.SEED, R.POINT0, R.DRAW0, R.SWEEP, ns=R.NS, variant=variant)
    if y.dtype == np.float64:
        differ = np.abs(wrong - y) > 1e-12 * np.abs(y)  # the GPU test's bar
    else:
        differ = wrong != y
    print(f"{variant} on {case_id}: {differ.mean():.1%} of draws differ")
    assert differ.mean() >= 0.01


def test_stream_index_is_the_sub_stream_of_the_point():
    """Counter word 3 = (p >> 32) & 0xFF plus (1 + d) << 8, word 2 = the low word of the point."""
    s = R.stream_index(2 ** 32 + 5, 65534)
    assert s & 0xFFFFFFFF == 5 and (s >> 32) == 1 + (65535 << 8)
    assert R.stream_index(7, 0) >> 32 == 1 << 8
    assert R.stream_index(2 ** 40 + 3 * 2 ** 32, 2 ** 24 - 3) >> 32 == 3 + ((2 ** 24 - 2) << 8) < 2 ** 32
