"""The numpy yardstick of the greedy conditional-variance selection (tests/greedy_reference.py) held against linear algebra it does not
use: its columns are the Cholesky factor of K at the picks, its residuals the Nystrom residuals of a direct solve, every pick the
brute-force argmax of that diagonal; and the properties of the named cases that tests/test_gpu_greedy.py relies on -- which cases have
residual gaps wide enough for the exact-index test, and how far every maximum stays from the threshold.  No GPU."""
import numpy as np
import pytest

import greedy_reference as G

IDS = [c.id for c in G.CASES]


@pytest.mark.parametrize("c", G.CASES, ids=IDS)
def test_columns_are_the_cholesky_factor_at_the_picks(c):
    r = G.run_case(c)
    x, picks = G.data(c), r["indices"]
    K = G.gram(x[picks], x[picks], G.ell_of(c), c.kernel, c.variance)
    L = np.linalg.cholesky(K)
    err = np.abs(r["cols"][:, picks] - L.T).max()
    print(f"{c.id}: max |cols[:, picks] - chol(K)'| = {err:.3e}")
    assert err <= 1e-10


@pytest.mark.parametrize("c", G.CASES, ids=IDS)
def test_residuals_are_nystrom_residuals_and_each_pick_is_the_greedy_pick(c):
    r = G.run_case(c)
    x, ell, picks = G.data(c), G.ell_of(c), r["indices"]
    m = len(picks)
    before, _, _ = G.replay(x, ell, c.kernel, c.variance, picks)
    worst = 0.0
    for k in sorted({1, 2, m // 3, m // 2, m - 1, m}):  # the residual after k steps, from a direct solve
        if not 1 <= k <= m:
            continue
        direct = G.nystrom_residual(x, x[picks[:k]], ell, c.kernel, c.variance)
        ours = before[k] if k < m else r["d"]
        worst = max(worst, np.abs(ours - direct).max() / c.variance)
        if k < m:  # pick k is the brute-force argmax of that diagonal (to what the direct solve resolves)
            assert direct[picks[k]] >= direct.max() - 1e-9 * c.variance
    print(f"{c.id}: max |d - diag(K - Q)| / variance = {worst:.3e}")
    assert worst <= 1e-9
    for j in range(m):  # and of the run's own diagonal, exactly, the first holder on a tie
        assert picks[j] == int(np.argmax(before[j]))
    assert np.array_equal(before.max(axis=1) / c.variance, r["max_residual"])


@pytest.mark.parametrize("c", G.CASES, ids=IDS)
def test_max_residual_does_not_increase_and_the_trace_decreases(c):
    r = G.run_case(c)
    mx, tr = r["max_residual"], r["trace"]
    assert mx[0] == 1.0 and (np.diff(mx) <= 0).all()
    assert tr[0] < c.N and (np.diff(tr) < 0).all()
    assert r["last"] <= mx[-1]
    # the decoded integer sum is the float64 sum of the residuals to half a quantum per point
    assert abs(tr[-1] - r["d"].sum() / c.variance) <= c.N * 2.0 ** -(G.trace_shift(c.N) + 1) + 1e-12 * tr[-1]


def test_which_cases_qualify_for_the_exact_index_test():
    q = [c for c in G.CASES if G.qualifies(G.run_case(c))]
    for c in G.CASES:
        g = G.run_case(c)["gaps"][1:]
        print(f"{c.id}: smallest gap of the two largest residuals after the first step = {g.min():.3e} variance")
    assert len(q) >= 3 and len({str(c.kernel) for c in q}) >= 3
    # the squared-exponential cases do not: points far from every pivot keep d = variance bit for bit
    assert not any(c.kernel == "se" for c in q)
    assert {c.D for c in G.CASES} == {1, 3, 16} and len({str(c.kernel) for c in G.CASES}) == 5
    assert min(c.N for c in G.CASES) == 777 and max(c.M for c in G.CASES) == 300 and all(c.variance != 1.0 for c in G.CASES)


def test_threshold_margin():
    ended = 0
    for c in G.CASES:
        r = G.run_case(c)
        if len(r["indices"]) == c.M:
            continue
        ended += 1
        assert r["last"] <= c.threshold  # it ended by the threshold
        assert (np.abs(np.append(r["max_residual"], r["last"]) - c.threshold) >= G.THRESHOLD_MARGIN).all()
    assert ended >= 2


def test_step_is_the_run_and_duplicates_leave_a_zero():
    c = G.CASES[0]
    r = G.run_case(c)
    x, ell = G.data(c), G.ell_of(c)
    before, cols, _ = G.replay(x, ell, c.kernel, c.variance, r["indices"])
    j = 17
    col, dn, mag = G.step(x, ell, c.kernel, c.variance, cols[:j], before[j], int(r["indices"][j]))
    assert np.array_equal(col, r["cols"][j]) and np.array_equal(dn, before[j + 1])
    assert (mag >= np.abs(col) * np.sqrt(before[j][r["indices"][j]]) - 1e-300).all()
    # a duplicated row: after its twin is picked its own residual is exactly zero and it is never picked
    xd = x.copy()
    xd[r["indices"][3] + 7] = xd[r["indices"][3]]
    rd = G.run(xd, ell, c.kernel, c.variance, c.M, c.threshold)
    assert rd["indices"][3] == r["indices"][3] and r["indices"][3] + 7 not in rd["indices"]
