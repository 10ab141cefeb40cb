"""CPU tests of tests/inducing_reference.py, the yardstick of tests/test_gpu_inducing.py: on the data of every GPU case the float64
Lloyd run has no near tie (so the cap of the assignment check hides nothing), no empty centre and a cost that never rises; the numpy
model of the fixed-point rule stays inside the bars of the GPU tests' accumulator and centre checks, and three wrong variants of
it leave them."""
import numpy as np
import pytest

import inducing_reference as R


@pytest.fixture(scope="module")
def runs():
    """Per Lloyd case: (x, ell, bound, [z_0 .. z_NITER], costs, near-tie counts, empty counts) -- computed once."""
    out = {}
    for c in R.LLOYD:
        x, ell = R.data(c), R.ell_of(c)
        zs, costs, near, empty = [R.start(c, x)], [], [], []
        for _ in range(R.NITER):
            z, _, cost, nt, em = R.lloyd_step(x, zs[-1], ell)
            zs.append(z)
            costs.append(cost)
            near.append(int(nt.sum()))
            empty.append(em)
        out[c.id] = (x, ell, R.bound_of(x, ell), zs, costs, near, empty)
    return out


@pytest.mark.parametrize("c", R.LLOYD, ids=[c.id for c in R.LLOYD])
def test_reference_has_no_near_tie_no_empty_centre_and_a_falling_cost(runs, c):
    _, _, _, _, costs, near, empty = runs[c.id]
    assert near == [0] * R.NITER    # no point is left out of the assignment check: its cap hides nothing
    assert empty == [0] * R.NITER
    assert all(b <= a for a, b in zip(costs, costs[1:])), costs


@pytest.mark.parametrize("c", [R.BIG_M, R.GLOBAL_ACC], ids=lambda c: c.id)
def test_single_step_cases_stay_under_the_cap(c):
    x, ell = R.data(c), R.ell_of(c)
    _, _, near = R.assignment(R.sqdist(x, R.start(c, x), ell))
    assert near.sum() <= R.TIE_CAP * c.N


def test_exact_tie_data_has_ties_and_exact_distances():
    c = R.CASES[1]
    x = R.data(c, quarter=True)
    r2 = R.sqdist(x, R.start(c, x), np.ones(c.D))
    assert np.array_equal(r2 * 16.0, np.rint(r2 * 16.0))  # multiples of 1/16: exact in float64 in any order, fused or not
    two = np.partition(r2, 1, axis=1)[:, :2]
    assert (two[:, 0] == two[:, 1]).sum() >= 20  # exact ties do occur: the lowest-index rule is exercised


@pytest.mark.parametrize("c", R.LLOYD, ids=[c.id for c in R.LLOYD])
def test_fixed_point_model_stays_inside_the_bars(runs, c):
    x, ell, bound, zs, costs, _, _ = runs[c.id]
    z = zs[0]
    for it in range(R.NITER):
        z, acc, cost = R.fixed_point_step(x, z, ell, bound)
        assert acc[:, 0].sum() == c.N and np.abs(acc).max() < 2 ** 62
        assert np.abs(z - zs[it + 1]).max() <= 8e-15 * bound * ell.max()  # the issue's figure for the rule's own error
        assert abs(cost - costs[it]) <= 1e-9 * costs[it]
    assert (np.abs(z - zs[-1]) <= 1e-10 * bound * ell).all()


@pytest.mark.parametrize("variant", ["wrong-quantum", "no-count", "no-ell"])
def test_wrong_variants_leave_the_bars(runs, variant):
    """Each wrong rule breaks the accumulator check (array_equal with the stated rule) or the centre check (1e-10 bound ell) on at
    least one case; "no-ell" can only show where ell != 1."""
    seen = False
    for c in R.LLOYD:
        x, ell, bound, zs, _, _, _ = runs[c.id]
        z_ok, acc_ok, _ = R.fixed_point_step(x, zs[0], ell, bound)
        z_bad, acc_bad, _ = R.fixed_point_step(x, zs[0], ell, bound, variant)
        acc_differs = not np.array_equal(acc_ok, acc_bad)
        z_leaves = not (np.abs(z_bad - zs[1]) <= 1e-10 * bound * ell).all()
        if variant == "no-ell":
            assert z_leaves == (c.ell is not None)
        elif variant == "no-count":
            assert acc_differs and z_leaves  # the sums wrap
        else:
            assert acc_differs
        seen = seen or acc_differs or z_leaves
    assert seen


def test_fused_distance_is_the_plain_one_within_rounding_and_equal_where_exact():
    c = R.CASES[2]
    x, ell = R.data(c)[:400], R.ell_of(c)
    z = R.start(c, R.data(c))
    r2 = R.sqdist(x, z, ell)
    a = np.argmin(r2, axis=1)
    f = R.fused_r2(x, z, ell, a)
    plain = r2[np.arange(400), a]
    assert (np.abs(f - plain) <= (c.D + 1) * 2.0 ** -52 * plain).all() and not np.array_equal(f, plain)
    xq = R.data(c, quarter=True)[:400]
    zq = R.start(c, R.data(c, quarter=True))
    r2q = R.sqdist(xq, zq, ell)
    aq = np.argmin(r2q, axis=1)
    assert np.array_equal(R.fused_r2(xq, zq, ell, aq), r2q[np.arange(400), aq])


def test_rule_matches_its_statement():
    assert R.quanta(8.5, 5000, 1) == (44, 38)
    assert R.quanta(1.0, 4096, 16) == (48, 41)
    for bound, N, D in [(8.5, 5000, 1), (0.3, 10 ** 7, 16), (1e6, 300, 3)]:
        sx, sd = R.quanta(bound, N, D)
        assert N * (bound * 2.0 ** sx) <= 2.0 ** 61 and N * (4 * D * bound * bound * 2.0 ** sd) <= 2.0 ** 61
        assert 2 * N * (bound * 2.0 ** sx) > 2.0 ** 59  # and not wastefully coarse


def test_shapes_cover_every_path_of_the_step():
    assert [R.lds_accumulator(c.M, c.D) for c in R.STEP_CASES] == [True, True, True, True, True, False, True]
    assert {R.tile_points(c.D) for c in R.STEP_CASES} == {1024, 2048}
    assert R.BIG_M.M == 2048 and any(c.M > 256 for c in R.CASES) and any(c.D == 16 for c in R.CASES)
