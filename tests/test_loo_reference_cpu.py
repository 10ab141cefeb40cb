"""tests/loo_reference.py held to itself, CPU-only: the closed form of the leave-one-out cavity against the brute-force refit (one
M x M inverse per site), the leverage sum against M - tr S, the float32-input route (the header's rule, include/agpl_loo.h) against the
closed form under the bound of the float32 marginals, every row of the header's table of special cases, and the order of lev_sum."""
import numpy as np
import pytest

import loo_reference as R

f64, f32 = np.float64, np.float32


@pytest.fixture(scope="module")
def world():
    c = R.case(N=300, M=40, L=2, seed=7, high=0.99)
    c["closed"] = R.closed_form(c["Phi"], c["d"], c["gamma"], c["beta"], c["mu0"], c["eta0"])
    c["refit"] = R.refit(c["Phi"], c["d"], c["gamma"], c["beta"], c["mu0"], c["eta0"])
    return c


def test_the_case_holds_what_it_says(world):
    h = world["closed"][2]
    assert 0.985 < h[0, 0] < 0.995  # the isolated point
    assert np.all(h[:, 1] == 0) and np.all(world["gamma"][:, 1] == 0)
    assert np.all(h >= 0) and np.all(h < 1)
    assert world["mu0"] is not None and world["eta0"] is not None


def test_closed_form_is_the_refit(world):
    (mu, var, _), (mu_r, var_r) = world["closed"], world["refit"]
    em = np.abs(mu - mu_r).max() / np.abs(mu_r).max()
    ev = np.abs(var - var_r).max() / np.abs(var_r).max()
    ep = (np.abs(var - var_r) / np.abs(var_r)).max()  # entry-wise too: the point at h = 0.99 has the largest variance
    print(f"closed form against {mu.size} refits: mean {em:.2e}, variance {ev:.2e} of max, {ep:.2e} entry-wise")
    assert em < 1e-10 and ev < 1e-10 and ep < 1e-10


def test_closed_form_is_the_refit_without_mu0_and_eta0():
    c = R.case(N=60, M=12, L=1, seed=3, with_mu0=False, with_eta0=False)
    mu, var, _ = R.closed_form(c["Phi"], c["d"], c["gamma"], c["beta"])
    mu_r, var_r = R.refit(c["Phi"], c["d"], c["gamma"], c["beta"])
    assert np.abs(mu - mu_r).max() < 1e-10 * np.abs(mu_r).max() and np.abs(var - var_r).max() < 1e-10 * np.abs(var_r).max()


def test_leverages_sum_to_the_effective_number_of_parameters(world):
    S, _, _, _ = R.posterior(world["Phi"], world["gamma"], world["beta"], world["eta0"])
    M = world["Phi"].shape[1]
    h = world["closed"][2]
    for l in range(h.shape[0]):
        want = M - np.trace(S[l])
        assert abs(h[l].sum() - want) < 1e-10 * want, (l, h[l].sum(), want)


def test_float32_inputs_stay_inside_their_bound(world):
    """The rule fed with the float32 roundings of the exact marginals: mu and var each carry at most 2^-24 relative.  Carried through
    the formulas, d var_-i = d var / (1 - h)^2 and d mu_-i = d mu / (1 - h) + |(a - beta q) gamma + beta (1 - h)| d var / (1 - h)^2:
    bars of 2^-23 var / (1 - h)^2 for the variance (the issue's: twice the rounding of var) and the same form with mu's own rounding
    for the mean."""
    c = world
    S, m, _, _ = R.posterior(c["Phi"], c["gamma"], c["beta"], c["eta0"])
    mu64, var64 = R.marginals(c["Phi"], c["d"], S, m, c["mu0"])
    out = R.rule(mu64.astype(f32), var64.astype(f32), c["d"], c["gamma"], c["beta"], c["mu0"])
    assert out["n_bad"] == 0 and out["first_bad"] == -1
    mu_c, var_c, h = c["closed"]
    u = 2.0 ** -23
    g, b = c["gamma"].astype(f64), c["beta"].astype(f64)
    q = var64 - c["d"].astype(f64)[None]
    a = mu64 - c["mu0"].astype(f64)
    bar_v = u * var64 / (1 - h) ** 2
    bar_m = u * np.abs(mu64) / (1 - h) + (np.abs(a - b * q) * g + np.abs(b) * (1 - h)) * u * var64 / (1 - h) ** 2
    rv = np.abs(out["var"].T - var_c) / bar_v
    rm = np.abs(out["mu"].T - mu_c) / bar_m
    print(f"float32-input route: worst |var - closed| / bar {rv.max():.3f} (at h = {h.flat[rv.argmax()]:.3f}), mean {rm.max():.3f}; "
          f"relative error of the variance at the h = 0.99 point {abs(out['var'][0, 0] - var_c[0, 0]) / var_c[0, 0]:.2e}")
    assert rv.max() <= 1.0 and rm.max() <= 1.0
    assert np.abs(out["lev"].T - h).max() <= u * (g * var64).max()


def _one(mu, var, d, g, b, m0=None):
    a32 = lambda x: np.array([[x]], f32)
    return R.rule(a32(mu), a32(var), np.array([d], f32), a32(g), a32(b), None if m0 is None else a32(m0))


def test_table_gamma_zero_is_the_marginal_with_the_linear_site_out():
    o = _one(0.75, 1.5, 0.25, 0.0, 2.0, m0=0.5)
    q = 1.25
    assert o["lev"][0, 0] == 0.0 and o["n_bad"] == 0
    assert o["var"][0, 0] == 0.25 + q  # resid + q
    assert o["mu"][0, 0] == 0.5 + ((0.75 - 0.5) - 2.0 * q)  # mu - beta q, through mu0 as the rule orders it
    assert o["mu"][0, 0] == 0.75 - 2.0 * q  # (these numbers are exact in binary: the two forms agree to the bit)
    assert o["h_in"][0, 0] == 0.0


@pytest.mark.parametrize("mu,var,g,b", [
    (0.1, 1.25, 1.0, 0.3),        # h = 1 exactly
    (0.1, 1.25, 4.0, 0.3),        # h > 1
    (0.1, 1.25, -0.5, 0.3),       # gamma < 0
    (0.1, 1.25, np.nan, 0.3), (0.1, 1.25, np.inf, 0.3),
    (0.1, 1.25, 0.5, np.inf), (0.1, 1.25, 0.5, np.nan), (0.1, 1.25, 0.0, -np.inf),
    (np.nan, 1.25, 0.5, 0.3), (np.inf, 1.25, 0.5, 0.3),
    (0.1, np.nan, 0.5, 0.3), (0.1, np.inf, 0.5, 0.3),
])
def test_table_pairs_without_a_cavity_are_nan_and_counted(mu, var, g, b):
    o = _one(mu, var, 0.25, g, b)
    assert np.isnan(o["mu"][0, 0]) and np.isnan(o["var"][0, 0]) and np.isnan(o["lev"][0, 0])
    assert o["n_bad"] == 1 and o["first_bad"] == 0 and o["h_in"][0, 0] == 0.0


def test_table_count_and_lowest_flat_index():
    L, N = 3, 7
    mu = np.full((L, N), 0.1, f32)
    var = np.full((L, N), 1.0, f32)
    d = np.full(N, 0.5, f32)
    g = np.full((L, N), 0.5, f32)
    b = np.full((L, N), 0.2, f32)
    g[2, 1] = -1
    g[1, 4] = np.nan
    b[1, 6] = np.inf
    o = R.rule(mu, var, d, g, b)
    assert o["n_bad"] == 3 and o["first_bad"] == 1 * N + 4
    assert np.isnan(o["var"][4, 1]) and np.isnan(o["var"][1, 2]) and np.isnan(o["var"][6, 1])
    assert np.isfinite(o["var"]).sum() == L * N - 3
    assert o["mu"].shape == (N, L)  # point-major


def test_table_q_negative_by_round_off_is_zero():
    o = _one(0.3, 0.25 - 2.0 ** -26, 0.25, 0.7, 0.4, m0=0.1)  # var a float32 step below the residual
    assert o["n_bad"] == 0 and o["lev"][0, 0] == 0.0
    assert o["var"][0, 0] == f64(f32(0.25)) and o["mu"][0, 0] == f64(f32(0.1)) + (f64(f32(0.3)) - f64(f32(0.1)))


def test_table_negative_zero_gamma_is_gamma_zero():
    o = _one(0.75, 1.5, 0.25, -0.0, 2.0)
    assert o["n_bad"] == 0 and o["var"][0, 0] == 1.5 and o["lev"][0, 0] == 0.0


@pytest.mark.parametrize("N", [1, 255, 257, 2049, 256 * 1024 + 300])
def test_lev_sum_order_is_a_sum(N):
    rng = np.random.default_rng(N)
    h = rng.random((2, N))
    h[1, ::7] = 0.0
    s = R.lev_sum(h)
    exact = np.array([float(np.sum(h[l].astype(np.longdouble))) for l in range(2)])
    assert np.all(np.abs(s - exact) <= 64 * 2.0 ** -53 * exact)  # (a tree of depth <= 6 + log2 of the partials + the tiles of a workgroup)
