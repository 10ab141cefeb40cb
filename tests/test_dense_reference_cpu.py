"""The reference side of tests/test_gpu_dense_tiles.py, checked on its own (no GPU): tests/dense_reference.py.

What this module proves:
  * the numpy model of the two blocked factorisations equals LAPACK;
  * its block widths are the ones written in csrc/agpl_dense.hip;
  * on the two new matrix families every tile of every trailing update and every row tile of every panel product contributes more
    than the device tests' bar (invisible share exactly 0), at N = 8192, 8192 + 1001 and 9216 on the look-ahead route, 8192 and 9216 on the
    inverse-block route, and for the look-ahead step's own B at 8192 + 300 (the dense step's counts use the c of its own bar);
  * on the existing dense tests' matrices most tiles contribute nothing that bar could see (measured, full size, numpy draws of the
    same constants; share of tiles whose every entry is at or below a LOWER bound of the bar):
        matrix                     update tiles (all)    outer updates alone    panel row tiles
        cholesky_blocked_route     0.947 (8269 / 8736)   0.994 (2736 / 2752)    in-block panel_solve 0.560
        cholesky_odd_order         0.947 (8269 / 8736)   0.994 (2736 / 2752)    in-block panel_solve 0.560
        gibbs_blocked_routes       0.911 (7414 / 8136)   0.989 (2128 / 2152)    in-block panel_solve 0.318
        gibbs_inverse_block        0.990 (4544 / 4592)   0.990                  gemm_nt_assign 0.786 (176 / 224)
    The update share is above 0.9 everywhere, as the arithmetic of the band predicts.  The panel product's row tiles of the
    inverse-block route are 0.786 invisible, NOT above 0.9: a panel is 1024 columns wide and the band (about 790 indices) reaches
    the first 6 or 7 of the 8 to 56 row tiles below it, a fifth of all row tiles at N = 8192.  That assertion is kept at the measured
    value (> 0.78);
  * every injected wrong tile is rejected by the device tests' comparison functions on the new families and leaves the result
    bit-identical on an existing matrix.

Time: the full-size counts take about 15 s per look-ahead run and 4 s per inverse-block run in numpy on 8 cores (the 64-column steps
inside a diagonal block are Python loops), several minutes for the module (it is the slowest CPU module of the suite).  The fault injections therefore run with every width divided
by 4 (tile 32, stage 4, inner block 16, blocks 512 and 256) at N = 2048 and 2048 + 251: four look-ahead blocks (the last one ragged),
eight inverse blocks; a dropped stage and a stale U_k are injected once more at N = 8192 with the source's widths, on both families
(measured: 321 x and 1.6e4 x the bar on exp_perm, 1.1e3 x and 7.1e4 x on wishart).
"""
import numpy as np
import pytest
import scipy.linalg as sla

import dense_reference as R

BL = R.Blocking.from_source()
BL4 = BL.scaled(4)
C_VIS = 3.0  # the margin the visibility counts use: above c_chain + c_eval = 2.01 (c_inv is added per matrix where it is known)


def test_constants_are_the_sources():
    c = R.read_constants()
    assert c == {"kTT": 128, "kTK": 16, "kPB": 64, "kDB": 1024, "NB": 2048, "THRESHOLD": 8192}, c
    assert (BL.tt, BL.tk, BL.pb, BL.nb, BL.db) == (128, 16, 64, 2048, 1024)
    # the shapes of the device module are the smallest that reach the routes, and they depend on these widths
    assert c["THRESHOLD"] % c["NB"] == 0 and c["THRESHOLD"] % c["kDB"] == 0 and 9216 % c["kDB"] == 0 and 9216 % c["NB"] != 0


def test_tile_index_round_trip():
    for nt in (1, 2, 7, 48, 56):
        seen = [R.tile_of_index(nt, i) for i in range(R.tri_tiles_before(nt, nt))]
        assert seen == [(I, J) for J in range(nt) for I in range(J, nt)]


# ---------------------------------------------------------------------------------------------- full size: model, visibility
_full = {}


def full_size(family, N):
    """(K, Lref) once per (family, N)"""
    if (family, N) not in _full:
        K = R.FAMILIES[family](N)
        _full[(family, N)] = (K, np.linalg.cholesky(K))
    return _full[(family, N)]


@pytest.mark.parametrize("family", ["exp_perm", "wishart"])
@pytest.mark.parametrize("N", [8192, 8192 + 1001, 9216])
def test_lookahead_model_equals_lapack_and_every_tile_is_visible(family, N):
    K, Lref = full_size(family, N)
    assert K.min() > (np.exp(-2.0) if family == "exp_perm" else -1.0)
    c, parts = R.factor_margin(Lref, BL)
    watch = R.Watch(K, max(C_VIS, c))
    L = R.lookahead_cholesky(K, BL, watch=watch)
    # forward agreement with LAPACK: both are backward stable, so they differ by cond_2(K) n u at the most
    ev = (1e-2, N) if family == "exp_perm" else (1.0, 4.0 * N / 64)  # (bounds of the spectrum: Gershgorin; Marchenko-Pastur edge x 2)
    assert np.abs(L - Lref).max() <= (ev[1] / ev[0]) * N * R.U * np.abs(Lref).max(), np.abs(L - Lref).max()
    print(family, N, "c =", c, parts, watch.counts)
    for tag in ("outer", "inner", "inner_panel"):
        assert watch.counts[tag][1] == watch.counts[tag][0], (tag, watch.counts[tag], watch.dark[:5])
    assert watch.share_visible(["outer", "inner", "inner_panel"]) == 1.0 and not watch.dark  # invisible share: exactly 0
    del _full[(family, N)]


def _step_margin(B, Cref):
    """c of bar (b) for this B: what the visibility counts of the dense step's matrix use"""
    N = B.shape[0]
    bmin, bmax, acc = R.power_norms(B, Cref)
    nb = N - N % BL.db
    return R.step_c(N, bmax, acc, 3.0 * 2.0 * BL.db * R.cond_of_blocks(Cref[:nb, :nb], BL.db) / N, BL)


@pytest.mark.parametrize("family", ["exp_perm", "wishart"])
@pytest.mark.parametrize("N", [8192, 9216])
def test_inverse_block_model_equals_lapack_and_every_tile_is_visible(family, N):
    """and, at N = 8192 with the source's widths, the step comparison rejects a dropped stage and a stale U_k"""
    K = R.FAMILIES[family](N)
    gamma = R.student_like_gamma(N)
    B = R.gibbs_matrix(K, gamma)
    Cref = np.linalg.cholesky(B)
    c_step = _step_margin(B, Cref)
    watch = R.Watch(B, max(C_VIS, c_step))
    L, Us = R.inverse_block_factor(B, BL, watch=watch)
    nrm = np.linalg.norm(B, 1)  # >= ||B||_2; B >= I
    assert np.abs(L - Cref).max() <= nrm * N * R.U * np.abs(Cref).max(), np.abs(L - Cref).max()
    r = np.random.default_rng(N).standard_normal(N)
    s = R.inverse_block_solve(L, Us, BL, r)
    s_ref = sla.cho_solve((Cref, True), r)
    assert np.linalg.norm(s - s_ref) <= nrm * N * R.U * 3 * np.linalg.norm(s_ref)
    print(family, N, "c of the step bar = %.4g" % c_step, watch.counts)
    assert N // BL.db >= 8 and watch.counts["panel"][0] == sum(-(-(N - e) // BL.tt) for e in range(BL.db, N, BL.db))
    assert watch.share_visible(["outer", "panel"]) == 1.0 and not watch.dark
    if N != 8192:
        return
    Lk = np.linalg.cholesky(K)
    _, beta, z, mu0 = _step_inputs(K, N, 1)
    f_ref, d = R.gibbs_f(K, Lk, mu0, beta, gamma, z, lambda r: sla.cho_solve((Cref, True), r))
    bar, parts = R.step_bar_from_reference(K, Lk, B, Cref, gamma, z[:N], d["s"], BL, f_ref)
    f, _ = R.gibbs_f(K, Lk, mu0, beta, gamma, z, lambda r: R.inverse_block_solve(L, Us, BL, r))
    print(family, "clean model: max|f - ref| = %.3g, bar = %.3g %s" % (np.abs(f - f_ref).max(), bar, parts))
    assert np.abs(f - f_ref).max() <= bar
    nt0, nt1 = (N - BL.db) // BL.tt, (N - 2 * BL.db) // BL.tt
    for name, fault in (("drop_stage", R.Fault("drop_stage", 0, (nt0 - 1, 0))), ("stale_u", R.Fault("stale_u", 1, nt1 - 1))):
        Lf, Uf = R.inverse_block_factor(B, BL, fault=fault)
        assert fault.hit == 1, name
        ff, _ = R.gibbs_f(K, Lk, mu0, beta, gamma, z, lambda r: R.inverse_block_solve(Lf, Uf, BL, r))
        print(family, name, "max|f - ref| = %.3g = %.3g x bar" % (np.abs(ff - f_ref).max(), np.abs(ff - f_ref).max() / bar))
        assert np.abs(ff - f_ref).max() > bar, (name, np.abs(ff - f_ref).max(), bar, parts)


def test_lookahead_step_matrix_every_tile_is_visible():
    """B = I + D^1/2 K D^1/2 of the look-ahead dense step (test_lookahead_step_on_a_dense_prior: wishart, N = 8192 + 300)"""
    N = 8192 + 300
    B = R.gibbs_matrix(R.wishart(N), R.student_like_gamma(N))
    c_step = _step_margin(B, np.linalg.cholesky(B))
    watch = R.Watch(B, max(C_VIS, c_step))
    R.lookahead_cholesky(B, BL, watch=watch)
    print("lookahead step B", N, "c of the step bar = %.4g" % c_step, watch.counts)
    assert watch.share_visible(["outer", "inner", "inner_panel"]) == 1.0 and not watch.dark


# measured at full size (this module's docstring); the update shares are asserted above 0.9, the panel share at what it is
@pytest.mark.parametrize("name,update_tags,panel_tag,panel_floor", [
    ("cholesky_blocked_route", ("outer", "inner"), "inner_panel", None),
    ("cholesky_odd_order", ("outer", "inner"), "inner_panel", None),
    ("gibbs_blocked_routes", ("outer", "inner"), "inner_panel", None),
    ("gibbs_inverse_block", ("outer",), "panel", 0.78),
])
def test_existing_matrices_leave_most_tiles_invisible(name, update_tags, panel_tag, panel_floor):
    _, route, N, span, ell, jitter, seed = [e for e in R.EXISTING if e[0] == name][0]
    K = R.se_sorted(N, span, ell, jitter, seed)
    if name.startswith("gibbs"):
        K = R.gibbs_matrix(K, R.student_like_gamma(N))
    watch = R.Watch(K, C_VIS)
    if route == "lookahead":
        R.lookahead_cholesky(K, BL, watch=watch)
    else:
        R.inverse_block_factor(K, BL, watch=watch)
    print(name, watch.counts, "update", watch.share_invisible(update_tags), "panel", watch.share_invisible([panel_tag]))
    assert watch.share_invisible(update_tags) > 0.9
    assert watch.share_invisible(["outer"]) > 0.9  # the N^3 / 3 launches alone
    if panel_floor is not None:
        assert watch.share_invisible([panel_tag]) > panel_floor


# ---------------------------------------------------------------------------------------------- sensitivity (all widths / 4)
def _lookahead_faults(N):
    nt = -(-(N - BL4.nb) // BL4.tt)
    return {
        "skip": R.Fault("skip", 0, (nt - 2, 0)),
        "drop_stage": R.Fault("drop_stage", 0, (nt - 2, 0)),
        "swap": R.Fault("swap", 0, (nt - 2, 0), (nt - 3, 1)),
        "late_launch": R.Fault("late_launch", 0),
    }


def _inverse_faults(N):
    nt0, nt1 = (N - BL4.db) // BL4.tt, (N - 2 * BL4.db) // BL4.tt
    return {
        "skip": R.Fault("skip", 0, (nt0 - 1, 0)),
        "drop_stage": R.Fault("drop_stage", 0, (nt0 - 1, 0)),
        "swap": R.Fault("swap", 0, (nt0 - 1, 0), (nt0 - 2, 1)),
        "stale_u": R.Fault("stale_u", 1, nt1 - 1),
    }


@pytest.fixture(scope="module")
def small_lookahead():
    out = {}
    for family in ("exp_perm", "wishart"):
        for N in (2048, 2048 + 251):
            K = R.FAMILIES[family](N, p=16) if family == "wishart" else R.FAMILIES[family](N)
            Lref = np.linalg.cholesky(K)
            out[(family, N)] = (K, Lref, np.abs(Lref) @ np.abs(Lref).T, R.factor_margin(Lref, BL4)[0])
    return out


@pytest.mark.parametrize("family", ["exp_perm", "wishart"])
@pytest.mark.parametrize("N", [2048, 2048 + 251])
def test_lookahead_faults_are_rejected_on_the_new_matrices(small_lookahead, family, N):
    K, Lref, absLL, c = small_lookahead[(family, N)]
    L = R.lookahead_cholesky(K, BL4)
    ok, worst, msg = R.check_factor(K - L @ L.T, absLL, c, BL4)
    assert ok, msg  # the unbroken model passes the device test's comparison
    for name, fault in _lookahead_faults(N).items():
        try:
            Lf = R.lookahead_cholesky(K, BL4, fault=fault)
        except np.linalg.LinAlgError:  # a pivot went non-positive: the device reports AGPL_ERR_NOT_POSDEF, which fails the test too
            assert fault.hit >= 1, name
            continue
        assert fault.hit >= 1, name
        ok, worst, msg = R.check_factor(K - Lf @ Lf.T, absLL, c, BL4)
        assert not ok, (name, msg)


@pytest.mark.parametrize("name", ["cholesky_blocked_route", "cholesky_odd_order"])
def test_lookahead_faults_are_invisible_on_an_existing_matrix(name):
    _, _, N, span, ell, jitter, seed = [e for e in R.EXISTING if e[0] == name][0]
    N4 = N // 4 + (N % 2)  # (keeps the odd order odd)
    K = R.se_sorted(N4, span, ell, jitter, seed)  # a quarter of the points on the same span: the band stays 3.5 tiles wide
    L = R.lookahead_cholesky(K, BL4)
    for fname, fault in _lookahead_faults(N4).items():
        Lf = R.lookahead_cholesky(K, BL4, fault=fault)
        assert fault.hit >= 1, fname
        assert np.array_equal(L, Lf), fname  # bit for bit: that test cannot see this fault


def _step_inputs(K, N, seed):
    rng = np.random.default_rng([seed, N, 7])
    gamma = R.student_like_gamma(N)
    return gamma, rng.standard_normal(N), rng.standard_normal(2 * N), 0.5 + 0.25 * np.cos(np.arange(N))


@pytest.mark.parametrize("family", ["exp_perm", "wishart"])
def test_inverse_block_faults_are_rejected_on_the_new_matrices(family):
    N = 2048
    K = R.FAMILIES[family](N, p=16) if family == "wishart" else R.FAMILIES[family](N)
    Lk = np.linalg.cholesky(K)
    gamma, beta, z, mu0 = _step_inputs(K, N, 1)
    B = R.gibbs_matrix(K, gamma)
    Cref = np.linalg.cholesky(B)
    f_ref, d = R.gibbs_f(K, Lk, mu0, beta, gamma, z, lambda r: sla.cho_solve((Cref, True), r))
    bar, parts = R.step_bar_from_reference(K, Lk, B, Cref, gamma, z[:N], d["s"], BL4, f_ref)
    assert bar <= R.FLAT_F * max(1.0, np.abs(f_ref).max())  # never above the existing dense-step tests' bar
    L, Us = R.inverse_block_factor(B, BL4)
    f, _ = R.gibbs_f(K, Lk, mu0, beta, gamma, z, lambda r: R.inverse_block_solve(L, Us, BL4, r))
    assert np.abs(f - f_ref).max() <= bar, (np.abs(f - f_ref).max(), bar)
    for name, fault in _inverse_faults(N).items():
        try:
            Lf, Uf = R.inverse_block_factor(B, BL4, fault=fault)
        except np.linalg.LinAlgError:  # (as above)
            assert fault.hit >= 1, name
            continue
        assert fault.hit >= 1, name
        ff, _ = R.gibbs_f(K, Lk, mu0, beta, gamma, z, lambda r: R.inverse_block_solve(Lf, Uf, BL4, r))
        assert np.abs(ff - f_ref).max() > bar, (name, np.abs(ff - f_ref).max(), bar, parts)


def test_inverse_block_faults_are_invisible_on_an_existing_matrix():
    _, _, N, span, ell, jitter, seed = [e for e in R.EXISTING if e[0] == "gibbs_inverse_block"][0]
    N4 = N // 4
    K = R.se_sorted(N4, span, ell, jitter, seed)
    Lk = np.linalg.cholesky(K)
    gamma, beta, z, mu0 = _step_inputs(K, N4, 2)
    B = R.gibbs_matrix(K, gamma)
    L, Us = R.inverse_block_factor(B, BL4)
    f, _ = R.gibbs_f(K, Lk, mu0, beta, gamma, z, lambda r: R.inverse_block_solve(L, Us, BL4, r))
    for name, fault in _inverse_faults(N4).items():
        Lf, Uf = R.inverse_block_factor(B, BL4, fault=fault)
        assert fault.hit >= 1, name
        ff, _ = R.gibbs_f(K, Lk, mu0, beta, gamma, z, lambda r: R.inverse_block_solve(Lf, Uf, BL4, r))
        assert np.array_equal(f, ff), name
