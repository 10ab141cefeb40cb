"""CPU checks of tests/pathwise_reference.py (no GPU, no library code): the spectral rule against kappa, the covariance of the
reference's draws against C_model, C_model against the exact posterior covariance as F grows, the numpy model of the device
arithmetic inside the element-wise bars on the data of every GPU case, and every wrong variant outside them."""
import numpy as np
import pytest

import chain_reference as CR
import pathwise_reference as R


@pytest.mark.parametrize("kind", R.KINDS)
def test_spectral_rule_gives_the_kernel(kind):
    """|mean_j cos(omega_j . Delta) - kappa(r)| <= 5 Monte-Carlo standard deviations, 5 / sqrt(2 F) (Var cos <= 1/2), F = 200000."""
    F, D = 200_000, 3
    rng = np.random.default_rng(2024)
    omega, _ = R.spectral(kind, F, D, rng, R.ALPHA)
    e = np.ones(D) / np.sqrt(D)
    for r in (0.1, 0.5, 1.0, 2.0, 4.0):
        err = abs(np.cos(omega @ (r * e)).mean() - R.kappa(kind, r, R.ALPHA))
        print(f"{kind} r = {r}: err {err:.4f} (bar {5 / np.sqrt(2 * F):.4f})")
        assert err <= 5 / np.sqrt(2 * F)


def _small_world(F, seed=5, M=8, n=6):
    rng = np.random.default_rng(seed)
    z = np.linspace(-2, 2, M)[:, None]
    x = rng.uniform(-2.5, 2.5, size=(n, 1))
    ell, s2, jitter = np.array([0.8]), 1.3, 1e-3
    Linv = R.whitening("se", z / ell, 1.0, s2, jitter)
    Phi = R.phi_f64("se", x / ell, z / ell, 1.0, s2, Linv)
    A = 0.3 * rng.standard_normal((M, M))
    S = np.linalg.inv(np.eye(M) + A @ A.T)
    m = rng.standard_normal(M)
    omega, phase = R.spectral("se", F, 1, np.random.default_rng(seed + 1))
    return rng, x, z, ell, s2, jitter, Linv, Phi, S, m, omega, phase


def test_reference_draws_have_the_model_covariance():
    """The sample mean and covariance of 20000 reference draws against mu0 + phi' m and C_model: every entry within 5 sigma."""
    T, F = 20_000, 64
    rng, x, z, ell, s2, jitter, Linv, Phi, S, m, omega, phase = _small_world(F)
    s = np.sqrt(s2) * np.sqrt(2.0 / F)
    V = (m + rng.standard_normal((T, len(m))) @ np.linalg.cholesky(S).T)[:, None, :]
    W, Xi = rng.standard_normal((T, 1, F)), rng.standard_normal((T, 1, len(m)))
    PsiZ, Psi = R.psi_f64(z, ell, omega, phase), R.psi_f64(x, ell, omega, phase)
    f = R.reference(Phi, Psi, R.coefficients(V, W, Xi, PsiZ, Linv, s, jitter), W, s)[:, 0]
    Cm = R.c_model(Phi, Psi, PsiZ, Linv, S, s, jitter)
    err, bar = np.abs(np.cov(f.T, bias=True) - Cm), R.mc_bar(Cm, T)
    print(f"covariance: max |C| {np.abs(Cm).max():.3f}, max err {err.max():.4f}, max err / bar {np.max(err / bar):.3f}")
    assert (err <= bar).all()
    em, bm = np.abs(f.mean(0) - Phi @ m), 5 * np.sqrt(np.diag(Cm) / T)
    print(f"mean: max err / bar {np.max(em / bm):.3f}")
    assert (em <= bm).all()


def test_model_covariance_approaches_the_exact_one():
    """|C_model - C_exact| at F = 16384 is below half its value at F = 1024, on the same data."""
    gap = {}
    for F in (1024, 4096, 16384):
        _, x, z, ell, s2, jitter, Linv, Phi, S, m, omega, phase = _small_world(F)
        s = np.sqrt(s2) * np.sqrt(2.0 / F)
        Cm = R.c_model(Phi, R.psi_f64(x, ell, omega, phase), R.psi_f64(z, ell, omega, phase), Linv, S, s, jitter)
        Ce = R.c_exact(R.kernel_matrix("se", x / ell, x / ell, 1.0, s2), Phi, S)
        gap[F] = np.abs(Cm - Ce).max()
        print(f"F = {F}: max |C_model - C_exact| {gap[F]:.4f} at max |C_exact| {np.abs(Ce).max():.3f}")
    assert gap[16384] < 0.5 * gap[1024]


def _case_world(c):
    x, z, ell = R.case_inputs(c)
    Linv = R.whitening(c.kind, z / ell, 1.0, R.VARIANCE, c.jitter, R.ALPHA)
    image, Phi = CR.model_features(R.phi_f64(c.kind, x / ell, z / ell, 1.0, R.VARIANCE, Linv, R.ALPHA))
    draws = R.case_draws(c)
    ref, bars, cc = R.case_reference(c, Phi, x, z, ell, draws, image[2])
    return x, z, ell, Linv, image, draws, ref, bars


@pytest.fixture(scope="module")
def worlds():
    cache = {}

    def get(c):
        if c not in cache:
            cache[c] = _case_world(c)
        return cache[c]

    return get


def _run(c, world, mutate=None):
    x, z, ell, Linv, image, (omega, phase, V, W, Xi, mu0), ref, bars = world
    out = R.model(image, x, z, ell, omega, phase, V, W, Xi, Linv, R.VARIANCE, c.jitter, mu0, mutate)
    return np.max(np.abs(out.astype(np.float64) - ref) / bars.F)


@pytest.mark.parametrize("c", R.CASES, ids=lambda c: c.id)
def test_model_stays_within_the_bars(worlds, c):
    ratio = _run(c, worlds(c))
    print(f"{c.id}: model max err / bar {ratio:.3f}")
    assert ratio <= 1.0


# What the data cannot show: a draw-0 mix-up needs T > 1.  The Psi lo plane carries about 2^-12 of each psi, with random signs: its
# loss moves an output by about 2^-13 s |psi o W|_2, which the data of a case can show only where that exceeds the bar (the bar is
# led by |Phi|'|c| where c is large).  So that variant is asked to leave the bars (by 2, from what the CPU shows: 5.5 and 70 on the
# cases that qualify) on the cases where this figure, computed from the data alone, is at least twice the bar -- and at least two
# cases must qualify.  Every other variant leaves by 100 on every case (the CPU shows 870 at the least).
LEAVE = {m: 100.0 for m in R.MUTATIONS}
LEAVE["psi_without_lo_plane"] = 2.0


def _lo_plane_shows(c, world):
    x, z, ell, Linv, image, (omega, phase, V, W, Xi, mu0), ref, bars = world
    s = np.sqrt(R.VARIANCE) * np.sqrt(2.0 / c.F)
    Psi = R.psi_f64(x, ell, omega, phase)
    moved = 2.0 ** -13 * s * np.sqrt(np.einsum("nf,tlf->tln", Psi * Psi, W * W))
    return np.max(moved / bars.F) >= 2.0


SHOWN = [(c, m) for m in R.MUTATIONS for c in R.CASES
         if not (m == "every_draw_reads_w0" and c.T == 1) and not (m == "psi_without_lo_plane" and not _lo_plane_shows(c, _case_world(c)))]
assert sum(m == "psi_without_lo_plane" for _, m in SHOWN) >= 2


@pytest.mark.parametrize("c, mutate", SHOWN, ids=lambda v: v if isinstance(v, str) else v.id)
def test_wrong_variants_leave_the_bars(worlds, c, mutate):
    ratio = _run(c, worlds(c), mutate)
    print(f"{c.id} {mutate}: max err / bar {ratio:.1f}")
    assert ratio >= LEAVE[mutate]
