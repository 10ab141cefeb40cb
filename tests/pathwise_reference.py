"""Float64 reference, the covariance the draws have (C_model), the spectral rule, a numpy model of the device arithmetic and the
element-wise error bars of pathwise posterior draws (include/agpl_pathwise.h: agpl_plan_sample_paths), for
tests/test_gpu_pathwise.py and tests/test_pathwise_reference_cpu.py.  No GPU, no library code: nothing here imports the package.

reference
    psi_j(x) = cos(omega_j . x / ell + b_j);  s = sigma sqrt(2 / F);  up = s Psi(Z)' W + sqrt(jitter) Xi;  c = V - L^-1 up;
    F[t, l, i] = mu0 + s psi(x_i)' W_tl + phi(x_i)' c_tl,   phi = L^-1 k_Z(x),  K_ZZ + jitter I = L L'.

C_model (the covariance of the draws over W, Xi and V ~ (m, S), given omega and b)
    B = s (Psi(x) - Psi(Z) L^-T phi) [F, n],  q = L^-T phi [M, n]:   C = B'B + jitter q'q + phi' S phi.
    The exact posterior covariance is k - phi' phi + phi' S phi; the two differ by O(sigma^2 / sqrt(F)).

bars (element-wise, from the arithmetic the header documents; Phi is the plan's own features, hi + lo of its image, so Phi's split is
exact; tests/chain_reference.py derives the split's figures)
    An operand entry x is packed as x 2^e -> float32 -> float16 hi + float16 lo.  Relative parts: float32 rounding 2^-24 and the lo
    rounding 2^-22 per packed operand (c, s W; Psi is float32 already: 2^-22 only), the dropped lo lo product 2^-22.  So the phi part
    carries 2^-21 + 2^-24 and the psi part 3 2^-22 + 2^-24 <= 2^-20, and float32 accumulation over n_k = 16 ceil(M / 16) + Fp products
    adds n_k 2^-24 of the sum of all magnitudes:
        (2^-21 + n_k 2^-24) |Phi|'|c|  +  (2^-20 + n_k 2^-24) s |Psi|'|W|.
    Absolute parts (the shared scales; every packed entry is within 2^-25 of its scaled value beyond the relative part):
        2^-25 2^-ec sum_a |Phi_a|  +  2^-25 2^-ew sum_j |psi_j|  +  2^-25 2^-epsi s sum_j |W_j|
    with the exponents of ``scales`` below.  2^-23 |F_ref|: the roundings of the unscaled sum and of "+ mu0".  The cosine:
    t = p / 2 pi - rint(p / 2 pi) in float64, then cospif(float32(2 t)) in float32: the argument's rounding is <= 2^-25 half turns
    = pi 2^-25 in the angle, the float32 function is within 2 ulp <= 2^-23 (the device library's stated accuracy), together
    <= 2.13e-7 < COS_ERR = 2^-22; the float64 phase itself, D + 2 roundings of a magnitude |b| + sum_d |omega_d u_d|, adds
    (D + 2) 2^-52 times that magnitude.  The term is (COS_ERR + that) s sum_j |W_j|.

model
    A restatement of the header's "numerics" paragraph in numpy, with switches for seven wrong variants.  It is never the reference
    of a GPU test: tests/test_pathwise_reference_cpu.py uses it to show that a correct implementation stays within the bars on the
    data of every GPU case and that each wrong variant leaves them.
"""
from collections import namedtuple

import numpy as np

import chain_reference as CR

KINDS = ("se", "matern12", "matern32", "matern52", "rq")
COS_ERR = 2.0 ** -22
PSI_EXP_MAX, PSI_EXP_MIN = 14, 0
N = 257  # training points of the GPU cases (two full 128-point tiles and one point)


def kappa(kind, r, alpha=2.0):
    """The correlation of include/agpl_kernels.h at scaled distance r."""
    r = np.asarray(r, np.float64)
    if kind == "se":
        return np.exp(-0.5 * r * r)
    if kind == "matern12":
        return np.exp(-r)
    if kind == "matern32":
        return (1 + np.sqrt(3) * r) * np.exp(-np.sqrt(3) * r)
    if kind == "matern52":
        return (1 + np.sqrt(5) * r + 5 * r * r / 3) * np.exp(-np.sqrt(5) * r)
    if kind == "rq":
        return (1 + r * r / (2 * alpha)) ** -alpha
    raise ValueError(kind)


def spectral(kind, F, D, rng, alpha=2.0):
    """(omega [F, D], phase [F]): the spectral rule of include/agpl_pathwise.h in the scaled units."""
    n = rng.standard_normal((F, D))
    phase = rng.uniform(0.0, 2 * np.pi, F)
    twonu = {"matern12": 1, "matern32": 3, "matern52": 5}.get(kind)
    if twonu is not None:
        n = n * np.sqrt(twonu / rng.chisquare(twonu, F))[:, None]
    elif kind == "rq":
        n = n * np.sqrt(rng.gamma(alpha, 1.0 / alpha, F))[:, None]
    elif kind != "se":
        raise ValueError(kind)
    return n, phase


def kernel_matrix(kind, a, b, ell, s2, alpha=2.0):
    d = (a[:, None, :] - b[None, :, :]) / ell
    return s2 * kappa(kind, np.sqrt((d * d).sum(-1)), alpha)


def whitening(kind, z, ell, s2, jitter, alpha=2.0):
    """L^-1 with K_ZZ + jitter I = L L'."""
    Lc = np.linalg.cholesky(kernel_matrix(kind, z, z, ell, s2, alpha) + jitter * np.eye(len(z)))
    return np.linalg.solve(Lc, np.eye(len(z)))


def phi_f64(kind, x, z, ell, s2, Linv, alpha=2.0):
    """Phi [n, M] = (L^-1 K_ZX)'."""
    return (Linv @ kernel_matrix(kind, z, x, ell, s2, alpha)).T


def psi_f64(x, ell, omega, phase):
    """Psi [n, F]."""
    return np.cos((x / ell) @ omega.T + phase)


def coefficients(V, W, Xi, PsiZ, Linv, s, jitter):
    """c [T, L, M] = V - L^-1 (s Psi(Z)' W + sqrt(jitter) Xi);  PsiZ [M, F]."""
    up = s * np.einsum("af,tlf->tla", PsiZ, W)
    if Xi is not None:
        up = up + np.sqrt(jitter) * Xi
    return V - np.einsum("ab,tlb->tla", Linv, up)


def reference(Phi, Psi, c, W, s, mu0=None):
    """F [T, L, n] float64."""
    m0 = 0.0 if mu0 is None else np.asarray(mu0, np.float64)
    return m0 + np.einsum("na,tla->tln", Phi, c) + s * np.einsum("nf,tlf->tln", Psi, W)


def c_model(Phi, Psi, PsiZ, Linv, S, s, jitter):
    """[n, n]: the covariance of the draws of one latent, S = Cov(V)."""
    q = Linv.T @ Phi.T
    B = s * (Psi.T - PsiZ.T @ q)
    return B.T @ B + jitter * q.T @ q + Phi @ S @ Phi.T


def c_exact(Kxx, Phi, S):
    return Kxx - Phi @ Phi.T + Phi @ S @ Phi.T


def mc_bar(Cm, T, nsigma=5.0):
    """The element-wise Monte-Carlo bar of a sample covariance of T Gaussian draws with covariance Cm."""
    d = np.diag(Cm)
    return nsigma * np.sqrt((d[:, None] * d[None, :] + Cm * Cm) / T)


# ---- the device arithmetic --------------------------------------------------------------------------------------------------------

Scales = namedtuple("Scales", "E ec ew epsi")
FREE = 1000


def scales(max_c, max_sw, e_phi):
    """pw_scales of csrc/agpl_pathwise.hip: e_phi + ec = epsi + ew = E, ec and ew no larger than float16 allows, 0 <= epsi <= 14."""
    ecm = CR.scale_exp(max_c) if max_c > 0 else FREE
    ewm = CR.scale_exp(max_sw) if max_sw > 0 else FREE
    E = min(e_phi + ecm, PSI_EXP_MAX + ewm)
    if ecm == FREE and ewm == FREE:
        E = e_phi
    epsi = PSI_EXP_MIN if ewm == FREE else max(E - ewm, PSI_EXP_MIN)
    return Scales(E, E - e_phi, E - epsi, epsi)


def n_products(M, F):
    return 16 * ((M + 15) // 16) + 16 * ((F + 15) // 16)


Bars = namedtuple("Bars", "F rel abs cos")


def bars(Phi, Psi, c, W, s, ref, e_phi, phase_mag=0.0, D=1):
    """Element-wise bar on |F - F_ref| [T, L, n] (the module's docstring).  phase_mag: max |b| + sum_d |omega_d u_d|."""
    aPhi, aPsi = np.abs(Phi), np.abs(Psi)
    M, F = Phi.shape[1], Psi.shape[1]
    nk = n_products(M, F)
    sc = scales(np.abs(c).max(), s * np.abs(W).max(), e_phi)
    rel = (2.0 ** -21 + nk * 2.0 ** -24) * np.einsum("na,tla->tln", aPhi, np.abs(c)) \
        + (2.0 ** -20 + nk * 2.0 ** -24) * s * np.einsum("nf,tlf->tln", aPsi, np.abs(W))
    sW = s * np.abs(W).sum(-1)[:, :, None]
    ab = 2.0 ** -25 * (2.0 ** -sc.ec * aPhi.sum(1) + 2.0 ** -sc.ew * aPsi.sum(1))[None, None, :] + 2.0 ** -25 * 2.0 ** -sc.epsi * sW
    cs = (COS_ERR + (D + 2) * 2.0 ** -52 * phase_mag) * sW * np.ones(Phi.shape[0])
    return Bars(rel + ab + cs + 2.0 ** -23 * np.abs(ref), rel, ab, cs)


MUTATIONS = ("sin_for_cos", "phase_dropped", "omega_on_unscaled_x", "no_linv_on_up", "no_sqrt_2_over_F", "every_draw_reads_w0",
             "psi_without_lo_plane")


def _project(Ah, Al, Bh, Bl, acc, drop_b_lo=False):
    """acc [r, n] float32 += hi hi + hi lo + lo hi over slices of 16 features (A: rows, B: points)."""
    for k0 in range(0, Ah.shape[1], 16):
        k = slice(k0, k0 + 16)
        acc += Ah[:, k] @ Bh[:, k].T
        if not drop_b_lo:
            acc += Ah[:, k] @ Bl[:, k].T
        acc += Al[:, k] @ Bh[:, k].T
    return acc


def _pad16(n):
    return (n + 15) // 16 * 16


def model(image, x, z, ell, omega, phase, V, W, Xi, Linv, s2, jitter, mu0=None, mutate=None):
    """F [T, L, n] float32 as the header's set-up / features / numerics paragraphs state it; ``image`` = (hi, lo, e_phi) of
    chain_reference.model_features(Phi).  ``mutate``: one of MUTATIONS."""
    assert mutate is None or mutate in MUTATIONS
    Ph, Pl, e_phi = image
    T, L, M = V.shape
    F = omega.shape[0]
    f32 = np.float32
    s = np.sqrt(s2) * np.sqrt(2.0 / F)
    s_used = np.sqrt(s2) if mutate == "no_sqrt_2_over_F" else s
    b = np.zeros_like(phase) if mutate == "phase_dropped" else phase
    fn = np.sin if mutate == "sin_for_cos" else np.cos

    def period(u):
        p = np.repeat(b[None, :], u.shape[0], 0)
        for d in range(u.shape[1]):  # d ascending (the device's fused multiply-add rounds once; the difference is in the bar)
            p = p + u[:, d:d + 1] * omega[None, :, d]
        q = p * 0.15915494309189535
        return q - np.rint(q)

    PsiZ = fn(2 * np.pi * period(z / ell))  # [M, F] float64
    Weff = np.repeat(W[:1], T, 0) if mutate == "every_draw_reads_w0" else W
    up = s_used * np.einsum("af,tlf->tla", PsiZ, Weff)
    if Xi is not None:
        up = up + np.sqrt(jitter) * Xi
    c = (V - (up if mutate == "no_linv_on_up" else np.einsum("ab,tlb->tla", Linv, up))).reshape(T * L, M)
    Wr = Weff.reshape(T * L, F)
    sc = scales(np.abs(c).max(), s_used * np.abs(Wr).max(), e_phi)
    t = period(x if mutate == "omega_on_unscaled_x" else x / ell)
    psi = fn(np.pi * (2.0 * t).astype(f32).astype(np.float64)).astype(f32)  # cospif of the float32 argument, rounded to float32
    Sh, Sl = CR.split16(psi.astype(np.float64), sc.epsi, _pad16(F))
    Mk = _pad16(M)
    Ch, Cl = CR.split16(c, sc.ec, Mk)
    Wh, Wl = CR.split16(Wr * s_used, sc.ew, _pad16(F))
    acc = np.zeros((T * L, x.shape[0]), f32)
    acc = _project(Ch, Cl, Ph[:, :Mk], Pl[:, :Mk], acc)
    acc = _project(Wh, Wl, Sh, Sl, acc, drop_b_lo=mutate == "psi_without_lo_plane")
    out = (f32(2.0 ** -sc.E) * acc).reshape(T, L, -1)
    if mu0 is not None:
        out = out + np.asarray(mu0, f32)[None]
    return out.astype(f32)


# ---- the cases of tests/test_gpu_pathwise.py -----------------------------------------------------------------------------------------

Case = namedtuple("Case", "kind M F L T D jitter mu0 xi")
Case.id = property(lambda c: f"{c.kind}-M{c.M}-F{c.F}-L{c.L}-T{c.T}-D{c.D}-j{c.jitter:g}" + ("-mu0" if c.mu0 else "") + ("-xi" if c.xi else ""))

# M = 5, 64, 300; F = 16, 100 (padding), 1000; L = 1, 3; D = 1, 3, 16; the five kinds; T L = 1, 33, 128, 129; mu0 / Xi present and
# absent; jitter 1e-6 and 1e-3
CASES = [
    Case("se", 64, 100, 1, 1, 1, 1e-6, True, True),
    Case("matern12", 5, 16, 3, 11, 3, 1e-3, False, True),
    Case("matern32", 300, 1000, 1, 128, 3, 1e-6, True, False),
    Case("matern52", 64, 100, 3, 43, 16, 1e-3, True, True),
    Case("rq", 64, 1000, 1, 33, 3, 1e-6, False, True),
    Case("matern12", 300, 16, 3, 43, 1, 1e-3, True, False),
    Case("se", 5, 1000, 1, 129, 16, 1e-6, False, True),
]
ALPHA = 2.0
VARIANCE = 1.7
ELL = {1: 0.9, 3: 0.8, 16: 3.0}


def case_inputs(c):
    """x [N, D], z [M, D], ell [D]: D = 1: z on a grid over [-3, 3] with lengthscale 0.9 grid steps; else z uniform in the cube."""
    rng = np.random.default_rng([c.M, c.D, 7])
    x = rng.uniform(-3, 3, size=(N, c.D))
    if c.D == 1:
        z = np.linspace(-3, 3, c.M)[:, None]
        ell = np.array([ELL[1] * (6.0 / max(c.M - 1, 1))])
    else:
        z = rng.uniform(-3, 3, size=(c.M, c.D))
        ell = ELL[c.D] * (1.0 + 0.1 * np.arange(c.D))
    return x, z, ell


def case_draws(c):
    """(omega, phase, V, W, Xi or None, mu0 [L, N] float32 or None): V independent per (t, l), times 1 + l, around a mean of 0.5."""
    rng = np.random.default_rng([c.M, c.F, c.L, c.T, c.D, KINDS.index(c.kind)])
    omega, phase = spectral(c.kind, c.F, c.D, rng, ALPHA)
    V = 0.5 + rng.standard_normal((c.T, c.L, c.M)) * (1.0 + np.arange(c.L))[None, :, None]
    W = rng.standard_normal((c.T, c.L, c.F))
    Xi = rng.standard_normal((c.T, c.L, c.M)) if c.xi else None
    mu0 = (3.0 * (1.0 + np.arange(c.L))[:, None] + 0.5 * rng.standard_normal((c.L, N))).astype(np.float32) if c.mu0 else None
    return omega, phase, V, W, Xi, mu0


def case_reference(c, Phi, x, z, ell, draws, e_phi):
    """(F_ref, bars, coefficients) of a case from the features Phi the test holds exactly (the plan's own, or the model image's)."""
    omega, phase, V, W, Xi, mu0 = draws
    s = np.sqrt(VARIANCE) * np.sqrt(2.0 / c.F)
    Linv = whitening(c.kind, z / ell, 1.0, VARIANCE, c.jitter, ALPHA)
    cc = coefficients(V, W, Xi, psi_f64(z, ell, omega, phase), Linv, s, c.jitter)
    Psi = psi_f64(x, ell, omega, phase)
    ref = reference(Phi, Psi, cc, W, s, mu0)
    mag = np.abs(phase).max() + (np.abs(x / ell) @ np.abs(omega).T).max()
    return ref, bars(Phi, Psi, cc, W, s, ref, e_phi, mag, c.D), cc
