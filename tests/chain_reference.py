"""Float64 reference, element-wise error bars and a numpy model of prediction from a chain of inducing draws
(include/agpl_chain.h: agpl_plan_predict_chain), for tests/test_gpu_chain_predict.py, tests/test_gpu_chain_predict_shapes.py and
tests/test_chain_reference_cpu.py.  No GPU, no library code: nothing here imports the package.

reference
    vbar = (1/T) sum_t V[t] in float64, t ascending (the header's order; numpy's pairwise mean may differ in the last bit, which only a
    chain of identical draws can see);  F = mu0 + Phi V[t, l];  mean = mu0 + Phi vbar;  spread = mean_t (Phi (V[t, l] - vbar))^2.

bars (element-wise, from the arithmetic the header documents; Phi is the plan's own features, hi + lo of its image, so Phi's split
is exact and the whole error is V's)
    An entry x of an image is packed as x 2^e -> float32 -> float16 hi + float16 lo, 2^e max|x| in [2^13, 2^14).
    * relative part: float32 rounding 2^-24; lo = f16(xf - hi), |xf - hi| <= 2^-11 |x|, rounded with unit round-off 2^-11: 2^-22;
      the dropped lo lo product: 2^-11 . 2^-11 = 2^-22 (Phi's lo is <= 2^-11 |phi|).  Together 2^-21 + 2^-24, and float32
      accumulation over the Mp products of a row: EPS = 2^-21 + Mp 2^-24 times sum_a |Phi_na| |x_a|  (the existing bar).
    * absolute part (the shared scale): float16 is normal down to 2^-14 and has spacing 2^-24 below.  A residual xf - hi below 2^-14 is
      rounded to that grid: error <= 2^-25 instead of 2^-11 |lo|.  An entry below 2^-14 altogether has a subnormal hi (error <= 2^-25)
      and a residual <= 2^-25 that rounds to 0 or 2^-24: hi + lo is still within 2^-25 of xf.  So every packed entry is within
      2^-25 of its scaled value beyond the relative part, 2^-25 2^-e unscaled.  Without the clamp 2^-e <= 2^-13 max|x|, which gives
      the 2^-38 max|x| of DESIGN 4.11; with |e| clamped at 90 (max|x| < 2^-77) that would understate it, so the bar uses 2^-25 2^-e
      with e from the documented rule (equal to or below 2^-38 max|x| whenever the clamp is idle).  A projection sums Mp entries
      against phi: the term is 2^-25 2^-e sum_a |Phi_na|, once with ec (centred draws) and once with eb (vbar).
    * 2^-23 |F_ref|: the roundings of base = mu0 + phi' vbar and of F = base + q (what |base| exceeds |F| by is below |q|, which the
      relative part covers with room to spare).
    * spread: with B the bar of one centred projection q, |q'^2 - q^2| <= 2 |q| B + B^2, averaged over t, plus T float32 roundings
      of the running sum, T 2^-24 spread.

model
    A restatement of the header's "numerics" paragraph in numpy, with switches for six wrong variants.  It is never the reference of
    a GPU test: tests/test_chain_reference_cpu.py uses it to show that a correct implementation stays within the bars on the data of
    every GPU case and that each wrong variant leaves them.
"""
from collections import namedtuple

import numpy as np

N = 300
BS = 128  # rows of a block of the V image; the sums of squares run per half block of 64


def plan_padded(M):
    return (M + 255) // 256 * 256


def eps(Mp):
    return 2.0 ** -21 + Mp * 2.0 ** -24


def scale_exp(mx):
    """e with 2^e mx in [2^13, 2^14), clamped to +-90; 0 for mx = 0."""
    if not (mx > 0.0 and np.isfinite(mx)):
        return 0
    e = 13 - (int(np.frexp(mx)[1]) - 1)
    return max(-90, min(90, e))


def chain_mean(V):
    s = np.zeros(V.shape[1:], np.float64)
    for t in range(V.shape[0]):
        s = s + V[t]
    return s / float(V.shape[0])


Reference = namedtuple("Reference", "F mean spread q vbar cen")


def reference(Phi, V, mu0=None):
    """Phi [n, M], V [T, L, M] float64, mu0 [L, n] or None -> F [T, L, n], mean [L, n], spread [L, n] (and q, vbar, cen)."""
    Phi, V = np.asarray(Phi, np.float64), np.asarray(V, np.float64)
    vbar = chain_mean(V)
    cen = V - vbar
    m0 = 0.0 if mu0 is None else np.asarray(mu0, np.float64)
    q = np.einsum("na,tla->tln", Phi, cen)
    return Reference(m0 + np.einsum("na,tla->tln", Phi, V), m0 + np.einsum("na,la->ln", Phi, vbar), (q * q).mean(0), q, vbar, cen)


Bars = namedtuple("Bars", "F mean spread cen")


def bars(Phi, ref, Mp, absolute=True):
    """Element-wise bars on |F - F_ref|, |mean - mean_ref|, |spread - spread_ref| (and on one centred projection).  ``absolute``:
    with the shared-scale term (the module's docstring); without it these are the bars tests/test_gpu_chain_predict.py always had."""
    absPhi = np.abs(np.asarray(Phi, np.float64))
    E, T = eps(Mp), ref.cen.shape[0]
    b_mean = E * np.einsum("na,la->ln", absPhi, np.abs(ref.vbar))
    b_cen = E * np.einsum("na,tla->tln", absPhi, np.abs(ref.cen))
    if absolute:
        S = absPhi.sum(1)
        b_cen = b_cen + 2.0 ** -25 * 2.0 ** -scale_exp(np.abs(ref.cen).max()) * S
        b_mean = b_mean + 2.0 ** -25 * 2.0 ** -scale_exp(np.abs(ref.vbar).max()) * S
    bar_F = b_cen + 2.0 ** -23 * np.abs(ref.F) + b_mean
    bar_mean = b_cen.mean(0) + 2.0 ** -23 * np.abs(ref.mean) + b_mean
    bar_spread = (2 * np.abs(ref.q) * b_cen + b_cen * b_cen).mean(0) + T * 2.0 ** -24 * ref.spread
    return Bars(bar_F, bar_mean, bar_spread, b_cen)


# ---- the cases of tests/test_gpu_chain_predict_shapes.py (and the tight chain of tests/test_gpu_chain_predict.py) --------------------

Case = namedtuple("Case", "M L T kind arg")
Case.id = property(lambda c: f"M{c.M}-L{c.L}-T{c.T}-{c.kind}" + ("" if c.arg is None else f"{c.arg:+d}"))

SEAMS = [Case(64, L, T, "separated", None) for L, Ts in ((1, (32, 33, 64, 65, 128, 129, 256, 257)), (3, (11, 22, 43, 128)), (5, (13, 26)),
                                                          (10, (13,)), (33, (2,)), (64, (2, 3))) for T in Ts]
PADS = [Case(300, 3, 43, "separated", None), Case(512, 2, 65, "separated", None)]
SCALES = [Case(64, 2, 37, "small_latent", -10), Case(64, 2, 37, "small_latent", -20), Case(64, 1, 37, "burn_in", 12),
          Case(64, 1, 37, "burn_in", 20)]
POW2 = [Case(64, 2, 37, "pow2", k) for k in (0, 20, -20)]
DEGENERATE = [Case(64, 3, 4, "identical", None), Case(64, 3, 3, "identical", None), Case(64, 3, 5, "zero_mu0", None),
              Case(64, 3, 5, "zero", None)]
TIGHT = [Case(M, L, 37, "tight", None) for M in (64, 200) for L in (1, 2)]
NS_EDGES = Case(64, 3, 22, "separated", None)  # one of SEAMS
CASES = SEAMS + PADS + SCALES + POW2 + DEGENERATE + TIGHT
_KINDS = ("separated", "small_latent", "burn_in", "pow2", "identical", "zero_mu0", "zero", "tight")


GRIDS = {64: (8, 8), 200: (20, 10), 300: (20, 15), 512: (32, 16)}


def se_inputs(M):
    """x [N, 2] in the square, z on a grid over it, lengthscales of 0.9 grid steps."""
    rng = np.random.default_rng(100 + M)
    x = rng.uniform(-10, 10, size=(N, 2))
    n0, n1 = GRIDS[M]
    g0, g1 = np.linspace(-10, 10, n0), np.linspace(-10, 10, n1)
    z = np.stack(np.meshgrid(g0, g1, indexing="ij"), -1).reshape(M, 2)
    ell = 0.9 * np.array([g0[1] - g0[0], g1[1] - g1[0]])
    return x, z, ell


def separated(rng, T, L, M, n=N):
    """Data that tell latents and draws apart: V[t, l, :] independent per (t, l), times 1 + l;  mu0[l, :] = 10 (l + 1) + 0.5 N(0, 1)."""
    V = rng.standard_normal((T, L, M)) * (1.0 + np.arange(L))[None, :, None]
    mu0 = (10.0 * (1.0 + np.arange(L))[:, None] + 0.5 * rng.standard_normal((L, n))).astype(np.float32)
    return V, mu0


def tight(rng, T, L, M):
    """A chain at |v| about 3 that moves by 1e-3 (test_spread_of_a_tight_chain)."""
    v0 = 3.0 + 0.5 * rng.standard_normal((1, L, M))
    return v0 + 1e-3 * rng.standard_normal((T, L, M))


def case_data(c, n=N):
    """(V [T, L, M] float64, mu0 [L, n] float32 or None) of a case; the draws of a kind do not depend on its ``arg``."""
    rng = np.random.default_rng([c.M, c.L, c.T, _KINDS.index(c.kind)])
    V, mu0 = separated(rng, c.T, c.L, c.M, n)
    if c.kind == "small_latent":
        V[:, 1] *= 2.0 ** c.arg
    elif c.kind == "burn_in":
        V[0] *= 2.0 ** c.arg
    elif c.kind == "pow2":
        V, mu0 = V * 2.0 ** c.arg, None
    elif c.kind == "identical":
        V = np.repeat(V[:1], c.T, axis=0)
    elif c.kind == "zero_mu0":
        V = np.zeros_like(V)
    elif c.kind == "zero":
        V, mu0 = np.zeros_like(V), None
    elif c.kind == "tight":
        V, mu0 = tight(rng, c.T, c.L, c.M), None
    return V, mu0


# ---- the model ------------------------------------------------------------------------------------------------------------------------

MUTATIONS = ("second_half_latent_from_0", "base_of_next_latent", "no_lo_plane_of_V", "rows_32_up_of_last_group_skipped",
             "spread_as_difference_of_sums", "ssq_into_latent_0")


def split16(x, e, Mp):
    """x [r, M] float64 at scale 2^e as float16 hi + lo (held in float32), features padded with zeros to Mp."""
    xf = np.zeros((x.shape[0], Mp), np.float32)
    xf[:, : x.shape[1]] = (x * 2.0 ** e).astype(np.float32)
    hi = xf.astype(np.float16)
    lo = (xf - hi.astype(np.float32)).astype(np.float16)
    return hi.astype(np.float32), lo.astype(np.float32)


def model_features(Phi):
    """The image of Phi (one power-of-two scale, float16 hi + lo) and the features it holds exactly, hi + lo unscaled."""
    Phi = np.asarray(Phi, np.float64)
    e = scale_exp(np.abs(Phi).max())
    hi, lo = split16(Phi, e, plan_padded(Phi.shape[1]))
    exact = ((hi.astype(np.float64) + lo) * 2.0 ** -e)[:, : Phi.shape[1]]
    return (hi, lo, e), exact


def _project(Ah, Al, Bh, Bl, drop_lo=False):
    """[r, n] float32: hi hi + hi lo + lo hi, accumulated in float32 over slices of 16 features."""
    acc = np.zeros((Ah.shape[0], Bh.shape[0]), np.float32)
    for s in range(0, Ah.shape[1], 16):
        k = slice(s, s + 16)
        acc += Ah[:, k] @ Bh[:, k].T
        acc += Ah[:, k] @ Bl[:, k].T
        if not drop_lo:
            acc += Al[:, k] @ Bh[:, k].T
    return acc


def _skip_rows_32_up(acc, live):
    """Wrong variant (d): in every block of 128 rows, rows >= 32 of the last 64-row group that holds a live row give nothing."""
    for b0 in range(0, live, BS):
        rows = min(live - b0, BS)
        g = b0 + (rows - 1) // 64 * 64
        acc[g + 32: g + 64] = 0.0
    return acc


def model(image, V, mu0=None, mutate=None):
    """(F [T, L, n], mean [L, n], spread [L, n]) float32 as the header's numerics paragraph states them; ``image`` from model_features.
    ``mutate``: one of MUTATIONS."""
    assert mutate is None or mutate in MUTATIONS
    (Ph, Pl, e_phi) = image
    V = np.asarray(V, np.float64)
    T, L, M = V.shape
    Mp, n, TL = Ph.shape[1], Ph.shape[0], T * L
    f32 = np.float32
    vbar = chain_mean(V)
    cen = (V - vbar).reshape(TL, M)
    eb, ec = scale_exp(np.abs(vbar).max()), scale_exp(np.abs(cen).max() if cen.size else 0.0)
    drop = mutate == "no_lo_plane_of_V"
    acc_b = _project(*split16(vbar, eb, Mp), Ph, Pl, drop)
    acc_c = _project(*split16(cen, ec, Mp), Ph, Pl, drop)
    if mutate == "rows_32_up_of_last_group_skipped":
        acc_b, acc_c = _skip_rows_32_up(acc_b, L), _skip_rows_32_up(acc_c, TL)
    base = f32(2.0 ** -(e_phi + eb)) * acc_b
    if mu0 is not None:
        base = base + np.asarray(mu0, f32)
    q = f32(2.0 ** -(e_phi + ec)) * acc_c
    F = np.empty((TL, n), f32)
    ssq = np.zeros((2, L, n), f32)
    for g in range(TL):
        hh, l = g % BS // 64, g % L
        if mutate == "second_half_latent_from_0" and hh == 1:
            l = g % 64 % L
        d = 0 if mutate == "ssq_into_latent_0" else l
        ssq[hh, d] = (q[g].astype(np.float64) * q[g] + ssq[hh, d]).astype(f32)  # fused multiply-add
        F[g] = base[(l + 1) % L if mutate == "base_of_next_latent" else l] + q[g]
    F = F.reshape(T, L, n)
    spread = (ssq[0] + ssq[1]) / f32(T)
    if mutate == "spread_as_difference_of_sums":
        s2 = np.zeros((L, n), f32)
        for t in range(T):
            s2 = s2 + F[t] * F[t]
        spread = s2 / f32(T) - base * base
    return F, base.astype(f32), spread.astype(f32)
