"""Float64 references, element-wise bars and numpy models of the two split-float16 contractions of a sweep, for
tests/test_gpu_split_planes.py and tests/test_split_reference_cpu.py.  No GPU, no library code: nothing here imports the package.

    accumulation (agpl_syrk.hip, syrk_strip_kernel):     G = Phi' Diag(gamma) Phi,  g = Phi' beta
    marginal pass (agpl_split.hip, marginal_factor_queue_kernel):  T = U Phi',  q_n = sum_a T_an^2,  m_n = sum_a v_a T_an

Both run a float32 product as hi hi + hi lo + lo hi of float16 planes (lo lo dropped).  With random-sign data a lost cross term
averages away below the suites' max-norm bars; the data here keep the sum behind every checked output SHORT and SAME-SIGNED and put
its few terms at the seams of a long launch, everything else exactly zero.

operands, as coded (one statement: chain_reference.scale_exp / split16 / model_features, which this module calls)
    Phi images (both kernels): one exponent e from max|Phi|, 2^e max|Phi| in [2^13, 2^14); xs = fl32(2^e phi) (exact);
    hi = f16(xs), lo = f16(xs - hi).  The library clamps |e| at 30 (chain_reference at 90): every case here has |e| <= 30, asserted.
    B of the accumulation: x = hi + lo (exact in float32), y = fl32((2^e_B gamma_n) x), 2^e_B max(gamma) in [1/2, 1), re-split as
    above.  (The kernel forms hi and lo of y with one rounding of the exact product each -- v_fma_mix -- which differs from the
    re-split of fl32(y) by at most the 2^-24 the bar carries for that rounding.)
    U images: fl32(2^15 U) split as above; v as the float32 the plan exports.

bars (u = 2^-24; every term multiplies sum |terms| OF THAT ELEMENT, never M u or N u times a norm)
    one split: |x - hi - lo| <= 2^-22 |x| (lo = f16(x - hi), |x - hi| <= 2^-11 |x|, unit round-off 2^-11), and 2^-25 absolute in
    scaled units where lo falls below the float16 normals.  The dropped lo lo: 2^-11 . 2^-11 = 2^-22 of the term.
    One MFMA (depth D = 32 products and the accumulator, in an order the hardware does not document): at most D roundings of at
    most the magnitude it ends with, D u (|C| + sum |products|).  A product with a zero factor, and an accumulator that is added
    zeros only, round nothing.
  accumulation, element (a, b) with S = sum_n |phi_na gamma_n phi_nb| (<= 4 terms, one step, one slice):
    A split 2^-22 + B split 2^-22 + lo lo 2^-22 + fl32(gamma x) u + three MFMAs 3 . 32 u + the slab store u (a power-of-two scaling:
    exact unless it underflows) = (3 . 2^-22 + 98 u) S, plus 2^-25 (|a_s| + |b_s|) summed over the terms, unscaled.  The slabs are
    added in float64 and all but one of them are exactly zero.
    g_a with S = sum_n |beta_n phi_na|: the image holds phi to 2^-22; <= 4 v_fmac + 2 lane additions + the slab store: (2^-22 + 7 u) S,
    plus 2^-25 sum |beta_n| unscaled.
  marginal pass, row a and point n, P_k = sum over the 32 features b of stage k of |U_ab phi_nb|:
    E_T = 3 . 2^-22 sum_k P_k + 96 u sum_{k live} (P_0 + ... + P_k) + 2^-25 sum_b (|U_s| + |phi_s|) unscaled
    (stage k is live for (a, n) when it multiplies at all -- k <= a / 32 -- and point n has a non-zero feature in it: the three MFMAs
    of a live stage end with at most the running sum; a stage of zeros rounds nothing).  Then, as the code orders them: the 8-term
    FMA chain of a lane (8), the two chains (1), the permlane tree over the four k-groups (2), the four row groups (2), the row
    blocks in ascending order (nb2), the residual or prior mean (1):
    bar_var = sum_a (2 |T| E_T + E_T^2) + (14 + nb2) u q + u |var|,   bar_mu = sum_a |v_a| E_T + (14 + nb2) u sum_a |v_a T_an| + u |mu|,
    c = sqrt(mu^2 + var) (Bernoulli): |c'^2 - c^2| / c + 4 u c  (mu^2, the addition, a square root good to one ulp).

models
    Restatements of the kernels' arithmetic with switches for named wrong variants, each restricted to one seam position / stage.
    Never the reference of a GPU test: tests/test_split_reference_cpu.py shows that the model stays within the bars on every GPU
    case and that each variant leaves them."""
import os
import re
from collections import namedtuple

import numpy as np

import chain_reference as R
import seam_shapes as S

U = 2.0 ** -24
f32, f64 = np.float32, np.float64

# ---- the seam constants, read from the sources --------------------------------------------------------------------------------------------

_SYRK, _SLICES, _SPLIT = "agpl_syrk.hip", "agpl_slices.h", "agpl_split.hip"


def _src(name):
    return open(os.path.join(S.CSRC, name)).read()


def _find(pattern, file):
    m = re.search(pattern, _src(file), flags=re.M)
    if not m:
        raise LookupError(f"{pattern!r} is not stated in {file}")
    return tuple(int(x) for x in m.groups())


def constants():
    """What decides where a launch is cut, as the sources state it today (LookupError when a statement is gone)."""
    c = {}
    c["kStagePts"], = _find(r"^constexpr int kStagePts = (\d+);", _SYRK)
    c["kRing"], = _find(r"^constexpr int kRing = (\d+);", _SYRK)
    c["kPanel"], = _find(r"^constexpr int kPanel = (\d+);", _SYRK)
    c["chunk_M"], c["chunk_small_M"], c["chunk_large_M"] = _find(r"agpl_chunk_points\(int M\) \{ return M <= (\d+) \? (\d+) : (\d+); \}", _SLICES)
    c["chunk_cap"], = _find(r"while \(chunk < (\d+) &&", _SLICES)
    c["min_wg"], = _find(r"^#define AGPL_SLICE_MIN_WG (\d+)", _SLICES)
    c["tail_div"], = _find(r"^#define AGPL_SLICE_TAIL_DIV (\d+)", _SLICES)
    c["round_wg"], = _find(r"int64_t tail = \((\d+) \+ wg_per_slice - 1\) / wg_per_slice;", _SLICES)
    c["KS"], = _find(r"^constexpr int KS = (\d+);", _SPLIT)
    c["KU"], = _find(r"constexpr int R = 2, KU = (\d+);", _SPLIT)
    c["NT2"], = _find(r"^constexpr int NT2 = (\d+);", _SPLIT)
    return c


# what the shapes below were chosen for (tests/test_split_reference_cpu.py holds the sources to it)
STEP, RING, PANEL, STAGE, TILE = 32, 4, 256, 32, 256
EXPECTED = {"kStagePts": 32, "kRing": 4, "kPanel": 256, "chunk_M": 256, "chunk_small_M": 8192, "chunk_large_M": 4096, "chunk_cap": 16384,
            "min_wg": 32, "tail_div": 4, "round_wg": 256, "KS": 16, "KU": 2, "NT2": 256}


def slice_plan(N, M, L):
    """agpl_slice_plan (agpl_slices.h) restated with today's constants: [(nbeg, nend)] of the slices, and the number of big ones."""
    Mp = R.plan_padded(M)
    chunk = 8192 if Mp <= 256 else 4096
    nb2 = Mp // 256
    pairs = nb2 * (nb2 + 1) // 2
    while chunk < 16384 and L * pairs * S.cdiv(N, 2 * chunk) >= 32 * 256:
        chunk *= 2
    small = chunk // 4
    nfull, wg = S.cdiv(N, chunk), L * pairs
    tail = S.cdiv(256, wg)
    if Mp < 512 and nfull * wg > 512:
        tail = 0
    nbig = max(nfull - tail, 0)
    rest = N - nbig * chunk
    ns = nbig + (S.cdiv(rest, small) if rest > 0 else 0)
    out = []
    for s in range(ns):
        b = s * chunk if s < nbig else nbig * chunk + (s - nbig) * small
        out.append((b, min(b + (chunk if s < nbig else small), N)))
    return out, nbig


# ---- small helpers ------------------------------------------------------------------------------------------------------------------------

def same_signed_lo(h, frac=0.9):
    """h (float64, on a float16 grid) -> float32 h (1 + frac 2^-12): hi is h again and lo about frac 2^-12 h, the sign of h; at
    frac = 0.9 near the largest a lo part can be (half a float16 ulp is between 2^-12 and 2^-11 of h)."""
    return (np.asarray(h, f64) * (1.0 + frac * 2.0 ** -12)).astype(f32)


def grid16(x, e):
    """x rounded to the float16 grid at scale 2^e."""
    return (np.asarray(x, f64) * 2.0 ** e).astype(np.float16).astype(f64) * 2.0 ** -e


def trunc16(x):
    """float32 -> float16 towards zero (held in float32): the wrong split 'truncate and keep no lo part'."""
    h = x.astype(np.float16)
    over = np.abs(h.astype(f32)) > np.abs(x)
    h[over] = np.nextafter(h[over], np.float16(0))
    return h.astype(f32)


def resplit(y):
    """float32 y -> float16 hi, lo (held in float32)."""
    hi = y.astype(np.float16).astype(f32)
    return hi, (y - hi).astype(np.float16).astype(f32)


def gamma_scale_exp(gmax):
    """e_B (acc_scale_exp): 2^e_B max(gamma) in [1/2, 1), clamped to +-60."""
    if not gmax > 0:
        return 0
    bits = int(np.array(gmax, f32).view(np.uint32))
    return max(-60, min(60, 126 - (bits >> 23)))


def image_exp(Phi):
    e = R.scale_exp(float(np.abs(Phi).max()))
    assert abs(e) <= 30  # the library's clamp (agpl_image_scale_exp) is idle
    return e


# ---- accumulation: point-banded features ---------------------------------------------------------------------------------------------------

AccCase = namedtuple("AccCase", "N M L")
AccCase.id = property(lambda c: f"N{c.N}-M{c.M}-L{c.L}")
ACC_CASES = [AccCase(33, 512, 1), AccCase(4097, 512, 1), AccCase(9011, 1024, 1), AccCase(9011, 768, 2), AccCase(352257, 512, 1),
             AccCase(5003, 300, 1)]


def seam_positions(N, M, L):
    """[(name, first point of the 32-point step)]: the steps of a launch at which something changes hands.  Steps are counted inside
    their slice (the ring and the prologue start over with every slice)."""
    sl, nbig = slice_plan(N, M, L)
    b0, e0 = sl[0]
    steps0 = S.cdiv(e0 - b0, STEP)
    pos = [("first step", b0)]
    for t in range(1, RING):
        if t < steps0:
            pos.append((f"ring slot {t}", b0 + t * STEP))
    if RING < steps0:
        pos.append(("ring wrapped", b0 + RING * STEP))
    if steps0 > RING + 1:
        pos.append(("last step of slice 0", b0 + (steps0 - 1) * STEP))
    if len(sl) > 1:
        pos.append(("first step of slice 1", sl[1][0]))
    if N >= 2 * STEP:
        pos.append(("last full step", (N // STEP - 1) * STEP))
    if N % STEP:
        pos.append(("ragged last step", N // STEP * STEP))
    if nbig > 0 and steps0 > 2 * RING + 2:
        pos.append(("inside a big slice", b0 + (steps0 // 2 + 1) * STEP))
    if len(sl) > nbig + 2:  # a fine slice that is neither the first nor the ragged last one
        s = nbig + (len(sl) - nbig) // 2
        pos.append(("inside a fine slice", sl[s][0] + (S.cdiv(sl[s][1] - sl[s][0], STEP) // 2) * STEP))
    seen, out = set(), []
    for name, p in pos:
        if p not in seen and p < N:
            seen.add(p)
            out.append((name, p))
    assert len(out) <= 16
    return out


AccData = namedtuple("AccData", "case positions bands Phi_nz pts band_of resid y e")


def acc_data(case):
    """Band j (position j) holds <= 4 consecutive points of its step; feature a is non-zero only on band a mod T, one sign per feature,
    magnitudes in [2^-4, 1] max|Phi| with same-signed lo parts.  resid in [0.5, 4]: var > 0 everywhere and gamma differs from point
    to point (a stale gamma shows).  Phi_nz: the rows of the non-zero points ``pts``; every other row of Phi is zero."""
    N, M, L = case
    rng = np.random.default_rng([N, M, L, 1])
    positions = seam_positions(N, M, L)
    T = len(positions)
    bands, rows, band_of = [], [], []
    sign = rng.choice([-1.0, 1.0], size=M)
    for j, (_, p0) in enumerate(positions):
        end = min(p0 + STEP, N)
        off = min((7 * j + 3) % 29, max(end - p0 - 4, 0))  # bands start in different k-groups of their step, and straddle them
        pts = np.arange(p0 + off, min(p0 + off + 4, end))
        feats = np.arange(j, M, T)
        mag = 2.0 ** rng.uniform(-4.0, -0.001, size=(pts.size, feats.size)) * 0.999
        row = np.zeros((pts.size, M), f32)
        row[:, feats] = same_signed_lo(grid16(mag, 14) * sign[feats])
        bands.append((pts, feats))
        rows.append(row)
        band_of += [j] * pts.size
    Phi_nz = np.concatenate(rows)
    Phi_nz[0, 0] = same_signed_lo(grid16(0.999 * sign[0], 14))  # max|Phi| in [1/2, 1): e = 14 in every case
    pts = np.concatenate([b[0] for b in bands])
    resid = rng.uniform(0.5, 4.0, size=N).astype(f32)
    if L == 1:
        y = (rng.uniform(size=N) < 0.5).astype(np.uint8)
    else:
        y = (rng.integers(0, L + 1, size=N)[:, None] == np.arange(L)[None, :]).astype(np.uint8)
    return AccData(case, positions, bands, Phi_nz, pts, np.array(band_of), resid, y, image_exp(Phi_nz))


def acc_dense(d):
    Phi = np.zeros((d.case.N, d.case.M), f32)
    Phi[d.pts] = d.Phi_nz
    return Phi


def standin_gamma_beta(d):
    """gamma, beta [L, N] float32 for the CPU test (the GPU tests use what the pass exports): the Bernoulli rule at q(v) = N(0, I),
    var = resid + |phi|^2, c = sqrt(var), gamma = tanh(c / 2) / (2 c) -- for latent l at c (1 + l) -- and beta = +-1/2."""
    N, M, L = d.case
    var = d.resid.astype(f64)
    var[d.pts] += (d.Phi_nz.astype(f64) ** 2).sum(1)
    c = np.sqrt(var)[None, :] * (1.0 + np.arange(L))[:, None]
    yy = d.y.astype(f64) if L == 1 else d.y.T.astype(f64)
    return (np.tanh(c / 2) / (2 * c)).astype(f32), (yy.reshape(L, N) - 0.5).astype(f32)


def _band_rows(d, j):
    return np.nonzero(d.band_of == j)[0]


def acc_reference(d, gamma, beta):
    """G [L, M, M], g [L, M] in float64 from the float32 features and the given gamma, beta (zero rows add nothing)."""
    N, M, L = d.case
    G, g = np.zeros((L, M, M)), np.zeros((L, M))
    for j, (pts, feats) in enumerate(d.bands):
        P = d.Phi_nz[_band_rows(d, j)][:, feats].astype(f64)
        for l in range(L):
            G[l][np.ix_(feats, feats)] = (P * gamma[l, pts].astype(f64)[:, None]).T @ P
            g[l, feats] = P.T @ beta[l, pts].astype(f64)
    return G, g


def acc_bars(d, gamma, beta):
    N, M, L = d.case
    bG, bg = np.zeros((L, M, M)), np.zeros((L, M))
    eB = gamma_scale_exp(float(gamma.max()))
    for j, (pts, feats) in enumerate(d.bands):
        P = np.abs(d.Phi_nz[_band_rows(d, j)][:, feats].astype(f64))
        for l in range(L):
            gm = gamma[l, pts].astype(f64)[:, None]
            Sab = (P * gm).T @ P
            a_s, b_s = P * 2.0 ** d.e, P * gm * 2.0 ** (d.e + eB)
            absolute = 2.0 ** -25 * (a_s.sum(0)[:, None] + b_s.sum(0)[None, :]) * 2.0 ** -(2 * d.e + eB)
            bG[l][np.ix_(feats, feats)] = (3 * 2.0 ** -22 + 98 * U) * Sab + np.maximum(absolute, absolute.T)
            ab = np.abs(beta[l, pts].astype(f64))
            bg[l, feats] = (2.0 ** -22 + 7 * U) * (P.T @ ab) + 2.0 ** -25 * ab.sum() * 2.0 ** -d.e
    return bG, bg


ACC_VARIANTS = ("A_lo_dropped", "B_lo_dropped", "lo_hi_from_wrong_operand", "truncated_hi_no_lo", "stale_gamma")


def _mfma_acc(A, B, acc):
    """acc + sum_k A[k, :, None] B[k, None, :]: float16 products are exact in float32; the depth is summed in order, in float32."""
    s = np.zeros_like(acc)
    for k in range(A.shape[0]):
        s = (s + A[k][:, None] * B[k][None, :]).astype(f32)
    return (acc + s).astype(f32)


def _acc_operands(d, j, gamma_l, eB, mutate):
    pts, feats = d.bands[j]
    x = d.Phi_nz[_band_rows(d, j)][:, feats]
    hi, lo = R.split16(x, d.e, feats.size)
    gp = pts
    if mutate == "stale_gamma":
        gp = pts - STEP
    gs = (gamma_l[gp].astype(f64) * 2.0 ** eB).astype(f32)
    xx = (hi + lo).astype(f32)  # exact
    y = (xx * gs[:, None]).astype(f32)
    bh, bl = resplit(y)
    if mutate == "truncated_hi_no_lo":
        hi, lo = trunc16((x.astype(f64) * 2.0 ** d.e).astype(f32)), np.zeros_like(lo)
        bh, bl = trunc16(y), np.zeros_like(bl)
    return hi, lo, bh, bl, xx


def acc_can_touch(d, variant, j):
    """A stale gamma needs a previous step in the same slice."""
    if variant != "stale_gamma":
        return True
    p0 = d.positions[j][1]
    return all(b != p0 for b, _ in slice_plan(*d.case)[0])


def acc_model(d, gamma, beta, mutate=None, where=None):
    """G, g as syrk_strip_kernel forms them; ``mutate`` (one of ACC_VARIANTS) applies at seam position ``where`` only."""
    assert mutate is None or mutate in ACC_VARIANTS
    N, M, L = d.case
    G, g = np.zeros((L, M, M)), np.zeros((L, M))
    eB = gamma_scale_exp(float(gamma.max()))
    for j, (pts, feats) in enumerate(d.bands):
        mu = mutate if j == where else None
        for l in range(L):
            ah, al, bh, bl, xx = _acc_operands(d, j, gamma[l], eB, mu)
            acc = _mfma_acc(ah, bh, np.zeros((feats.size, feats.size), f32))
            if mu != "B_lo_dropped":
                acc = _mfma_acc(ah, bl, acc)
            if mu == "lo_hi_from_wrong_operand":
                acc = _mfma_acc(ah, bl, acc)
            elif mu != "A_lo_dropped":
                acc = _mfma_acc(al, bh, acc)
            G[l][np.ix_(feats, feats)] = acc.astype(f64) * 2.0 ** -(2 * d.e + eB)
            part = np.zeros((4, feats.size), f32)  # the lane partial sums of the four k-groups of the step
            for k, n in enumerate(pts):
                kg = (n % STEP) // 8
                part[kg] = (part[kg].astype(f64) + f64(beta[l, n]) * xx[k].astype(f64)).astype(f32)
            tot = ((part[0] + part[1]).astype(f32) + (part[2] + part[3]).astype(f32)).astype(f32)
            g[l, feats] = tot.astype(f64) * 2.0 ** -d.e
    return G, g


def acc_cross_terms(d, gamma):
    """Per latent and seam position: the float64 size of the two cross terms (hi lo', lo hi') of every element of the band."""
    N, M, L = d.case
    eB = gamma_scale_exp(float(gamma.max()))
    out = []
    for l in range(L):
        row = []
        for j, (pts, feats) in enumerate(d.bands):
            ah, al, bh, bl, _ = _acc_operands(d, j, gamma[l], eB, None)
            s = 2.0 ** -(2 * d.e + eB)
            row.append((np.abs(ah.astype(f64).T @ bl.astype(f64)) * s, np.abs(al.astype(f64).T @ bh.astype(f64)) * s))
        out.append(row)
    return out


def acc_visibility(d, gamma, bG):
    """min over latents, seam positions and the two cross terms of max over the band's elements of |cross term| / bar."""
    worst = np.inf
    for l, row in enumerate(acc_cross_terms(d, gamma)):
        for j, (hl, lh) in enumerate(row):
            feats = d.bands[j][1]
            bar = bG[l][np.ix_(feats, feats)]
            worst = min(worst, float((hl / bar).max()), float((lh / bar).max()))
    return worst


def ratio(got, ref, bar):
    """max |got - ref| / bar; where the bar is zero the value must be exactly zero (inf otherwise)."""
    err = np.abs(np.asarray(got, f64) - ref)
    z = bar == 0
    if np.any(err[z] != 0):
        return np.inf
    return float((err[~z] / bar[~z]).max()) if np.any(~z) else 0.0


# ---- marginal pass: stage-banded features, same-signed U -----------------------------------------------------------------------------------

MargCase = namedtuple("MargCase", "N M L kind")
MargCase.id = property(lambda c: f"N{c.N}-M{c.M}-L{c.L}-{c.kind}")
MARG_CASES = [MargCase(257, 256, 1, "banded"), MargCase(2049, 512, 2, "banded"), MargCase(2049, 1024, 1, "banded"),
              MargCase(700, 300, 1, "banded"), MargCase(2049, 512, 1, "dense")]

MargData = namedtuple("MargData", "case Phi stage_of U_int v_int G g resid y e")


def marg_stage_of(N, M):
    """s(n): every live stage (one with a feature below M) inside every 256-point tile, the ragged tile included."""
    return (np.arange(N) % TILE) % S.cdiv(M, STAGE)


def marg_data(case):
    """Positive features, lo parts 0.45 2^-12 of them, on the 32 features of stage s(n) only (``dense``: on all of them); U_int lower triangular, positive, entries
    h (1 + 0.9 2^-12) with h on the float16 grid of 2^15 U, the off-diagonal sized so that every 256-row block carries a like share
    of q; v_int positive.  G = (U_int' U_int)^-1 - I, g = U_int^-1 v_int: the update then leaves U = U_int, v = v_int."""
    N, M, L, kind = case
    rng = np.random.default_rng([N, M, L, 2, kind == "dense"])
    stage_of = marg_stage_of(N, M)
    mag = grid16(2.0 ** rng.uniform(-4.0, -0.001, size=(N, M)) * 0.999, 14)
    mag[0, 0] = grid16(0.999, 14)
    if kind == "banded":
        mag *= (np.arange(M)[None, :] // STAGE == stage_of[:, None])
    Phi = same_signed_lo(mag, 0.45)  # (half of U's: the two cross terms differ, so that swapping them shows)
    U_int, v_int = np.zeros((L, M, M)), np.zeros((L, M))
    G, g = np.zeros((L, M, M)), np.zeros((L, M))
    for l in range(L):
        dg = rng.uniform(0.05, 0.1, size=M) / (1.0 + l)
        off = 0.011 * 0.075 / (1.0 + l) * 2.0 ** rng.uniform(-4.0, 0.0, size=(M, M))
        Ul = np.tril(off, -1) + np.diag(dg)
        Ul = np.tril(same_signed_lo(grid16(Ul, 15)).astype(f64))
        U_int[l], v_int[l] = Ul, rng.uniform(0.5, 1.0, size=M)
        G[l] = np.linalg.inv(Ul.T @ Ul) - np.eye(M)
        G[l] = (G[l] + G[l].T) / 2
        g[l] = np.linalg.solve(Ul, v_int[l])
    resid = rng.uniform(1e-4, 2e-4, size=N).astype(f32)  # var > 0, and small beside q: the sums are what var shows
    y = (rng.uniform(size=N) < 0.5).astype(np.uint8) if L == 1 else \
        (rng.integers(0, L + 1, size=N)[:, None] == np.arange(L)[None, :]).astype(np.uint8)
    return MargData(case, Phi, stage_of, U_int, v_int, G, g, resid, y, image_exp(Phi))


def _pad_U(Ul, Mp):
    out = np.eye(Mp)
    out[: Ul.shape[0], : Ul.shape[0]] = np.tril(Ul)
    return out


MargRef = namedtuple("MargRef", "mu var c")


def marg_reference(d, Uv, v32):
    """mu, var [L, N] and c = sqrt(mu^2 + var) in float64 from the float32 features, the given U [L, M, M] (float64) and v [L, M]."""
    P = d.Phi.astype(f64)
    mu, var = [], []
    for l in range(d.case.L):
        T = np.tril(Uv[l]) @ P.T
        var.append(d.resid.astype(f64) + (T * T).sum(0))
        mu.append(v32[l].astype(f64) @ T)
    mu, var = np.array(mu), np.array(var)
    return MargRef(mu, var, np.sqrt(mu * mu + var))


def marg_bars(d, Uv, v32, ref):
    N, M, L, _ = d.case
    Mp = R.plan_padded(M)
    nb2, nst = Mp // 256, S.cdiv(M, STAGE)
    aP = np.abs(d.Phi.astype(f64))
    live = np.stack([(aP[:, STAGE * k: STAGE * (k + 1)] != 0).any(1) for k in range(nst)])  # [stage, n]
    bmu, bvar = np.zeros((L, N)), np.zeros((L, N))
    for l in range(L):
        aU = np.abs(np.tril(Uv[l]))
        T = np.tril(Uv[l]) @ d.Phi.astype(f64).T
        cum, W = np.zeros((M, N)), np.zeros((M, N))
        for k in range(nst):
            cols = slice(STAGE * k, min(STAGE * (k + 1), M))
            cum += aU[:, cols] @ aP[:, cols].T
            rows = (np.arange(M) // STAGE >= k)[:, None]  # the stages a row runs through (its zero blocks are skipped)
            W += cum * (rows & live[k][None, :])
        absolute = 2.0 ** -25 * 2.0 ** -(d.e + 15) * ((aU * 2.0 ** 15) @ (aP != 0).astype(f64).T + (aU != 0).astype(f64) @ (aP * 2.0 ** d.e).T)
        ET = 3 * 2.0 ** -22 * cum + 96 * U * W + absolute
        q = (T * T).sum(0)
        av = np.abs(v32[l].astype(f64))[:, None]
        bvar[l] = (2 * np.abs(T) * ET + ET * ET).sum(0) + (14 + nb2) * U * q + U * np.abs(ref.var[l])
        bmu[l] = (av * ET).sum(0) + (14 + nb2) * U * (av * np.abs(T)).sum(0) + U * np.abs(ref.mu[l])
    c2 = 2 * np.abs(ref.mu) * bmu + bmu * bmu + bvar
    return MargRef(bmu, bvar, c2 / ref.c + 4 * U * ref.c)


ALL = "all"  # ``where`` of marg_model: every stage (the dense case, where one stage is a sixteenth of a sum)
MARG_VARIANTS = ("U_lo_dropped", "Phi_lo_dropped", "lo_hi_from_wrong_operand", "truncated_hi_no_lo", "stage_planes_dropped")


def _row_sums(X, w):
    """sum over the rows a of w_a X_an as item_sums_rows and the item's end order them.  X [Mp, n] float32, w [Mp] float32 or None
    (X itself: the squares).  Row a = 256 rb + 64 wr + 16 i + 4 kg + r; a lane's two chains take r = (0, 2) and (1, 3) of i = 0..3."""
    Mp, n = X.shape
    X6 = X.reshape(Mp // 256, 4, 4, 4, 4, n).astype(f64)  # [rb, wr, i, kg, r, n]
    W6 = X6 if w is None else np.broadcast_to(w.astype(f64).reshape(Mp // 256, 4, 4, 4, 4, 1), X6.shape)
    chains = []
    for c in (0, 1):
        acc = np.zeros((Mp // 256, 4, 4, n), f32)  # [rb, wr, kg, n]
        for i in range(4):
            for r in (c, c + 2):
                acc = (W6[:, :, i, :, r] * X6[:, :, i, :, r] + acc.astype(f64)).astype(f32)  # fused multiply-add
        chains.append(acc)
    lane = (chains[0] + chains[1]).astype(f32)
    kg = ((lane[:, :, 0] + lane[:, :, 1]).astype(f32) + (lane[:, :, 2] + lane[:, :, 3]).astype(f32)).astype(f32)  # [rb, wr, n]
    return ((kg[:, 0] + kg[:, 1]).astype(f32) + (kg[:, 2] + kg[:, 3]).astype(f32)).astype(f32)  # [rb, n]


def marg_operands(d, Ul):
    """(Uh, Ul) [Mp, Mp] and (Ph, Pl) [N, Mp], float16 values held in float32."""
    Mp = R.plan_padded(d.case.M)
    (Ph, Pl, e), _ = R.model_features(d.Phi)
    assert e == d.e
    Uh, Ulo = R.split16(_pad_U(Ul, Mp), 15, Mp)
    return Uh, Ulo, Ph, Pl


def marg_model(d, Uv, v32, mutate=None, where=None):
    """mu, var [L, N] float32 and c as marginal_factor_queue_kernel and the per-point kernel behind it form them; ``mutate`` (one of
    MARG_VARIANTS) applies in stage ``where`` only."""
    assert mutate is None or mutate in MARG_VARIANTS
    N, M, L, _ = d.case
    Mp = R.plan_padded(M)
    mus, vars_ = [], []
    for l in range(L):
        Uh, Ulo, Ph, Pl = marg_operands(d, Uv[l])
        acc = np.zeros((Mp, N), f32)
        for k in range(Mp // STAGE):
            rows, cols = slice(STAGE * k, Mp), slice(STAGE * k, STAGE * (k + 1))
            mu_ = mutate if (k == where or where == ALL) else None
            uh, ul, ph, pl = Uh[rows, cols], Ulo[rows, cols], Ph[:, cols], Pl[:, cols]
            if mu_ == "truncated_hi_no_lo":
                uh, ph = trunc16((uh + ul).astype(f32)), trunc16((ph + pl).astype(f32))
                ul, pl = np.zeros_like(ul), np.zeros_like(pl)
            acc[rows] += uh @ ph.T
            if mu_ not in ("Phi_lo_dropped", "stage_planes_dropped"):
                acc[rows] += uh @ pl.T
            if mu_ == "lo_hi_from_wrong_operand":
                acc[rows] += uh @ pl.T
            elif mu_ not in ("U_lo_dropped", "stage_planes_dropped"):
                acc[rows] += ul @ ph.T
        vp = np.zeros(Mp, f32)
        vp[:M] = v32[l]
        q = _row_sums(acc, None) * f32(2.0 ** -(2 * (d.e + 15)))
        m = _row_sums(acc, vp) * f32(2.0 ** -(d.e + 15))
        qs, ms = np.zeros(N, f32), np.zeros(N, f32)
        for rb in range(Mp // 256):
            qs, ms = (qs + q[rb]).astype(f32), (ms + m[rb]).astype(f32)
        mus.append(ms)
        vars_.append((d.resid + qs).astype(f32))
    mu, var = np.array(mus), np.array(vars_)
    c = np.sqrt((mu.astype(f64) * mu + var).astype(f32)).astype(f32)
    return MargRef(mu, var, c)


def marg_visibility(d, Uv, bars, whole=False):
    """min over latents, live stages and the two cross terms (U_hi Phi_lo, U_lo Phi_hi of that stage alone; ``whole``: of all stages
    together) of max over the points of the change of var the term stands for, 2 sum_a |T_an X_an|, over bar_var."""
    N, M, L, _ = d.case
    worst = np.inf
    for l in range(L):
        Uh, Ulo, Ph, Pl = (x.astype(f64) for x in marg_operands(d, Uv[l]))
        T = np.tril(Uv[l]) @ d.Phi.astype(f64).T
        s = 2.0 ** -(d.e + 15)
        for k in range(1 if whole else S.cdiv(M, STAGE)):
            cols = slice(0, R.plan_padded(M)) if whole else slice(STAGE * k, STAGE * (k + 1))
            for X in (Uh[:M, cols] @ Pl[:, cols].T, Ulo[:M, cols] @ Ph[:, cols].T):
                worst = min(worst, float((2 * np.abs(T * X * s).sum(0) / bars.var[l]).max()))
    return worst
