"""Reference side of the dense-route tile tests (tests/test_dense_reference_cpu.py, tests/test_gpu_dense_tiles.py).

Four things, numpy only:

1. the tile constants of csrc/agpl_dense.hip, read from the source;
2. the matrix families: two new ones whose entries are O(1) at every index distance (`exp_perm`, `wishart`) and the banded
   squared-exponential matrices of the existing dense tests (`se_sorted`);
3. a model of the two blocked factorisations as the source states them, block by block and tile by tile, with hooks that (a) watch
   what every tile contributes and (b) inject one wrong tile;
4. the bars of the device tests, with their derivation, and the comparison functions that apply them.

---------------------------------------------------------------------------------------------------------------------------------
The bars.  u = 2^-53, gamma_k = k u / (1 - k u), n the order of the matrix.

(a) Look-ahead factor, entry-wise backward error.  Textbook (Higham, Accuracy and Stability, Thm 10.3): every entry of the factor
    is (a_ij - sum_k l_ik l_jk) / l_jj evaluated in ANY order with at most n + 1 roundings on any term, hence
    |K - L L'| <= gamma_{n+1} |L| |L|'.  What the kernels add to that count:
      * The tile routine sums the w products of a panel in one FMA chain through the MFMA accumulator (16 columns per stage, 4 per
        instruction): w roundings for w terms, the textbook count -- and then ONE subtraction from the stored entry.  An entry sees
        one such subtraction per outer step (at most n / NB) and per 64-column step inside its own diagonal block (at most NB / PB).
      * potrf64 replaces sqrt and divide by rsq + two Newton steps and a multiply: at most 6 roundings where the textbook has 1.
      So the chain is at most n + 1 + n / NB + NB / PB + 6 roundings long:   c_chain = (n + 7 + n / NB + NB / PB) / (n + 1).
      * The rows below a 64-column pivot block are multiplied by the EXPLICIT inverse U = R^-1 (panel_solve_kernel), and rocBLAS'
        dtrsm of the 2048-wide panel inverts 128-wide diagonal blocks in the same way.  x = fl(a fl(R^-1)') has the residual
        |x R' - a| <= gamma_w (rho + rho^2) |x| |R'| with rho = || |R^-1| |R| ||_inf (the product's own w-term chain, and Higham
        sec. 14.2: |fl(R^-1) - R^-1| <= gamma_w |R^-1| |R| |R^-1|), against gamma_w of a substitution.  This is a norm-wise
        argument, not an entry-wise one, and it is the one place where a condition number enters: rho is taken from the REFERENCE
        factor's 128-wide diagonal blocks (rho of a block bounds rho of its two 64-wide halves), so
            c_inv = 2 * 128 * rho^2 / (n + 1)        (rho^2 <= cond_2 of the pivot block).
      * Forming R = K - L L' in float64 to look at it costs gamma_{n+1} |L| |L|' itself (n-term dot product, one subtraction):
            c_eval = 1.
      bar_ij = (c_chain + c_inv + c_eval) gamma_{n+1} (|Lref| |Lref|')_ij     with Lref = np.linalg.cholesky(K).

(b) Dense step, forward error of f.  f = f0 + K D^1/2 s, s = B^-1 r, f0 = mu0 + L_K z1.
      * Solve (Higham Thm 10.4): (B + dB) s^ = r with |dB| <= gamma_{3n+1} |C| |C|' (factor and two substitutions),
        so ||dB||_2 / ||B||_2 <= 3 n u c_chain tau, tau = || |C| |C|' ||_2 / ||B||_2 in [1, n] (taken from the reference factor), and
            ||s^ - s||_2 <= cond_2(B) n u c ||s||_2,     c = 3 c_chain tau + c_inv_blocks.
        The inverse-block route multiplies by U_k = chol(D_k)^-1 in the panel and in both substitutions; by the argument of (a)
        each costs a factor of at most rho_k^2 <= cond_2(D_k) <= cond_2(B) on a 1024-term chain:
            c_inv_blocks = 3 * 2 * DB * max_k cond_2(D_k) / n       (D_k from the reference factor's diagonal blocks).
        The look-ahead step (N % 1024 != 0) uses substitutions on the diagonal blocks; the same c covers it.
      * f0: the device draws with ITS factor of K, and every factor of K gives an exact draw.  The device test therefore checks
        that factor against bar (a) first and hands it to the oracle, so that both sides form f0 = mu0 + L z1 from the same L; what
        is left is the rounding of the product, |df0| <= gamma_n |L| |z1| per entry.  f depends on f0 through (I + K D)^-1, of
        2-norm at most sqrt(cond_2(K)).
      * The symv: gamma_{n+2} |K| |D^1/2 s| per entry.
      bar = sqrt(cond_2 K) * df0  +  max_i ||(K D^1/2)_i||_2 * ds  +  gamma_{n+2} max_i (|K| |D^1/2 s|)_i      (max norm of f).
    Every quantity is computed from the reference's own K, B, s.  This is a worst-case norm bound: ||s||_2 and the row norms of
    K D^1/2 each cost a factor of up to sqrt(n), and for exp_perm (cond_2(B) ~ 1.5e4, cond_2(D_k) of the same order) it comes out
    ABOVE the flat 1e-6 max(1, max|f|) of the existing dense-step tests.  The tests therefore assert
            max|f - ref| <= min(bar (b), 1e-6 max(1, max|f|)),
    never less than the existing tests ask; test_dense_reference_cpu.py injects a dropped stage and a stale U_k at N = 8192 with
    the source's widths on both families and asserts that this bar rejects them.

(c) Visibility.  A tile's contribution (the 128 x 128 product an update tile subtracts; the raw rows a panel row tile multiplies)
    is certainly VISIBLE if one of its entries exceeds an upper bound of bar (a) there, gamma_{n+1} c sqrt(a_ii a_jj)
    ((|L||L|')_ij <= ||l_i|| ||l_j||), and certainly INVISIBLE if every entry is at or below a lower bound of it,
    gamma_{n+1} c |a_ij| (|a_ij| <= (|L||L|')_ij).  For the dense step the matrix is B; bar (b) is this backward bar times
    cond_2(B), so the same condition applies.
"""
import math
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DENSE_SRC = os.path.join(ROOT, "augmentedgplikelihoods.jl_amd", "csrc", "agpl_dense.hip")
U = 2.0 ** -53


def gamma_k(k):
    return k * U / (1.0 - k * U)


# ----------------------------------------------------------------------------------------------------------- constants
def read_constants(path=DENSE_SRC):
    """kTT, kTK, kPB, kDB, AGPL_DENSE_NB and the blocking threshold, as written in the source."""
    src = open(path).read()
    out = {}
    for name in ("kTT", "kTK", "kPB", "kDB"):
        m = re.findall(r"constexpr\s+int\s+%s\s*=\s*(\d+)\s*;" % name, src)
        assert len(m) == 1, (name, m)
        out[name] = int(m[0])
    m = re.findall(r"#define\s+AGPL_DENSE_NB\s+(\d+)", src)
    assert len(m) == 1, m
    out["NB"] = int(m[0])
    m = re.findall(r"constexpr\s+int64_t\s+nb\s*=\s*(\w+)\s*;", src)  # blocked_potrf_steps: the macro; blocked_potrs_vec: a literal
    assert sorted(m) == sorted(["AGPL_DENSE_NB", str(out["NB"])]), m
    thr = set(re.findall(r"N\s*>=\s*(\d+)", src))
    assert len(thr) == 1, thr
    out["THRESHOLD"] = int(thr.pop())
    assert re.search(r"inv_route\s*=\s*N\s*>=\s*%d\s*&&\s*N\s*%%\s*kDB\s*==\s*0" % out["THRESHOLD"], src)
    return out


class Blocking:
    """Block widths of both routes (the source's by default; the sensitivity tests scale all of them down together)."""

    def __init__(self, tt, tk, pb, nb, db):
        assert nb % tk == 0 and nb % tt == 0 and nb % pb == 0 and db % tt == 0 and pb % tk == 0 and db % tk == 0
        self.tt, self.tk, self.pb, self.nb, self.db = tt, tk, pb, nb, db

    @classmethod
    def from_source(cls):
        c = read_constants()
        return cls(c["kTT"], c["kTK"], c["kPB"], c["NB"], c["kDB"])

    def scaled(self, by):
        return Blocking(self.tt // by, self.tk // by, self.pb // by, self.nb // by, self.db // by)


# ------------------------------------------------------------------------------------------------------------ matrices
def exp_perm(N, seed=0):
    """exp(-|x_i - x_j| / 0.5) + 1e-2 I, x uniform on [0, 1] in a fixed random order: every entry >= e^-2."""
    rng = np.random.default_rng([seed, N, 1])
    x = rng.uniform(0.0, 1.0, size=N)  # (drawn in random order: never sorted)
    K = np.exp(-np.abs(x[:, None] - x[None, :]) / 0.5)
    K[np.diag_indices(N)] += 1e-2
    return K


def wishart(N, seed=0, p=64):
    """I + W W' / p, W [N, p] Gaussian: cond_2 ~ N / p, off-diagonal entries ~ p^-1/2 at every index distance."""
    rng = np.random.default_rng([seed, N, 2])
    W = rng.standard_normal((N, p))
    K = W @ W.T / p
    K[np.diag_indices(N)] += 1.0
    return K


FAMILIES = {"exp_perm": exp_perm, "wishart": wishart}


def se_sorted(N, span, ell, jitter, seed):
    """The existing dense tests' matrix: exp(-((x - x') / ell)^2 / 2) + jitter I on N SORTED uniform points over `span` units."""
    x = np.sort(np.random.default_rng(seed).uniform(-span / 2, span / 2, size=N))
    K = np.exp(-0.5 * ((x[:, None] - x[None, :]) / ell) ** 2)
    K[np.diag_indices(N)] += jitter
    return K


# (name, route, N, span, ell, jitter, seed): the constants of test_dense_cholesky_blocked_route[_with_an_odd_order]
# (tests/test_gpu_parity.py, test_gpu_regressions_r4.py; the device generator's draws are replaced by numpy's: the band is a matter
# of density) and of test_dense_gibbs_step_blocked_routes_match_oracle / ..._inverse_block_route_matches_oracle
EXISTING = [
    ("cholesky_blocked_route", "lookahead", 8192 + 1000, 40.0, 0.05, 1e-3, 3),
    ("cholesky_odd_order", "lookahead", 8192 + 1001, 40.0, 0.05, 1e-3, 3),
    ("gibbs_blocked_routes", "lookahead", 8192 + 300, 800.0, 2.0, 1e-3, 37),
    ("gibbs_inverse_block", "inverse", 8192, 800.0, 2.0, 1e-3, 41 + 8192),
]


def student_like_gamma(N, seed=0):
    """Positive precisions of the size a Student-t (nu = 3.5, sigma = 2) step draws: Gamma(2.25) / 5, mean 0.45."""
    return np.random.default_rng([seed, N, 3]).gamma(2.25, 0.2, size=N)


def gibbs_matrix(K, gamma):
    sg = np.sqrt(gamma)
    B = sg[:, None] * K * sg[None, :]
    B[np.diag_indices(K.shape[0])] += 1.0
    return B


# ------------------------------------------------------------------------------------------------------------ the model
def tri_tiles_before(nt, J):
    return J * nt - J * (J - 1) // 2


def tile_of_index(nt, idx):
    J = 0
    while J + 1 < nt and tri_tiles_before(nt, J + 1) <= idx:
        J += 1
    return J + (idx - tri_tiles_before(nt, J)), J


class Fault:
    """One wrong tile.  kind: 'skip' | 'drop_stage' | 'swap' | 'late_launch' | 'stale_u'; where: 'outer' (the update after a whole
    panel) at `step`; tile (I, J) of that update's triangle (swap: and `other`); stale_u: panel row tile I of `step`."""

    def __init__(self, kind, step, tile=None, other=None):
        self.kind, self.step, self.tile, self.other = kind, step, tile, other
        self.hit = 0  # how many tiles it changed (the tests assert it was reached)


class Watch:
    """Counts, per kind of launch, the tiles whose contribution is certainly visible / certainly invisible under (c)."""

    def __init__(self, A0, c):
        self.lo = gamma_k(A0.shape[0] + 1) * c
        self.d = np.sqrt(np.diag(A0)).copy()
        self.A0 = A0
        self.counts = {}   # tag -> [tiles, certainly visible, certainly invisible]
        self.dark = []     # (tag, step, I, J) of tiles not certainly visible

    def see(self, tag, step, I, J, contrib, r0, c0):
        h, w = contrib.shape
        a = np.abs(contrib)
        hi = self.lo * self.d[r0:r0 + h, None] * self.d[None, c0:c0 + w]
        vis = bool((a > hi).any())
        inv = bool((a <= self.lo * np.abs(self.A0[r0:r0 + h, c0:c0 + w])).all())
        t = self.counts.setdefault(tag, [0, 0, 0])
        t[0] += 1
        t[1] += vis
        t[2] += inv
        if not vis:
            self.dark.append((tag, step, I, J))

    def share_invisible(self, tags):
        n = sum(self.counts[t][0] for t in tags if t in self.counts)
        return sum(self.counts[t][2] for t in tags if t in self.counts) / n

    def share_visible(self, tags):
        n = sum(self.counts[t][0] for t in tags if t in self.counts)
        return sum(self.counts[t][1] for t in tags if t in self.counts) / n


def _update(A, k0, w, lim, bl, launches, tag, step, fault, watch, group=8):
    """trailing_update_kernel: A[e:lim, e:lim] -= P P' on the lower-triangle tiles, P = A[e:lim, k0:e]; `launches` are the
    (base, count) index ranges of the 1-D grid.  `group` tile columns per matrix product (the tiles above the diagonal that a
    group's rectangle contains lie in the triangle nobody reads)."""
    tt = bl.tt
    e = k0 + w
    m = lim - e
    nt = -(-m // tt)
    P = np.ascontiguousarray(A[e:lim, k0:e])
    covered = np.zeros(tri_tiles_before(nt, nt), dtype=bool)
    for base, count in launches:
        covered[base:base + count] = True  # (an index past the triangle maps to a tile outside the matrix: nothing is stored)
    mine = fault is not None and fault.step == step and tag == "outer"
    for J0 in range(0, nt, group):
        g0, g1 = J0 * tt, min((J0 + group) * tt, m)
        big = P[g0:] @ P[g0:g1].T  # rows g0 .. m of these tile columns
        for J in range(J0, min(J0 + group, nt)):
            c0, c1 = J * tt, min((J + 1) * tt, m)
            for I in range(J, nt):
                r0, r1 = I * tt, min((I + 1) * tt, m)
                blk = big[r0 - g0:r1 - g0, c0 - g0:c1 - g0]
                if watch is not None:
                    watch.see(tag, step, I, J, blk, e + r0, e + c0)
                if not covered[tri_tiles_before(nt, J) + I - J]:
                    blk[:] = 0.0
                    if mine and fault.kind == "late_launch":
                        fault.hit += 1
                if mine and fault.kind in ("skip", "drop_stage", "swap") and (I, J) in (fault.tile, fault.other):
                    fault.hit += 1
                    if fault.kind == "skip":
                        blk[:] = 0.0
                    elif fault.kind == "drop_stage":
                        blk[:] = P[r0:r1, :w - bl.tk] @ P[c0:c1, :w - bl.tk].T
                    else:  # the workgroup computes the other tile's product and stores it here
                        Io, Jo = fault.other if (I, J) == fault.tile else fault.tile
                        blk[:] = P[Io * tt:Io * tt + (r1 - r0)] @ P[Jo * tt:Jo * tt + (c1 - c0)].T
        A[e + g0:lim, e + g0:e + g1] -= big


def _launches(nt, ncol1, fault, step):
    first = tri_tiles_before(nt, ncol1)
    total = tri_tiles_before(nt, nt)
    if nt <= ncol1:
        return [(0, total)]
    late = fault is not None and fault.kind == "late_launch" and fault.step == step
    return [(0, first), (first + (1 if late else 0), total - first)]


def lookahead_cholesky(K, bl, fault=None, watch=None):
    """blocked_potrf_steps: right-looking, NB-wide steps; a diagonal block goes PB columns at a time (potrf64 with U = R^-1, the
    rows below by B <- B U', the rest of the block by the update with w = PB), a ragged last block to LAPACK; the panel by a
    triangular solve; the update in two launches, block column k + 1 first.  Returns the lower factor."""
    import scipy.linalg as sla

    A = np.array(K, dtype=np.float64)
    N = A.shape[0]
    step = 0
    for k in range(0, N, bl.nb):
        e = min(k + bl.nb, N)
        w = e - k
        if w % bl.pb == 0:
            for j in range(0, w, bl.pb):
                kj = k + j
                R = np.linalg.cholesky(A[kj:kj + bl.pb, kj:kj + bl.pb])
                A[kj:kj + bl.pb, kj:kj + bl.pb] = R
                if kj + bl.pb < e:
                    Uj = sla.solve_triangular(R, np.eye(bl.pb), lower=True)
                    raw = A[kj + bl.pb:e, kj:kj + bl.pb]
                    if watch is not None:
                        for I in range(-(-(e - kj - bl.pb) // bl.tt)):
                            r0 = kj + bl.pb + I * bl.tt
                            watch.see("inner_panel", (step, j // bl.pb), I, 0, raw[I * bl.tt:(I + 1) * bl.tt], r0, kj)
                    A[kj + bl.pb:e, kj:kj + bl.pb] = raw @ Uj.T
                    nt = -(-(e - kj - bl.pb) // bl.tt)
                    _update(A, kj, bl.pb, e, bl, [(0, tri_tiles_before(nt, nt))], "inner", (step, j // bl.pb), None, watch)
        else:
            A[k:e, k:e] = np.linalg.cholesky(A[k:e, k:e])
        if e < N:
            A[e:, k:e] = sla.solve_triangular(np.tril(A[k:e, k:e]), A[e:, k:e].T, lower=True).T
            nt = -(-(N - e) // bl.tt)
            _update(A, k, w, N, bl, _launches(nt, min(nt, bl.nb // bl.tt), fault, step), "outer", step, fault, watch)
        step += 1
    return np.tril(A)


def inverse_block_factor(B, bl, fault=None, watch=None):
    """inverse_block_factor: per DB-wide block U_k = chol(D_k)^-1, the panel raw U_k' by row tiles, the update in one launch.
    Returns (L, Us): L holds the factor's panels below the diagonal blocks and chol(D_k) on them; Us the kept inverses."""
    import scipy.linalg as sla

    A = np.array(B, dtype=np.float64)
    N = A.shape[0]
    assert N % bl.db == 0
    Us = []
    for step, k in enumerate(range(0, N, bl.db)):
        e = k + bl.db
        Ck = np.linalg.cholesky(A[k:e, k:e])
        A[k:e, k:e] = Ck
        Us.append(sla.solve_triangular(Ck, np.eye(bl.db), lower=True))
        if e < N:
            raw = A[e:, k:e].copy()
            A[e:, k:e] = raw @ Us[step].T
            for I in range(-(-(N - e) // bl.tt)):
                rows = slice(I * bl.tt, min((I + 1) * bl.tt, N - e))
                if watch is not None:
                    watch.see("panel", step, I, 0, raw[rows], e + rows.start, k)
                if fault is not None and fault.kind == "stale_u" and fault.step == step and fault.tile == I:
                    fault.hit += 1
                    A[e + rows.start:e + rows.stop, k:e] = raw[rows] @ Us[step - 1].T
            nt = -(-(N - e) // bl.tt)
            _update(A, k, bl.db, N, bl, [(0, tri_tiles_before(nt, nt))], "outer", step, fault, watch)
    return np.tril(A), Us


def inverse_block_solve(L, Us, bl, r):
    """inverse_block_solve_vec: x <- B^-1 x with the kept U_k on the diagonal blocks and one matrix-vector product per panel."""
    x = np.array(r, dtype=np.float64)
    N = x.size
    for i, k in enumerate(range(0, N, bl.db)):
        e = k + bl.db
        x[k:e] = Us[i] @ x[k:e]
        if e < N:
            x[e:] -= L[e:, k:e] @ x[k:e]
    for i, k in reversed(list(enumerate(range(0, N, bl.db)))):
        e = k + bl.db
        if e < N:
            x[k:e] -= L[e:, k:e].T @ x[e:]
        x[k:e] = Us[i].T @ x[k:e]
    return x


def lookahead_solve(L, r):
    import scipy.linalg as sla

    return sla.cho_solve((L, True), r)


def gibbs_f(K, Lk, mu0, beta, gamma, z, solve):
    """The dense step's arithmetic after the draws (oracle.dense_gibbs_step's, with the solve left to the caller)."""
    N = K.shape[0]
    sg = np.sqrt(gamma)
    f0 = Lk @ z[:N] + mu0
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(sg > 0, beta / sg, 0.0) - sg * f0 - z[N:]
    s = solve(r)
    return f0 + K @ (sg * s), dict(f0=f0, r=r, s=s)


# ------------------------------------------------------------------------------------------------------------- the bars
def c_chain(n, bl):
    return (n + 7 + n / bl.nb + bl.nb / bl.pb) / (n + 1)


def rho_of_blocks(Lref, width):
    """max over the width-wide diagonal blocks R of the factor of || |R^-1| |R| ||_inf"""
    import scipy.linalg as sla

    rho = 1.0
    for k in range(0, Lref.shape[0], width):
        R = Lref[k:k + width, k:k + width]
        Ri = sla.solve_triangular(R, np.eye(R.shape[0]), lower=True)
        rho = max(rho, float((np.abs(Ri) @ np.abs(R)).sum(axis=1).max()))
    return rho


def cond_of_blocks(Lref, width):
    """max over the width-wide diagonal blocks C_kk of the factor of cond_2(C_kk C_kk') -- the pivot blocks D_k"""
    worst = 1.0
    for k in range(0, Lref.shape[0], width):
        sv = np.linalg.svd(Lref[k:k + width, k:k + width], compute_uv=False)
        worst = max(worst, float((sv[0] / sv[-1]) ** 2))
    return worst


def factor_margin(Lref, bl):
    """c of bar (a): (c_chain + c_inv + c_eval, its three parts)"""
    n = Lref.shape[0]
    rho = rho_of_blocks(Lref, 2 * bl.pb)
    parts = (c_chain(n, bl), 2.0 * (2 * bl.pb) * rho * rho / (n + 1), 1.0)
    return sum(parts), parts


def locate(i, j, bl):
    """(outer step whose update last touched entry (i, j), tile row, tile column of that update) for a failure message"""
    step = min(i, j) // bl.nb - 1
    if step < 0:
        return (0, None, None)
    e = (step + 1) * bl.nb
    return (step, (max(i, j) - e) // bl.tt, (min(i, j) - e) // bl.tt)


def check_factor(R, absLL, c, bl, xp=np):
    """bar (a) on a residual R = K - L L' (lower triangle): (ok, worst ratio, message).  xp: numpy, or torch for arrays on the
    device -- the device tests and the fault injections of the CPU module run this one function."""
    n = R.shape[0]
    ratio = xp.tril(xp.abs(R) / (c * gamma_k(n + 1) * absLL))
    flat = int(ratio.argmax())
    i, j = flat // n, flat % n
    worst = float(ratio[i, j])
    step, ti, tj = locate(i, j, bl)
    msg = "worst |R| / bar = %.4g at (%d, %d): R = %.3g, step %s, tile row %s, tile column %s" % (
        worst, i, j, float(R[i, j]), step, ti, tj)
    return worst <= 1.0, worst, msg


FLAT_F = 1e-6  # the existing dense-step tests' bar on f, relative to max(1, max|f|): the derived bar never exceeds it


def step_c(n, B_norm, absCC_norm, c_inv_blocks, bl):
    """c of bar (b)"""
    return 3.0 * c_chain(n, bl) * absCC_norm / B_norm + c_inv_blocks


def step_bar(K, Lk, cond_K, B_cond, absCC_norm, B_norm, gamma, z1, s, c_inv_blocks, bl, f_ref):
    """bar (b), in the max norm of f: (bar, (f0 part, solve part, symv part, flat bar)).  bar = min(derived, flat).  Every argument
    comes from the reference."""
    n = K.shape[0]
    sg = np.sqrt(gamma)
    c = step_c(n, B_norm, absCC_norm, c_inv_blocks, bl)
    ds = B_cond * n * U * c * float(np.linalg.norm(s))
    df0 = gamma_k(n) * float(np.linalg.norm(np.abs(Lk) @ np.abs(z1)))
    row = float(np.sqrt(((K * sg[None, :]) ** 2).sum(axis=1)).max())
    symv = gamma_k(n + 2) * float((np.abs(K) @ np.abs(sg * s)).max())
    flat = FLAT_F * max(1.0, float(np.abs(f_ref).max()))
    parts = (math.sqrt(cond_K[0] * cond_K[1]) * df0, row * ds, symv, flat)
    return min(sum(parts[:3]), flat), parts


def power_norms(M, C, iters=60, seed=1):
    """(smallest eigenvalue of M, largest eigenvalue of M, || |C| |C|' ||_2) for M = C C' by power iteration on M, M^-1 and
    |C| |C|'.  Rayleigh quotients: the largest values are approached from below and the smallest from above, so neither cond_2(M)
    nor the norm is overstated (a bar built from them is never widened)."""
    import scipy.linalg as sla

    rng = np.random.default_rng(seed)
    v = rng.standard_normal(M.shape[0])
    w, a = v.copy(), np.abs(v)
    Ca = np.abs(C)
    Cf = np.asfortranarray(C)  # (LAPACK's layout, once: cho_solve would copy the factor on every call)
    for _ in range(iters):
        v = M @ v
        v /= np.linalg.norm(v)
        w = sla.cho_solve((Cf, True), w, check_finite=False)
        w /= np.linalg.norm(w)
        a = Ca @ (Ca.T @ a)
        a /= np.linalg.norm(a)
    return float(w @ (M @ w)), float(v @ (M @ v)), float(np.linalg.norm(Ca.T @ a) ** 2)


def step_bar_from_reference(K, Lk, B, Cref, gamma, z1, s, bl, f_ref):
    """bar (b) with the norms taken from the reference matrices themselves (power iteration: power_norms)."""
    n = K.shape[0]
    kmin, kmax, _ = power_norms(K, Lk)
    bmin, bmax, acc = power_norms(B, Cref)
    c_inv_blocks = 3.0 * 2.0 * bl.db * cond_of_blocks(Cref[:n - n % bl.db, :n - n % bl.db], bl.db) / n
    return step_bar(K, Lk, (kmax, 1.0 / kmin), bmax / bmin, acc, bmax, gamma, z1, s, c_inv_blocks, bl, f_ref)
