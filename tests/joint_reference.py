"""Float64 reference, element-wise error bars and a numpy model of the joint posterior covariance at new inputs
(include/agpl_joint.h: agpl_plan_predict_cov), for tests/test_gpu_predict_cov.py and tests/test_joint_reference_cpu.py.  No GPU, no
library code: nothing here imports the package.

reference
    Cov_l[i][j] = k(x_a_i, x_b_j) + phi(x_a_i)' W_l phi(x_b_j),  W_l = U_l' U_l - I,  k = s2 kappa(r),  r^2 = sum_d ((x_a - x_b) / ell)_d^2,
    everything in float64; kappa as KernelFunctions.jl states the five kinds of include/agpl_kernels.h.

bars (element-wise, from the arithmetic the header documents).  Phi_a and Phi_b are the device's own features, hi + lo of their
images at the plan's scale 2^e, so their split is exact; EPS(Mp) = 2^-21 + Mp 2^-24 is tests/chain_reference.py's relative bar of
one split operand in a product of length Mp (float32 rounding of the scaled entry, the rounding of lo, the dropped lo lo product,
float32 accumulation).
    * T = W Phi_b, W split at 2^15:       B1[a][j] = EPS sum_k |W_ak| |phi_jk| + 2^-25 2^-15 sum_k |phi_jk|  (the second term: the
      float16 grid below 2^-14 of the scaled entries, chain_reference's absolute part; it also covers W formed in another order).
    * T split again at 2^e:               B2[a][j] = 2^-22 |T_aj| + 2^-25 2^-e   (T is float32 already: the rounding of lo, the grid).
    * Phi_a' T:                           sum_a |phi_ia| (B1 + B2)[a][j] + (2^-22 + Mp 2^-24) sum_a |phi_ia| |T_aj|
      (the dropped lo lo product of two split operands, float32 accumulation).
    * k = s2 kappa(r) in float32, r^2 rounded from float64: every rule is exp(-w) times a polynomial of at most three terms, with
      w = r^2/2 (SE), r (Matern 1/2), sqrt(3) r, sqrt(5) r (Matern 3/2, 5/2), alpha log1p(r^2 / (2 alpha)) (RQ).  w is formed with at
      most six float32 roundings (the cast of r^2 or r, the constant, the products; log1pf within two units, and
      d log1p(s) / d log s <= 1), an error 6 2^-24 w of the exponent, i.e. a relative error 6 2^-24 w of kappa; d(polynomial)/d log u is
      below the polynomial itself times 2, two more; expf within two units, the polynomial and s2 four more roundings:
                                          Bk = s2 kappa (8 w + 8) 2^-24.
    * the final sum:                      2^-23 (|quad| + |k|).
"""
from collections import namedtuple

import numpy as np

import chain_reference as CR

KINDS = ("se", "matern12", "matern32", "matern52", "rq")
ALPHA = 0.7
N_TRAIN = 300
JITTER = 1e-8
U_EXP = 15


def plan_padded(M):
    return (M + 255) // 256 * 256


def plan_scale_exp(s2):
    """e of a plan from raw inputs: 2^e smax in [2^13, 2^14), smax = 1.001 sigma rounded to float32 (agpl_se_create.h)."""
    return 13 - (int(np.frexp(np.float32(np.sqrt(s2) * (1.0 + 1e-3)))[1]) - 1)


# ---- the covariance functions ---------------------------------------------------------------------------------------------------------

def scaled_sqdist(xa, xb, ell):
    """r^2 [na, nb] in float64 from x / ell, summed over d ascending (the device's order)."""
    a, b = np.asarray(xa, np.float64) / ell, np.asarray(xb, np.float64) / ell
    r2 = np.zeros((a.shape[0], b.shape[0]))
    for d in range(a.shape[1]):
        u = a[:, d][:, None] - b[:, d][None, :]
        r2 += u * u
    return r2


def kappa(kind, r2, param=ALPHA, dtype=np.float64):
    """kappa(r) of ``kind``; dtype float32 restates the device's rule (agpl_kernel_rules.h): r in float64, everything after in float32."""
    T = dtype
    r2 = np.asarray(r2, np.float64)
    if kind == "se":
        return np.exp(T(-0.5) * r2.astype(T))
    r = np.sqrt(r2).astype(T)
    if kind == "matern12":
        return np.exp(-r)
    if kind == "matern32":
        u = T(1.7320508075688772) * r
        return (T(1) + u) * np.exp(-u)
    if kind == "matern52":
        u = T(2.23606797749979) * r
        return (T(1) + u + u * u * T(1.0 / 3.0)) * np.exp(-u)
    if kind == "rq":
        a = T(param)
        return np.exp(-a * np.log1p(r2.astype(T) / (T(2) * a)))
    raise ValueError(kind)


def exponent(kind, r2, param=ALPHA):
    """w of the module's docstring."""
    r = np.sqrt(r2)
    return {"se": 0.5 * r2, "matern12": r, "matern32": np.sqrt(3.0) * r, "matern52": np.sqrt(5.0) * r,
            "rq": param * np.log1p(r2 / (2.0 * param))}[kind]


def kernel(kind, xa, xb, ell, s2, param=ALPHA):
    return s2 * kappa(kind, scaled_sqdist(xa, xb, ell), param)


def phi_f64(kind, x, z, ell, s2, param=ALPHA, jitter=JITTER):
    """Phi [n, M] = (L^-1 K_ZX)' in float64, K_ZZ + jitter I = L L'."""
    Lc = np.linalg.cholesky(kernel(kind, z, z, ell, s2, param) + jitter * np.eye(len(z)))
    return np.linalg.solve(Lc, kernel(kind, z, x, ell, s2, param)).T


# ---- the reference and its bars ---------------------------------------------------------------------------------------------------------

def w_of_u(U):
    """W [L, M, M] = U' U - I from U [L, M, M] (lower triangular: U[l][a][b], b <= a)."""
    U = np.tril(np.asarray(U, np.float64))
    return np.einsum("lca,lcb->lab", U, U) - np.eye(U.shape[-1])


def reference(Phi_a, Phi_b, W, K):
    """Cov [L, na, nb] in float64."""
    Phi_a, Phi_b = np.asarray(Phi_a, np.float64), np.asarray(Phi_b, np.float64)
    return K[None] + np.stack([Phi_a @ W[l] @ Phi_b.T for l in range(W.shape[0])])


Bars = namedtuple("Bars", "total quad k")


def bars(Phi_a, Phi_b, W, kind, r2, s2, Mp, e, param=ALPHA):
    """Element-wise bars [L, na, nb] on |Cov - Cov_ref| (the module's docstring); .k: the part of the kernel term alone."""
    A, B = np.abs(np.asarray(Phi_a, np.float64)), np.abs(np.asarray(Phi_b, np.float64))
    E = CR.eps(Mp)
    t = np.einsum("lab,jb->laj", W, np.asarray(Phi_b, np.float64))
    b1 = E * np.einsum("lab,jb->laj", np.abs(W), B) + 2.0 ** -25 * 2.0 ** -U_EXP * B.sum(1)[None, None, :]
    b2 = 2.0 ** -22 * np.abs(t) + 2.0 ** -25 * 2.0 ** -e
    quad_abs = np.einsum("ia,laj->lij", A, np.abs(t))
    b_quad = np.einsum("ia,laj->lij", A, b1 + b2) + (2.0 ** -22 + Mp * 2.0 ** -24) * quad_abs
    k = s2 * kappa(kind, r2, param)
    b_k = k * (8.0 * exponent(kind, r2, param) + 8.0) * 2.0 ** -24
    quad = np.einsum("ia,laj->lij", np.asarray(Phi_a, np.float64), t)
    total = b_quad + b_k[None] + 2.0 ** -23 * (np.abs(quad) + np.abs(k)[None])
    return Bars(total, b_quad, b_k + 2.0 ** -23 * np.abs(k))


def predict_var_bar(Phi, U, s2, Mp):
    """Bar [L, n] on agpl_plan_predict's var = (s2 - |phi|^2) + |U phi|^2 against float64 with the same features: U is split at 2^15 as
    W is (B_u[a] = EPS sum_k |U_ak| |phi_k| + 2^-25 2^-15 sum_k |phi_k| on each T_a = (U phi)_a), the squares are summed in float32
    (2 |T| B_u + B_u^2 + Mp 2^-24 T^2 each), |phi|^2 is a float32 sum of Mp squares and the residual and the final sum round once each."""
    Phi, U = np.asarray(Phi, np.float64), np.tril(np.asarray(U, np.float64))
    t = np.einsum("lab,nb->lna", U, Phi)
    bu = CR.eps(Mp) * np.einsum("lab,nb->lna", np.abs(U), np.abs(Phi)) + 2.0 ** -25 * 2.0 ** -U_EXP * np.abs(Phi).sum(1)[None, :, None]
    ssq = (Phi * Phi).sum(1)
    return (2 * np.abs(t) * bu + bu * bu + Mp * 2.0 ** -24 * t * t).sum(2) + Mp * 2.0 ** -24 * ssq[None] + 2.0 ** -22 * (s2 + (t * t).sum(2))


# ---- the cases of tests/test_gpu_predict_cov.py -----------------------------------------------------------------------------------------

Case = namedtuple("Case", "M L D kind Na Nb sym")
Case.id = property(lambda c: f"M{c.M}-L{c.L}-D{c.D}-{c.kind}-{c.Na}x{c.Nb}" + ("-sym" if c.sym else ""))

# every M in {5, 64, 256, 300} (Mp 256 and 512), L in {1, 3}, D in {1, 2, 16}, every kind, and each of 1, 127, 128, 129, 257 as Na and as Nb
TIGHT = [Case(5, 1, 1, "se", 1, 257, False), Case(64, 3, 2, "matern32", 127, 129, False), Case(256, 1, 1, "matern12", 128, 127, False),
         Case(300, 3, 2, "rq", 129, 128, False), Case(64, 1, 16, "matern52", 257, 1, False), Case(300, 1, 2, "se", 257, 257, True),
         Case(64, 3, 2, "se", 129, 129, True)]
FRESH = Case(64, 1, 2, "matern52", 129, 257, False)   # U = I: the prior covariance
SAMPLE = Case(64, 3, 2, "matern52", 257, 257, True)    # sample_f (variance 2.5: jitter variance I is not jitter I)


def workload(N, M, D, seed=3):
    """tests/test_gpu_plan_inputs.py::workload, restated."""
    rng = np.random.default_rng(seed)
    x = rng.uniform(-10, 10, size=(N, D))
    if D == 1:
        z = np.linspace(-10, 10, M)[:, None]
        ell = np.array([1.5 * 20 / (M - 1)])
    else:
        z = rng.uniform(-10, 10, size=(M, D))
        ell = np.array([1.0, 1.4, 1.8][:D]) if D <= 3 else np.full(D, 12.0)
    return x, z, ell


Data = namedtuple("Data", "x z ell s2 param xa xb G g")


def case_data(c, fresh=False):
    """The plan's inputs (x [300, D], z [M, D], ell, s2), the test inputs xa [Na, D], xb [Nb, D] (xb = xa for the symmetric form) and
    natural parameters (G [L, M, M] positive semi-definite, g [L, M]) whose update gives a q(v) with U != I, different per latent."""
    if c.D == 2 and c.M in CR.GRIDS:
        x, z, ell = CR.se_inputs(c.M)
    else:
        x, z, ell = workload(N_TRAIN, c.M, c.D)
    rng = np.random.default_rng([c.M, c.L, c.D, KINDS.index(c.kind), c.Na, c.Nb])
    xa = rng.uniform(-10, 10, size=(c.Na, c.D))
    xb = xa if c.sym else rng.uniform(-10, 10, size=(c.Nb, c.D))
    s2 = 1.0 if c.kind in ("se", "matern12") else 2.5
    B = rng.standard_normal((c.L, c.M, max(2, c.M // 2)))
    G = np.einsum("lak,lbk->lab", B, B) * (0.5 + np.arange(c.L))[:, None, None]
    if fresh:
        G = np.zeros_like(G)
    return Data(x, z, ell, s2, ALPHA, xa, xb, G, rng.standard_normal((c.L, c.M)))


def u_of_g(G):
    """U [L, M, M] = chol(I + G)^-1 (lower) in float64: the factor agpl_plan_update keeps."""
    return np.stack([np.linalg.inv(np.linalg.cholesky(np.eye(G.shape[-1]) + G[l])) for l in range(G.shape[0])])


# ---- the model ------------------------------------------------------------------------------------------------------------------------

MUTATIONS = ("no_minus_identity", "u_for_utu", "uut_for_utu", "kernel_term_transposed", "no_lo_plane_of_t", "w_of_latent_0")


def visible(mutate, c, fresh=False):
    """Whether a wrong variant changes the result on a case's data at all: with U = I every W is 0 whatever its latent or transpose;
    one latent has no other latent's W; k of the symmetric form is its own transpose."""
    if mutate == "w_of_latent_0":
        return c.L > 1 and not fresh
    if mutate == "kernel_term_transposed":
        return not c.sym and (c.Na > 1 or c.Nb > 1)
    if mutate == "no_minus_identity":
        return True
    if mutate == "uut_for_utu":
        return not fresh and c.M > 1
    return not fresh


def feature_image(Phi, e):
    """The image of Phi at the plan's scale (float16 hi + lo, zero-padded to Mp) and the features it holds exactly."""
    Phi = np.asarray(Phi, np.float64)
    hi, lo = CR.split16(Phi, e, plan_padded(Phi.shape[1]))
    return (hi, lo), ((hi.astype(np.float64) + lo) * 2.0 ** -e)[:, : Phi.shape[1]]


def model(img_a, img_b, U, kind, xa, xb, ell, s2, e, param=ALPHA, mutate=None):
    """Cov [L, na, nb] float32 as the header's numerics paragraph states it; img_a / img_b from feature_image; U [L, M, M]."""
    assert mutate is None or mutate in MUTATIONS
    f32 = np.float32
    (Ah, Al), (Bh, Bl) = img_a, img_b
    U = np.tril(np.asarray(U, np.float64))
    L, M, Mp = U.shape[0], U.shape[1], Ah.shape[1]
    I = np.eye(M)
    r2 = scaled_sqdist(xa, xb, ell)
    if mutate == "kernel_term_transposed":
        na, nb = r2.shape
        r2 = scaled_sqdist(xa[np.arange(nb) % na], xb[np.arange(na) % nb], ell).T
    k = f32(s2) * kappa(kind, r2, f32(param), f32)
    out = np.empty((L,) + r2.shape, f32)
    for l in range(L):
        Ul = U[0 if mutate == "w_of_latent_0" else l]
        W = {None: Ul.T @ Ul - I, "no_minus_identity": Ul.T @ Ul, "u_for_utu": Ul - I, "uut_for_utu": Ul @ Ul.T - I}.get(mutate, Ul.T @ Ul - I)
        Wh, Wl = CR.split16(W, U_EXP, Mp)
        Wh, Wl = np.pad(Wh, ((0, Mp - M), (0, 0))), np.pad(Wl, ((0, Mp - M), (0, 0)))
        T = f32(2.0 ** -U_EXP) * CR._project(Wh, Wl, Bh, Bl)  # [Mp, nb] at 2^e
        Th = T.astype(np.float16).astype(f32)
        Tl = np.zeros_like(Th) if mutate == "no_lo_plane_of_t" else (T - Th).astype(np.float16).astype(f32)
        quad = f32(2.0 ** (-2 * e)) * CR._project(Ah, Al, np.ascontiguousarray(Th.T), np.ascontiguousarray(Tl.T))
        out[l] = quad + k
    return out
