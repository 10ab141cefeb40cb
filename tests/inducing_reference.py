"""The float64 numpy yardstick of the k-means inducing inputs (include/agpl_inducing.h), for tests/test_gpu_inducing.py and
tests/test_inducing_reference_cpu.py: the Lloyd step, the fixed-point rule and the near-tie measure, each stated once.  No GPU, no
torch."""
from collections import namedtuple

import numpy as np

Case = namedtuple("Case", "id N M D ell")

# (N, M, D) of the issue; `ell` None = 1 in every dimension
CASES = [
    Case("n5000-m5-d1", 5000, 5, 1, None),
    Case("n4097-m64-d2", 4097, 64, 2, None),
    Case("n8193-m257-d16", 8193, 257, 16, None),          # M crosses a 256-centre chunk, D at its maximum
    Case("n20000-m300-d3-ell", 20000, 300, 3, (1.0, 2.0, 0.5)),
]
LLOYD = CASES                                              # the cases whose six Lloyd steps are followed (assertion 5)
BIG_M = Case("n4096-m2048-d1", 4096, 2048, 1, None)       # the largest M
GLOBAL_ACC = Case("n4099-m900-d16", 4099, 900, 16, None)  # M (D + 2) 8 bytes beyond the LDS budget: global integer atomics
OWN_CENTRE = Case("n300-m300-d2", 300, 300, 2, None)      # N = M
STEP_CASES = CASES + [BIG_M, GLOBAL_ACC, OWN_CENTRE]
NITER = 6
TIE_REL = 1e-9          # two nearest centres closer than this (relative): the point is left out of the assignment check
TIE_CAP = 1e-3          # at most this fraction of the points may be left out
LDS_BUDGET = 144 * 1024  # csrc/agpl_inducing.hip: the chunk (256 centres) + 16 lengthscales + the accumulator


def lds_accumulator(M, D):
    """Whether the step keeps its accumulator in LDS at (M, D) (csrc/agpl_inducing.hip: km_step_launch)."""
    return 8 * (256 * D + 16) + 8 * M * (D + 2) <= LDS_BUDGET


def tile_points(D):
    """Points a workgroup takes at a time (512 lanes, 4 points per lane for D <= 8, else 2)."""
    return 512 * (4 if D <= 8 else 2)


def ell_of(c):
    return np.ones(c.D) if c.ell is None else np.asarray(c.ell, dtype=np.float64)


def data(c, quarter=False):
    """A mixture of four shifted normals, [N, D] float64; `quarter`: rounded to multiples of 1/4 (every distance exact in float64)."""
    rng = np.random.default_rng(7000 + 131 * c.N + 17 * c.M + c.D)
    shifts = rng.uniform(-6.0, 6.0, size=(4, c.D))
    scales = np.array([0.6, 1.0, 1.5, 0.8])
    k = rng.integers(0, 4, size=c.N)
    x = shifts[k] + scales[k, None] * rng.standard_normal((c.N, c.D))
    return np.round(x * 4.0) / 4.0 if quarter else x


def start(c, x):
    """A stratified start for the CPU-only tests (the device's own indices come from its Philox stream): the middle of each stratum."""
    j = np.arange(c.M)
    lo, hi = j * c.N // c.M, (j + 1) * c.N // c.M
    return x[(lo + hi) // 2].copy()


def bound_of(x, ell):
    b = float(np.abs(x / ell).max())
    return b if b > 0.0 else 1.0


def sqdist(x, z, ell):
    """r2 [N, M] = sum over d ascending of (x_d / ell_d - z_d / ell_d)^2, float64."""
    u, zs = x / ell, z / ell
    r2 = np.zeros((x.shape[0], z.shape[0]))
    for d in range(x.shape[1]):
        t = u[:, d:d + 1] - zs[None, :, d]
        r2 += t * t
    return r2


def fused_r2(x, z, ell, a):
    """r2 of point i to centre a[i] as the device forms it: t = x_d / ell_d - z_d / ell_d, r <- fma(t, t, r) over d ascending -- one
    rounding per term, reproduced with exact rationals (float() of a Fraction rounds correctly)."""
    from fractions import Fraction

    u, zs = x / ell, (z / ell)[a]
    out = np.empty(x.shape[0])
    for i in range(x.shape[0]):
        r = 0.0
        for d in range(x.shape[1]):
            t = Fraction(float(u[i, d] - zs[i, d]))
            r = float(t * t + Fraction(r))
        out[i] = r
    return out


def assignment(r2):
    """(argmin with the lowest index on a tie, min r2, near-tie mask: the two smallest r2 within TIE_REL relative)."""
    a = np.argmin(r2, axis=1)
    if r2.shape[1] == 1:
        return a, r2[:, 0].copy(), np.zeros(r2.shape[0], dtype=bool)
    two = np.partition(r2, 1, axis=1)[:, :2]
    near = (two[:, 1] - two[:, 0]) <= TIE_REL * two[:, 1]
    return a, two[:, 0], near


def lloyd_step(x, z, ell):
    """One float64 Lloyd step in the scaled metric: (new z in input units, assignment, cost, near-tie mask, empty centres).  A centre
    without points keeps its value."""
    a, dmin, near = assignment(sqdist(x, z, ell))
    M = z.shape[0]
    cnt = np.bincount(a, minlength=M)
    znew = z.copy()
    u = x / ell
    for d in range(x.shape[1]):
        s = np.bincount(a, weights=u[:, d], minlength=M)
        znew[cnt > 0, d] = ell[d] * (s[cnt > 0] / cnt[cnt > 0])
    return znew, a, float(dmin.sum()), near, int((cnt == 0).sum())


# ---- the fixed-point rule (include/agpl_inducing.h) ----------------------------------------------------------------------------------

def ceil_log2(n):
    c = 0
    while (1 << c) < n:
        c += 1
    return c


def quanta(bound, N_total, D, variant=None):
    """(sx, sd).  `variant` "no-count": the number of points left out of the overflow bound (a wrong rule, for the CPU test)."""
    eb = int(np.frexp(bound)[1])
    cl = 0 if variant == "no-count" else ceil_log2(N_total)
    clamp = lambda s: max(-1000, min(1000, s))
    return clamp(61 - cl - eb), clamp(61 - cl - 2 * eb - 2 - ceil_log2(D))


def accumulate(x, ell, a, dmin, bound, N_total, M, variant=None):
    """acc int64 [M, D + 2] of the points x under the assignment a with their min distances dmin: count, rint(u 2^sx), rint(min(r2,
    4 D bound^2) 2^sd), summed in (wrapping) int64.  `variant` "wrong-quantum": sx one too small."""
    D = x.shape[1]
    sx, sd = quanta(bound, N_total, D, variant)
    if variant == "wrong-quantum":
        sx -= 1
    acc = np.zeros((M, D + 2), dtype=np.int64)
    np.add.at(acc[:, 0], a, 1)
    u = x / ell
    with np.errstate(over="ignore"):
        for d in range(D):
            np.add.at(acc[:, 1 + d], a, np.rint(np.ldexp(u[:, d], sx)).astype(np.int64))  # |q| <= 2^61 under every variant
        np.add.at(acc[:, D + 1], a, np.rint(np.ldexp(np.minimum(dmin, 4.0 * D * bound * bound), sd)).astype(np.int64))
    return acc


def centres(acc, z, ell, bound, N_total, variant=None):
    """(z, empty, movement, cost) from a summed acc: z_jd = ell_d * ((double(S) / double(count)) * 2^-sx); count 0 keeps its value.
    `variant` "no-ell": the centres are left in scaled units."""
    D = z.shape[1]
    sx, sd = quanta(bound, N_total, D, "no-count" if variant == "no-count" else None)
    cnt = acc[:, 0]
    live = cnt > 0
    znew = z.copy()
    for d in range(D):
        un = np.ldexp(acc[live, 1 + d].astype(np.float64) / cnt[live].astype(np.float64), -sx)
        znew[live, d] = un if variant == "no-ell" else ell[d] * un
    dz = (znew - z) / ell
    move = float(np.sqrt((dz * dz).sum(axis=1).max()))
    cost = float(np.ldexp(float(int(acc[:, D + 1].sum())), -sd))
    return znew, int((~live).sum()), move, cost


def fixed_point_step(x, z, ell, bound, variant=None):
    """The device's step and update as numpy models them: (new z, acc, cost)."""
    a, dmin, _ = assignment(sqdist(x, z, ell))
    acc = accumulate(x, ell, a, dmin, bound, x.shape[0], z.shape[0], variant)
    znew, _, _, cost = centres(acc, z, ell, bound, x.shape[0], variant)
    return znew, acc, cost


def nystrom_residual_mean(x, z, ell, variance=1.0, jitter=1e-8):
    """mean_i of k_ii - k_i' (K_ZZ + jitter I)^-1 k_i for the squared-exponential kernel, float64 (assertion 10's ordering)."""
    Kzz = variance * np.exp(-0.5 * sqdist(z, z, ell)) + jitter * np.eye(z.shape[0])
    Kzx = variance * np.exp(-0.5 * sqdist(z, x, ell))
    L = np.linalg.cholesky(Kzz)
    import scipy.linalg as sla

    Phi = sla.solve_triangular(L, Kzx, lower=True)
    return float(np.mean(variance - (Phi * Phi).sum(axis=0)))
