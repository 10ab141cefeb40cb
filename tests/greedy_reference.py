"""The float64 numpy yardstick of the greedy conditional-variance inducing inputs (include/agpl_greedy.h), for
tests/test_gpu_greedy.py and tests/test_greedy_reference_cpu.py: the run, the replay of a given pivot sequence and one step, each
stated once.  No GPU, no torch."""
from collections import namedtuple

import numpy as np

Case = namedtuple("Case", "id N M D kernel variance ell threshold")

# five kinds, D in {1, 3, 16}, N from 777 to about 4000, M from 40 to 300, variance != 1, per-dimension lengthscales
CASES = [
    Case("m12-n777-m40-d1", 777, 40, 1, "matern12", 1.7, (0.8,), 1e-6),
    Case("m32-n2049-m120-d3", 2049, 120, 3, "matern32", 0.6, (3.0, 6.0, 1.5), 1e-6),
    Case("m52-n3001-m300-d3", 3001, 300, 3, "matern52", 2.5, (4.5, 2.1, 3.3), 1e-6),
    Case("m12-n4001-m200-d16", 4001, 200, 16, "matern12", 1.3, tuple(2.0 + 0.25 * k for k in range(16)), 1e-6),
    Case("se-n2500-m150-d3", 2500, 150, 3, "se", 1.9, (0.9, 1.4, 0.6), 1e-6),
    Case("rq-n1500-m100-d1", 1500, 100, 1, ("rq", 1.5), 0.4, (0.5,), 1e-6),
    Case("se-n3000-m300-d1-threshold", 3000, 300, 1, "se", 1.2, (1.0,), 1e-4),  # ends by the threshold well before M
]
BY_ID = {c.id: c for c in CASES}
GAP = 1e-9            # a case qualifies for the exact-index test if the two largest residuals differ by >= GAP variance at every step after the first
THRESHOLD_MARGIN = 1e-9


def kappa(kernel, r2):
    """k / variance of the scaled squared distance, the expressions of csrc/agpl_kernel_rules.h in float64."""
    if kernel == "se":
        return np.exp(-0.5 * r2)
    if kernel in ("matern12", "exponential"):
        return np.exp(-np.sqrt(r2))
    if kernel == "matern32":
        u = 1.7320508075688772 * np.sqrt(r2)
        return (1.0 + u) * np.exp(-u)
    if kernel == "matern52":
        u = 2.23606797749979 * np.sqrt(r2)
        return (1.0 + u + u * u * (1.0 / 3.0)) * np.exp(-u)
    if isinstance(kernel, (tuple, list)) and kernel[0] == "rq":
        a = float(kernel[1])
        return np.exp(-a * np.log1p(r2 / (2.0 * a)))
    raise ValueError(kernel)


def ell_of(c):
    return np.asarray(c.ell, dtype=np.float64)


def data(c):
    """A mixture of four shifted normals, [N, D] float64."""
    rng = np.random.default_rng(9000 + 131 * c.N + 17 * c.M + c.D)
    shifts = rng.uniform(-4.0, 4.0, size=(4, c.D))
    scales = np.array([0.6, 1.0, 1.5, 0.8])
    k = rng.integers(0, 4, size=c.N)
    return shifts[k] + scales[k, None] * rng.standard_normal((c.N, c.D))


def sqdist_to(x, xp, ell):
    """r2 [N] to one point: the sum over d ascending of (x_d / ell_d - xp_d / ell_d)^2."""
    u, up = x / ell, xp / ell
    r2 = np.zeros(x.shape[0])
    for d in range(x.shape[1]):
        t = u[:, d] - up[d]
        r2 += t * t
    return r2


def gram(x, z, ell, kernel, variance):
    u, v = x / ell, z / ell
    r2 = np.zeros((x.shape[0], z.shape[0]))
    for d in range(x.shape[1]):
        t = u[:, d:d + 1] - v[None, :, d]
        r2 += t * t
    return variance * kappa(kernel, r2)


def ceil_log2(n):
    c = 0
    while (1 << c) < n:
        c += 1
    return c


def trace_shift(N_total):
    return 61 - ceil_log2(N_total)


def trace_word(d, variance, N_total):
    """The int64 a range adds into trace_acc[j]: the sum of rint(d_i / variance 2^s)."""
    return int(np.rint(np.ldexp(d / variance, trace_shift(N_total))).astype(np.int64).sum())


def step(x, ell, kernel, variance, cols, d, p, with_mag=True):
    """One step from the columns cols [j, N], the residual d [N] and the pivot p: (column j, the new d, |k| + sum_t |cols[t][i]
    cols[t][p]| -- the scale of the column's rounding error; None unless `with_mag`)."""
    k = variance * kappa(kernel, sqdist_to(x, x[p], ell))
    row = np.ascontiguousarray(cols[:, p])
    s = row @ cols                       # (any order: the yardstick's own rounding is inside every bar that uses it)
    mag = np.abs(k) + np.abs(row) @ np.abs(cols) if with_mag else None
    c = (k - s) / np.sqrt(d[p])
    dn = np.maximum(d - c * c, 0.0)
    dn[p] = 0.0
    return c, dn, mag


def replay(x, ell, kernel, variance, indices):
    """For a given pivot sequence: (the residual vector before every pick [m, N], the columns [m, N], the residual after the last)."""
    N = x.shape[0]
    d = np.full(N, float(variance))
    cols = np.zeros((len(indices), N))
    before = np.zeros((len(indices), N))
    for j, p in enumerate(indices):
        before[j] = d
        cols[j], d, _ = step(x, ell, kernel, variance, cols[:j], d, int(p), with_mag=False)
    return before, cols, d


def run(x, ell, kernel, variance, M, threshold):
    """The algorithm of include/agpl_greedy.h: dict(indices [m], max_residual [m] = max d / variance before each pick, trace [m] =
    tr(K - Q) / variance after each pick decoded from the integer sum, gaps [m] = (largest - second largest d) / variance before each
    pick, last = max d / variance after the last pick, cols [m, N], d [N])."""
    N = x.shape[0]
    d = np.full(N, float(variance))
    cols = np.zeros((M, N))
    idx, mx, tr, gaps = [], [], [], []
    for j in range(M):
        p = int(np.argmax(d))  # the first holder of the maximum
        if d[p] <= threshold * variance:
            break
        two = np.partition(d, N - 2)[N - 2:] if N > 1 else np.array([0.0, d[p]])
        gaps.append((two[1] - two[0]) / variance)
        idx.append(p)
        mx.append(d[p] / variance)
        cols[j], d, _ = step(x, ell, kernel, variance, cols[:j], d, p, with_mag=False)
        tr.append(float(trace_word(d, variance, N)) * 2.0 ** -trace_shift(N))
    m = len(idx)
    return dict(indices=np.asarray(idx, dtype=np.int64), max_residual=np.asarray(mx), trace=np.asarray(tr), gaps=np.asarray(gaps),
                last=float(d.max() / variance), cols=cols[:m], d=d)


def qualifies(r):
    """Whether the exact-index test may hold a run to its indices: the two largest residuals GAP variance apart at every step after
    the first (where every d is the variance and the lowest index wins by rule)."""
    return bool((r["gaps"][1:] >= GAP).all())


_RUNS = {}


def run_case(c):
    """run(...) of a named case, computed once and shared (treat the result as read-only)."""
    if c.id not in _RUNS:
        _RUNS[c.id] = run(data(c), ell_of(c), c.kernel, c.variance, c.M, c.threshold)
    return _RUNS[c.id]


def nystrom_residual(x, z, ell, kernel="se", variance=1.0, jitter=0.0):
    """diag(K - K_XZ (K_ZZ + jitter I)^-1 K_ZX) from a direct solve, float64 [N]."""
    Kzz = gram(z, z, ell, kernel, variance) + jitter * np.eye(z.shape[0])
    Kzx = gram(z, x, ell, kernel, variance)
    return variance - (Kzx * np.linalg.solve(Kzz, Kzx)).sum(axis=0)
