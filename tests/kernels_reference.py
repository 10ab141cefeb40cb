"""Float64 numpy reference of the stationary covariance functions a plan can be built from (include/agpl_kernels.h) and of the
whitened features Phi = L^-1 K_ZX, for tests/test_kernels_cpu.py and tests/test_gpu_kernels.py.  No GPU, no library code: nothing
here imports the package.  Conventions are KernelFunctions.jl's: r^2 = sum_d ((a_d - b_d) / ell_d)^2, k = s2 kappa(r)."""
import numpy as np

SE, MATERN12, MATERN32, MATERN52, RQ = 0, 1, 2, 3, 4
KINDS = (SE, MATERN12, MATERN32, MATERN52, RQ)
NAMES = {SE: "se", MATERN12: "matern12", MATERN32: "matern32", MATERN52: "matern52", RQ: "rq"}
RQ_ALPHA = 2.0  # the alpha the GPU cases use

# the shapes of tests/test_gpu_kernels.py: N = 300 is three 128-point tiles, the last holding 44 points; M = 37 is one k-slice short
# of a multiple of 16 and pads to 256; M = 300 pads to 512: four row blocks, the triangular skip crossing the 256 pad
# D = 1 has z on a grid, D = 3 three different lengthscales.  The variance 2.5 goes with D = 3: on the D = 1 grid the float64
# residual falls to the jitter (1.0e-8 for the squared exponential), which is >= 1e-8 s2 -- the floor tests/test_kernels_cpu.py
# checks the reference against -- for s2 = 1 only.
N = 300
SHAPES = [(37, 1, 1.0), (37, 3, 2.5), (300, 1, 1.0), (300, 3, 2.5)]  # (M, D, s2)
JITTER = 1e-8


def param_of(kind):
    return RQ_ALPHA if kind == RQ else 0.0


def python_kernel(kind):
    """The ``kernel`` argument of the ``from_inputs`` constructors for a kind."""
    return ("rq", RQ_ALPHA) if kind == RQ else NAMES[kind]


def kappa(kind, r2, param=0.0):
    """k / s2 as a function of the scaled squared distance."""
    r2 = np.asarray(r2, np.float64)
    r = np.sqrt(r2)
    if kind == SE:
        return np.exp(-0.5 * r2)
    if kind == MATERN12:
        return np.exp(-r)
    if kind == MATERN32:
        return (1.0 + np.sqrt(3.0) * r) * np.exp(-np.sqrt(3.0) * r)
    if kind == MATERN52:
        return (1.0 + np.sqrt(5.0) * r + 5.0 * r2 / 3.0) * np.exp(-np.sqrt(5.0) * r)
    if kind == RQ:
        return (1.0 + r2 / (2.0 * param)) ** (-param)
    raise ValueError(kind)


def kernel(kind, a, b, ell, s2, param=0.0):
    """K [len(a), len(b)] float64; a [n, D], b [m, D], ell [D]."""
    d = (np.asarray(a, np.float64)[:, None, :] - np.asarray(b, np.float64)[None, :, :]) / np.asarray(ell, np.float64)
    return s2 * kappa(kind, (d * d).sum(-1), param)


def phi_f64(kind, x, z, ell, s2, jitter, param=0.0):
    """Phi [N, M] = (L^-1 K_ZX)' and the residual s2 - |phi|^2 in float64 (numpy), and L^-1 (phi_f64 of
    tests/test_gpu_plan_inputs.py for any kind)."""
    Kzz = kernel(kind, z, z, ell, s2, param) + jitter * np.eye(len(z))
    Lc = np.linalg.cholesky(Kzz)
    Linv = np.linalg.solve(Lc, np.eye(len(z)))
    Phi = (Linv @ kernel(kind, z, x, ell, s2, param)).T
    return Phi, np.maximum(s2 - (Phi * Phi).sum(1), 0.0), Linv


def workload(N, M, D, seed=3):
    """The recipe of tests/test_gpu_plan_inputs.py::workload, restated (tests/test_gpu_kernels.py checks that they agree)."""
    rng = np.random.default_rng(seed)
    x = rng.uniform(-10, 10, size=(N, D))
    if D == 1:
        z = np.linspace(-10, 10, M)[:, None]
        ell = np.array([1.5 * 20 / (M - 1)])
    else:
        z = rng.uniform(-10, 10, size=(M, D))
        ell = np.array([1.0, 1.4, 1.8][:D]) if D <= 3 else np.full(D, 12.0)
    return x, z, ell
