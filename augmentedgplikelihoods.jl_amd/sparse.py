"""Sparse sweep drivers: the reference's user-level loops (``cavi!`` examples/bernoulli/script.jl:29-39,
multi-latent examples/categorical/script.jl:64-77, ``gibbs_sample`` :76-87) restated in the sparse form the
docs give only as a formula (docs/src/index.md:154-163), in the whitened feature basis

    Phi = L^-1 K_ZX  (K_Z = L L'),   u = L v,   q(v) = N(m, S),
    S = (I + G)^-1,  m = S g,        G = Phi Diag(gamma) Phi',  g = Phi beta,
    q(f_i) = N(phi_i' m, d_i + phi_i' S phi_i),   d_i = k_ii - |phi_i|^2.

All O(N) work is two MFMA passes over Phi per sweep (agpl_cavi_pass) plus an M x M update
(agpl_gaussian_update).  N is sharded over ranks with one all-reduce of (G, g) per sweep.
"""
from __future__ import annotations

import ctypes as C
import dataclasses

import numpy as np

from . import _ffi
from .operators import Context, _prep, _prep_y, _ptr, _torch, default_context

PAD = 128  # feature rows are padded to a multiple of the MFMA block


def padded(M: int) -> int:
    return (M + PAD - 1) // PAD * PAD


def _dist():
    import torch.distributed as dist

    return dist


def _all_reduce_sum(t, group):
    """Sum ``t`` over the ranks of ``group``, in place; nothing to do without a group."""
    if group is not None:
        dist = _dist()
        dist.all_reduce(t, op=dist.ReduceOp.SUM, group=group)


def _lengthscales(lengthscale, D: int):
    """``lengthscale``, a number or D numbers, as a float64 host tensor [D]."""
    torch = _torch()
    if not 1 <= D <= 16:
        raise _ffi.ArgumentError(-1, f"the input dimension must be 1 ... 16 (got {D})")
    ell = torch.as_tensor(lengthscale, dtype=torch.float64).reshape(-1).cpu()
    if ell.numel() == 1 and D > 1:
        ell = ell.expand(D)
    if ell.numel() != D:
        raise _ffi.ArgumentError(-1, f"{ell.numel()} lengthscales for D = {D} inputs")
    if not bool(torch.isfinite(ell).all()) or not bool((ell > 0).all()):
        raise _ffi.ArgumentError(-1, f"lengthscales must be positive and finite (got {ell.tolist()})")
    return ell


def _check_variance(variance):
    if not (np.isfinite(variance) and variance > 0):
        raise _ffi.ArgumentError(-1, f"variance must be positive and finite (got {variance})")


def _check_jitter(jitter):
    if not (np.isfinite(jitter) and jitter >= 0):
        raise _ffi.ArgumentError(-1, f"jitter must be >= 0 and finite (got {jitter})")


def _point_major(mu, var, L: int):
    """(mu, var) float32 [L][N] in the layout of the float64 operators: float64 [N] (one latent) or [N, L]."""
    torch = _torch()
    if L == 1:
        return mu[0].to(torch.float64), var[0].to(torch.float64)
    return mu.t().contiguous().to(torch.float64), var.t().contiguous().to(torch.float64)


def _mu0_at(mu0_s, L: int, Ns: int):
    """The prior mean at Ns new inputs as the kernels read it: float32, L Ns numbers (or None)."""
    mu0_s = _prep(mu0_s, _torch().float32, "mu0_s")
    if mu0_s is not None and mu0_s.numel() != L * Ns:
        raise _ffi.ArgumentError(-1, f"mu0_s must be [{L}, {Ns}] (got {tuple(mu0_s.shape)})")
    return mu0_s


def _check_sites(L: int, N: int, **sites):
    """Per-point site tensors [L][N] by name; only ``mu0`` may be absent."""
    for n, t in sites.items():
        if (t is None and n != "mu0") or (t is not None and t.numel() != L * N):
            raise _ffi.ArgumentError(-1, f"{n} must be [{L}, {N}]")


def _adam_step(par, grad, m1, m2, it: int, step):
    """One Adam ascent step (beta 0.9 / 0.999, eps 1e-8), the ``it``-th (1-based): ``(par, m1, m2)``."""
    m1, m2 = 0.9 * m1 + 0.1 * grad, 0.999 * m2 + 0.001 * grad * grad
    return par + step * (m1 / (1 - 0.9 ** it)) / ((m2 / (1 - 0.999 ** it)).sqrt() + 1e-8), m1, m2


def synth_xy(lik, seed: int, i0: int, n: int, ctx: Context | None = None, want_x: bool = True):
    """Synthetic workload of SURVEY.md 8(d): x_i = -10 + 20 u_i, y_i ~ lik(f*(x_i)), pure function of
    (seed, i0 + i).  Real-valued y comes back as float32 (the fused pass's element type)."""
    if lik.ykind == "i32x2":
        raise _ffi.ArgumentError(-1, "synth_xy does not generate per-point trial counts: draw trials yourself and sample y with "
                                     "BinomialLikelihood per group, or build the observation with binomial_obs")
    torch = _torch()
    ctx = ctx or default_context()
    L = lik._nlatent
    x = torch.empty(n, dtype=torch.float64, device=ctx.device) if want_x else None
    ydt = {"u8": torch.uint8, "i32": torch.int32, "real": torch.float32}[lik.ykind]
    y = torch.empty((n,) if L == 1 else (n, L), dtype=ydt, device=ctx.device)
    d = lik.desc()
    ctx.call("agpl_synth_xy", C.byref(d), C.c_uint64(seed), C.c_int64(i0), C.c_int64(n), _ptr(x), _ptr(y))
    return x, y


def se_features(x, z, ell: float, ctx: Context | None = None, out=None):
    """K_ZX for the squared-exponential kernel with lengthscale ``ell`` (examples/bernoulli/script.jl:15):
    float32 [N, Mp] (= [Mp, N] column-major), rows M..Mp zero."""
    torch = _torch()
    ctx = ctx or default_context()
    x = _prep(x, torch.float64, "x")
    z = _prep(z, torch.float64, "z")
    N, M = x.numel(), z.numel()
    Mp = padded(M)
    if out is None:
        out = torch.empty((N, Mp), dtype=torch.float32, device=x.device)
    ctx.call("agpl_se_features", C.c_int64(N), C.c_int32(M), C.c_int32(Mp), _ptr(x), _ptr(z), C.c_double(ell),
             _ptr(out))
    return out


def whitening_matrix(Kzz: np.ndarray, jitter: float = 0.0):
    """Host float64 setup (M x M, once): L = chol(K_Z + jitter I) (``_chol_cov`` of
    examples/bernoulli/script.jl:30 with the 1e-8 of :44) and L^-1."""
    Kzz = np.asarray(Kzz, dtype=np.float64)
    Lc = np.linalg.cholesky(Kzz + jitter * np.eye(Kzz.shape[0]))
    import scipy.linalg as sla

    Linv = sla.solve_triangular(Lc, np.eye(Kzz.shape[0]), lower=True)
    return Lc, Linv


def whiten_features(Kzx, Linv: np.ndarray, ctx: Context | None = None, out=None):
    """Phi = L^-1 K_ZX on the matrix cores (agpl_transform_features).  Kzx: float32 [N, Mp]."""
    torch = _torch()
    ctx = ctx or default_context()
    Kzx = _prep(Kzx, torch.float32, "Kzx")
    N, Mp = Kzx.shape
    M = Linv.shape[0]
    A = np.zeros((Mp, Mp), dtype=np.float32)
    A[:M, :M] = Linv
    At = torch.from_numpy(np.ascontiguousarray(A.T)).to(Kzx.device)  # column-major A
    if out is None:
        out = torch.empty_like(Kzx)
    ctx.call("agpl_transform_features", C.c_int64(N), C.c_int32(Mp), _ptr(At), _ptr(Kzx), _ptr(out))
    return out


def shard_range(N: int, rank: int, world: int):
    """Points [i0, i1) owned by ``rank`` when N observations are sharded over ``world`` ranks:
    contiguous, sizes differ by at most one, a pure function of (N, rank, world)."""
    return rank * N // world, (rank + 1) * N // world


def natural_parameter_buffers(L, M, device, extra=0):
    """(flat, G, g): G [L, M, M] and g [L, M] float64 as views of ONE flat buffer, so that the exchange step of a
    sweep is a single collective of L (M^2 + M) doubles.  ``extra`` more doubles ride at its end (the ELBO terms of a sweep
    are summed over ranks by the same collective)."""
    torch = _torch()
    flat = torch.zeros(L * M * M + L * M + extra, dtype=torch.float64, device=device)
    return flat, flat[: L * M * M].view(L, M, M), flat[L * M * M: L * M * M + L * M].view(L, M)


def plan_padded(M: int) -> int:
    """The feature count a plan works on: M rounded up to a multiple of 256 (include/agpl.h: the state arrays of agpl_plan_state
    are sized by it; the images carry zero features beyond M)."""
    return (M + 255) // 256 * 256


_KERNEL_KINDS = {"se": _ffi.KERNEL_SE, "matern12": _ffi.KERNEL_MATERN12, "exponential": _ffi.KERNEL_MATERN12,
                 "matern32": _ffi.KERNEL_MATERN32, "matern52": _ffi.KERNEL_MATERN52}
_KERNEL_NAMES = {_ffi.KERNEL_SE: "se", _ffi.KERNEL_MATERN12: "matern12", _ffi.KERNEL_MATERN32: "matern32",
                 _ffi.KERNEL_MATERN52: "matern52", _ffi.KERNEL_RQ: "rq", _ffi.KERNEL_PERIODIC: "periodic",
                 _ffi.KERNEL_SE_PERIODIC: "se_periodic", _ffi.KERNEL_SE_COSINE: "se_cosine"}
# the kinds that carry a parameter: (kind, what the refusal names)
_KERNEL_PARAMS = {"rq": (_ffi.KERNEL_RQ, "alpha of the rational quadratic kernel"),
                  "periodic": (_ffi.KERNEL_PERIODIC, "the period p of the periodic kernel"),
                  "se_periodic": (_ffi.KERNEL_SE_PERIODIC, "the period p of the squared exponential x periodic kernel"),
                  "se_cosine": (_ffi.KERNEL_SE_COSINE, "the period p of the squared exponential x cosine kernel")}


def kernel_dim_warped(kind: int, d: int, D: int) -> bool:
    """Whether ``kind`` warps dimension ``d`` of ``D``, the host's copy of the rule of csrc/agpl_kernel_rules.h (the one place on
    this side that names the warped kinds): the periodic kind every dimension, the squared exponential x periodic kind the last
    one, any other kind none."""
    return kind == _ffi.KERNEL_PERIODIC or (kind == _ffi.KERNEL_SE_PERIODIC and d == D - 1)


# the kinds whose distance is warped in some dimension: derived from the predicate, as kernel_kind_warps is in C++
_KERNEL_WARPED = tuple(k for k in _KERNEL_NAMES if any(kernel_dim_warped(k, d, 16) for d in range(16)))


def kernel_dim_modulated(kind: int, d: int, D: int) -> bool:
    """Whether ``kind`` multiplies the squared exponential by a factor of dimension ``d`` of ``D`` that is no function of r^2, the
    host's copy of the rule of csrc/agpl_kernel_rules.h (the one place on this side that names such kinds): the squared exponential
    x cosine kind the last one, cos(2 pi (x_d - x'_d) / p); any other kind none."""
    return kind == _ffi.KERNEL_SE_COSINE and d == D - 1


# the kinds with such a factor: derived from the predicate, as kernel_kind_modulated is in C++
_KERNEL_MODULATED = tuple(k for k in _KERNEL_NAMES if any(kernel_dim_modulated(k, d, 16) for d in range(16)))


def kernel_kind(kernel):
    """``(kind, param)`` of include/agpl_kernels.h for the ``kernel`` argument of the ``from_inputs`` constructors: ``"se"``,
    ``"matern12"`` (alias ``"exponential"``), ``"matern32"``, ``"matern52"``, ``("rq", alpha)``, ``("periodic", p)`` (the period,
    one scalar for all dimensions), ``("se_periodic", p)`` (squared exponential in the leading dimensions, periodic with period p
    in the last) or ``("se_cosine", p)`` (squared exponential in every dimension times cos(2 pi (x_D - x'_D) / p) in the last: the one
    kind that takes negative values).  Anything else is an ``ArgumentError`` (raised before any device work)."""
    if isinstance(kernel, str) and kernel in _KERNEL_KINDS:
        return _KERNEL_KINDS[kernel], 0.0
    if isinstance(kernel, (tuple, list)) and len(kernel) == 2 and isinstance(kernel[0], str) and kernel[0] in _KERNEL_PARAMS:
        kind, what = _KERNEL_PARAMS[kernel[0]]
        try:
            param = float(kernel[1])
        except (TypeError, ValueError):
            param = float("nan")
        if not (np.isfinite(param) and param > 0):
            raise _ffi.ArgumentError(-1, f"{what} must be positive and finite (got {kernel[1]!r})")
        return kind, param
    raise _ffi.ArgumentError(-1, f'kernel must be "se", "matern12" ("exponential"), "matern32", "matern52", ("rq", alpha), '
                                 f'("periodic", p), ("se_periodic", p) or ("se_cosine", p) (got {kernel!r})')


MAX_PATH_FEATURES = 8192  # agpl_plan_sample_paths: 1 <= F <= 8192


def periodic_spectral_weights(lengthscale: float):
    """The spectral measure of one dimension of the periodic kernel, which is discrete: with a = 1 / (4 ell^2),

        exp(-sin^2(pi delta / p) / (2 ell^2)) = sum_{k in Z} e^-a I_k(a) cos(2 pi k delta / p),

    returned as w [K + 1] float64 with w[k] = e^-a I_k(a) for k = 0 ... K (the weight of -k is w[k]), truncated where the two-sided tail
    mass is below 1e-16, so w[0] + 2 sum_{k >= 1} w[k] = 1.  Formed on the host in float64 by the ratio recurrence: the ratios
    r_k = I_k / I_{k-1} downward from a start far in the tail (Miller), r_k = 1 / (2 k / a + r_{k+1}), then the products upward and
    the normalisation by the sum, which never forms e^-a or I_k themselves (neither overflows nor underflows for any ell > 0)."""
    a = 1.0 / (4.0 * float(lengthscale) ** 2)
    if not (np.isfinite(a) and a > 0):
        raise _ffi.ArgumentError(-1, f"lengthscale must be positive and finite (got {lengthscale!r})")
    K = int(a + 12.0 * np.sqrt(a + 1.0)) + 40  # far beyond the mode's width sqrt(a): the start's error has decayed to nothing at k <= K / 2
    r = np.zeros(2 * K + 2)
    for k in range(2 * K, 0, -1):
        r[k] = 1.0 / (2.0 * k / a + r[k + 1])
    logw = np.concatenate(([0.0], np.cumsum(np.log(r[1:K + 1]))))
    w = np.exp(logw)
    w /= w[0] + 2.0 * w[1:].sum()
    tail = 2.0 * np.cumsum(w[::-1])[::-1]  # tail[k] = mass of |j| >= k
    keep = max(1, int(np.searchsorted(-tail, -1e-16)))  # first k whose tail mass is below 1e-16
    w = w[:keep]
    return w / (w[0] + 2.0 * w[1:].sum())


def spectral_frequencies(kernel, F: int, D: int, generator=None, device=None, lengthscale=None):
    """Random Fourier frequencies of a stationary kernel's spectral measure, in the scaled units u = x / ell, for
    ``Plan.sample_paths`` / agpl_plan_sample_paths (include/agpl_pathwise.h states the same rule for C and Julia callers):
    ``(omega [F, D], phase [F])`` float64, with n ~ N(0, I_D) and phase ~ U[0, 2 pi),

        "se": omega = n;   Matern-nu (nu = 1/2, 3/2, 5/2): omega = n sqrt(2 nu / c), c ~ chi^2(2 nu);
        ("rq", alpha): omega = n sqrt(tau), tau ~ Gamma(shape alpha, scale 1 / alpha),
        ("periodic", p): omega_d = 2 pi k_d ell_d / p, the integer k_d drawn with probability e^-a I_|k|(a), a = 1 / (4 ell_d^2)
        (``periodic_spectral_weights``); the periodic kinds alone need ``lengthscale`` (a scalar or [D]; the others ignore it),
        ("se_periodic", p): the first D - 1 columns as for "se", the last as for ("periodic", p) with ell_{D-1},
        ("se_cosine", p): omega = n, then the last column shifted by +-2 pi ell_{D-1} / p with a fair sign per feature (the squared
        exponential's Gaussian moved to the two frequencies of the cosine; drawn after the normals, before the phase; needs
        ``lengthscale`` too), so that E cos(omega . du) = exp(-|du|^2 / 2) cos(2 pi ell_{D-1} du_{D-1} / p),

    so that E cos(omega . (u - u')) = kappa(|u - u'|).  ``kernel`` as for the ``from_inputs`` constructors (``kernel_kind``).
    Drawn with ``torch`` on ``device`` (default: the generator's device, else the current CUDA device)."""
    torch = _torch()
    kind, kparam = kernel_kind(kernel)
    if not 1 <= int(F) <= MAX_PATH_FEATURES:
        raise _ffi.ArgumentError(-1, f"the number of features must be 1 ... {MAX_PATH_FEATURES} (got {F})")
    if not 1 <= int(D) <= 16:
        raise _ffi.ArgumentError(-1, f"the input dimension must be 1 ... 16 (got {D})")
    F, D = int(F), int(D)
    if device is None:
        device = generator.device if generator is not None else torch.device("cuda", torch.cuda.current_device())
    kw = dict(dtype=torch.float64, device=device, generator=generator)
    if kind in _KERNEL_WARPED:
        if lengthscale is None:
            raise _ffi.ArgumentError(-1, "the periodic kernel's spectral measure depends on the lengthscales: pass lengthscale=")
        ell = _lengthscales(lengthscale, D).numpy()
        nlead = sum(not kernel_dim_warped(kind, d, D) for d in range(D))  # the squared exponential's dimensions: omega_d = n
        n = torch.randn((F, nlead), **kw) if nlead else None
        cols, j = [], 0
        for d in range(D):  # k_d by inversion of the two-sided distribution function, one uniform per (feature, warped dimension)
            if not kernel_dim_warped(kind, d, D):
                cols.append(n[:, j])
                j += 1
                continue
            w = periodic_spectral_weights(ell[d])
            two = np.concatenate((w[:0:-1], w))  # k = -K ... K
            cdf = torch.as_tensor(np.cumsum(two), dtype=torch.float64, device=device)
            u = torch.rand(F, **kw)
            k = torch.searchsorted(cdf, u).clamp_(max=len(two) - 1) - (len(w) - 1)
            cols.append(k.to(torch.float64) * (2.0 * np.pi * ell[d] / kparam))
        phase = torch.rand(F, **kw) * (2.0 * np.pi)
        return torch.stack(cols, 1).contiguous(), phase
    n = torch.randn((F, D), **kw)
    if kind in _KERNEL_MODULATED:
        if lengthscale is None:
            raise _ffi.ArgumentError(-1, "the squared exponential x cosine kernel's spectral measure depends on the lengthscales: "
                                         "pass lengthscale=")
        ell = _lengthscales(lengthscale, D).numpy()
        sign = torch.where(torch.rand(F, **kw) < 0.5, -1.0, 1.0).to(torch.float64)
        for d in range(D):
            if kernel_dim_modulated(kind, d, D):
                n[:, d] += sign * (2.0 * np.pi * ell[d] / kparam)
    phase = torch.rand(F, **kw) * (2.0 * np.pi)
    twonu = {_ffi.KERNEL_MATERN12: 1, _ffi.KERNEL_MATERN32: 3, _ffi.KERNEL_MATERN52: 5}.get(kind)
    if twonu is not None:
        c = (torch.randn((F, twonu), **kw) ** 2).sum(1)
        n = n * torch.sqrt(twonu / c).unsqueeze(1)
    elif kind == _ffi.KERNEL_RQ:
        tau = torch._standard_gamma(torch.full((F,), kparam, dtype=torch.float64, device=device), generator=generator) / kparam
        n = n * torch.sqrt(tau).unsqueeze(1)
    return n.contiguous(), phase


class Paths:
    """Pathwise (Matheron-rule) draws of the posterior function of a plan made by ``from_inputs`` (agpl_plan_sample_paths,
    include/agpl_pathwise.h): T functions f_t = mu0 + prior draw + phi' (V_t - L^-1 up_t), the prior draw a sum of ``nfeatures``
    random Fourier features.  The object holds ``omega`` [F, D], ``phase`` [F], ``W`` [T, L, F], ``Xi`` [T, L, M] and ``V`` [T, L, M]
    on the device and the plan; calling it evaluates the SAME functions at any inputs, any number of times:
    ``paths(x_s, mu0_s=None)`` -> float32 [T, L, Ns].  A value depends on its input (and the draw) alone, so evaluations at
    different sets of inputs are coherent.  The cost per point is O((M + F) T L): no Ns x Ns matrix is formed."""

    def __init__(self, plan, V, omega, phase, W, Xi):
        self.plan, self.V, self.omega, self.phase, self.W, self.Xi = plan, V, omega, phase, W, Xi
        self.T, self.L, self.F = int(V.shape[0]), plan.L, int(omega.shape[0])

    def __call__(self, x_s, mu0_s=None):
        torch = _torch()
        plan = self.plan
        x_s = plan._inputs_at(x_s, "x_s", "Paths")
        Ns = int(x_s.shape[0])
        mu0_s = _mu0_at(mu0_s, self.L, Ns)
        out = torch.empty((self.T, self.L, Ns), dtype=torch.float32, device=x_s.device)
        plan.call("agpl_plan_sample_paths", C.c_int32(self.T), _ptr(self.V), C.c_int32(self.F), _ptr(self.omega), _ptr(self.phase),
                  _ptr(self.W), _ptr(self.Xi), C.c_int64(Ns), _ptr(x_s), _ptr(mu0_s), _ptr(out), lib=_ffi.pathwise_lib())
        return out

    _Y_CHUNK = 1 << 15  # points per step of sample_y (T L float32 function values per point)

    def sample_y(self, lik, x_s, mu0_s=None, sweep: int | None = None):
        """One draw of the observable per path and input: ``operators.sample_y`` of ``self(x_s)``, evaluated ``_Y_CHUNK`` points at a
        time (no [T, L, Ns] block of function values is held) with ``point0`` = the chunk's start, so the result does not depend on
        the chunking: uint8 / int32 / float64 [T, Ns], one-hot uint8 [T, Ns, L] for the categorical kinds.  Draw t of input i uses
        the stream (seed, point_offset + i, sweep, t); ``sweep`` None takes the context's next draw counter."""
        from . import operators as ops

        torch = _torch()
        plan = self.plan
        if lik._nlatent != self.L:
            raise _ffi.ArgumentError(-1, f"the likelihood has {lik._nlatent} latents, the paths {self.L}")
        x_s = plan._inputs_at(x_s, "x_s", "Paths.sample_y")
        Ns = int(x_s.shape[0])
        mu0_s = _mu0_at(mu0_s, self.L, Ns)
        if mu0_s is not None:
            mu0_s = mu0_s.reshape(self.L, Ns)
        if sweep is None:
            sweep = plan.ctx.next_sweep()
        cat = lik.kind in (ops.KIND_CATEGORICAL, ops.KIND_CATEGORICAL_BIJ)
        out = torch.empty((self.T, Ns, self.L) if cat else (self.T, Ns), dtype=ops._ydtype(lik, torch.float64), device=x_s.device)
        for c0 in range(0, Ns, self._Y_CHUNK):
            c1 = min(Ns, c0 + self._Y_CHUNK)
            F = self(x_s[c0:c1], None if mu0_s is None else mu0_s[:, c0:c1].contiguous())
            out[:, c0:c1] = ops.sample_y(lik, F, point0=c0, sweep=sweep, ctx=plan.ctx)
        return out


def kmeans_quanta(bound: float, N_total: int, D: int):
    """``(sx, sd)``: the exponents of the fixed-point rule of include/agpl_inducing.h (agpl_kmeans_quanta; a pure host function):
    a scaled coordinate is summed as ``rint(u 2^sx)``, a squared distance as ``rint(min(r2, 4 D bound^2) 2^sd)``."""
    sx, sd = C.c_int32(), C.c_int32()
    rc = _ffi.inducing_lib().agpl_kmeans_quanta(None, bound, N_total, D, C.byref(sx), C.byref(sd))
    if rc:
        raise _ffi.ArgumentError(rc, f"bound must be positive and finite, 1 <= N_total < 2^48, 1 <= D <= 16 (got {bound}, {N_total}, {D})")
    return sx.value, sd.value


def select_inducing(x, M: int, lengthscale=1.0, niter: int = 10, z0=None, ctx: Context | None = None, group=None,
                    return_info: bool = False, kernel=None):
    """Inducing inputs from the data: M centres of Lloyd's k-means over x [N] or [N, D] (float64 CUDA tensor) in the kernel's
    metric x / lengthscale, from a stratified start (or ``z0`` [M, D]) -- z [M, D] float64 on the device, ready for every
    ``from_inputs`` (include/agpl_inducing.h; KmeansAlg of InducingPoints.jl).  The centres are sums of INTEGERS (fixed point):
    with ``group`` (``x`` = this rank's shard of ``shard_range``; bound by all_reduce(MAX), start rows and accumulators by
    all_reduce(SUM), every rank forming the centres itself) each rank ends with the bits of the one-process call.
    ``return_info``: also ``{"empty", "movement", "cost"}`` (empty centres of the final assignment, largest movement of a centre
    in the last update, sum of squared scaled distances).  ``kernel`` (optional, as for ``from_inputs``) only checks that this
    metric is the kernel's: the periodic kernels' (``("periodic", p)``, ``("se_periodic", p)``) is not, so it is refused (``AGPLError``, unsupported) in favour of
    ``select_inducing_greedy``; so is ``("se_cosine", p)``, whose k changes sign within a cluster of that metric."""
    torch = _torch()
    if kernel is not None and kernel_kind(kernel)[0] in _KERNEL_MODULATED:
        raise _ffi.AGPLError(_ffi.ERR_UNSUPPORTED, "k-means works in the Euclidean metric x / lengthscale, which does not see the "
                                                   "cosine factor of the squared exponential x cosine kernel: use select_inducing_greedy")
    if kernel is not None and kernel_kind(kernel)[0] in _KERNEL_WARPED:
        raise _ffi.AGPLError(_ffi.ERR_UNSUPPORTED, "k-means works in the Euclidean metric x / lengthscale, which is not the periodic "
                                                   "kernel's: use select_inducing_greedy")
    if not isinstance(M, (int, np.integer)) or isinstance(M, bool) or not 1 <= M <= 2048:
        raise _ffi.ArgumentError(-1, f"M must be an integer in 1 ... 2048 (got {M!r})")
    if not isinstance(niter, (int, np.integer)) or isinstance(niter, bool) or niter < 0:
        raise _ffi.ArgumentError(-1, f"niter must be an integer >= 0 (got {niter!r})")
    x = _prep(x, torch.float64, "x")
    if x.dim() == 1:
        x = x.unsqueeze(1)
    if x.dim() != 2:
        raise _ffi.ArgumentError(-1, f"x must be [N] or [N, D] (got {tuple(x.shape)})")
    n, D = int(x.shape[0]), int(x.shape[1])
    ell = _lengthscales(lengthscale, D).contiguous().numpy()
    ellp = ell.ctypes.data_as(C.c_void_p)
    if z0 is not None:
        z0 = _prep(z0, torch.float64, "z0")
        if z0.dim() == 1:
            z0 = z0.unsqueeze(1)
        if tuple(z0.shape) != (M, D):
            raise _ffi.ArgumentError(-1, f"z0 must be [{M}, {D}] (got {tuple(z0.shape)})")
    ctx = ctx or default_context()
    lib = _ffi.inducing_lib()
    z = torch.empty((M, D), dtype=torch.float64, device=x.device)
    info = torch.zeros(3, dtype=torch.float64, device=x.device)

    def result():
        if not return_info:
            return z
        h = info.cpu().tolist()
        return z, {"empty": int(h[0]), "movement": h[1], "cost": h[2]}

    if group is None:
        if M > n:
            raise _ffi.ArgumentError(-1, f"M = {M} centres need at least as many points (got {n})")
        h = ctx.bind()
        _ffi.check(h, lib.agpl_select_inducing_kmeans(h, n, M, D, x.data_ptr(), ellp, int(niter), _ptr(z0), z.data_ptr(),
                                                       info.data_ptr()))
        return result()

    dist = _dist()
    # the shard's place among all points: the sizes of the ranks before it (shard_range gives exactly these)
    rank, world = dist.get_rank(group), dist.get_world_size(group)
    sizes = torch.zeros(world, dtype=torch.int64, device=x.device)
    sizes[rank] = n
    dist.all_reduce(sizes, op=dist.ReduceOp.SUM, group=group)
    sizes = sizes.cpu().tolist()
    N_total, i0 = int(sum(sizes)), int(sum(sizes[:rank]))
    if M > N_total:
        raise _ffi.ArgumentError(-1, f"M = {M} centres need at least as many points (got {N_total})")
    h = ctx.bind()
    b = torch.zeros(1, dtype=torch.float64, device=x.device)
    _ffi.check(h, lib.agpl_kmeans_bound(h, n, D, _ptr(x if n else None), ellp, b.data_ptr()))
    dist.all_reduce(b, op=dist.ReduceOp.MAX, group=group)
    bound = float(b.item())
    bound = bound if bound > 0.0 else 1.0  # an all-zero x (the convenience call's rule)
    if z0 is None:
        _ffi.check(h, lib.agpl_kmeans_seed(h, N_total, i0, n, M, D, _ptr(x if n else None), z.data_ptr(), None))
        dist.all_reduce(z, op=dist.ReduceOp.SUM, group=group)  # every row has one owner, the others add zeros: exact
    else:
        z.copy_(z0)
    acc = torch.empty((M, D + 2), dtype=torch.int64, device=x.device)
    flag = torch.zeros(1, dtype=torch.int32, device=x.device)
    for it in range(int(niter) + 1):  # the last round is the step for the final cost alone
        acc.zero_()
        err = None
        try:
            _ffi.check(h, lib.agpl_kmeans_step(h, N_total, n, M, D, _ptr(x if n else None), ellp, z.data_ptr(), bound,
                                               acc.data_ptr(), None))
        except _ffi.AGPLError as e:
            err = e
        if it == 0:  # x does not change and z is the same on every rank: a refusal shows in the first step, on all ranks together
            flag.fill_(0 if err is None else 1)
            dist.all_reduce(flag, op=dist.ReduceOp.MAX, group=group)
            if err is None and int(flag.item()):
                raise _ffi.DomainError(_ffi.ERR_DOMAIN, "another rank's shard was refused (a non-finite input?)")
        if err is not None:
            raise err
        dist.all_reduce(acc, op=dist.ReduceOp.SUM, group=group)  # int64: the sum is exact, whatever the order
        if it < niter:
            _ffi.check(h, lib.agpl_kmeans_centres(h, N_total, M, D, ellp, bound, acc.data_ptr(), z.data_ptr(), info.data_ptr()))
        else:  # the final step: its cost and empty count, the movement of the last update (the convenience call's info)
            sd = kmeans_quanta(bound, N_total, D)[1]
            info[0] = float((acc[:, 0] == 0).sum().item())
            info[2] = float(np.ldexp(float(int(acc[:, D + 1].sum().item())), -sd))
    return result()


def select_inducing_greedy(x, M: int, lengthscale=1.0, variance: float = 1.0, kernel="se", threshold: float = 1e-6,
                           ctx: Context | None = None, group=None, return_info: bool = False):
    """Inducing inputs from the data by greedy conditional variance -- the partial pivoted Cholesky of K_XX (include/agpl_greedy.h;
    Burt, Rasmussen, van der Wilk 2020): repeatedly the point of x [N] or [N, D] (float64 CUDA tensor) whose prior variance given the
    inputs chosen so far is largest, until M are chosen or that variance is at most ``threshold * variance``.  Returns ``z[:m]``,
    float64 [m, D] on the device, ready for every ``from_inputs``; m <= M is the answer to "how many inducing inputs are needed".  The
    default threshold 1e-6 is the jitter scale plans are built at: an input whose conditional variance is below it adds nothing a plan
    can resolve.  ``kernel`` as for the ``from_inputs`` constructors (``kernel_kind``).  No floating-point sum crosses a point, so with
    ``group`` (``x`` = this rank's shard of ``shard_range``; per step MAX / MIN of the candidate record and SUM of the pivot record,
    the integer trace summed once at the end) every rank ends with the bits of the one-process call.
    ``return_info``: also ``{"selected": m, "indices": int64 [m] (host), "max_residual": [m] max d / variance before each pick
    (non-increasing), "trace": [m] tr(K - Q) / variance after each pick}``."""
    torch = _torch()
    if not isinstance(M, (int, np.integer)) or isinstance(M, bool) or not 1 <= M <= 2048:
        raise _ffi.ArgumentError(-1, f"M must be an integer in 1 ... 2048 (got {M!r})")
    kind, kparam = kernel_kind(kernel)
    x = _prep(x, torch.float64, "x")
    if x.dim() == 1:
        x = x.unsqueeze(1)
    if x.dim() != 2:
        raise _ffi.ArgumentError(-1, f"x must be [N] or [N, D] (got {tuple(x.shape)})")
    n, D = int(x.shape[0]), int(x.shape[1])
    ell = _lengthscales(lengthscale, D).contiguous().numpy()
    ellp = ell.ctypes.data_as(C.c_void_p)
    variance, threshold = float(variance), float(threshold)
    _check_variance(variance)
    if not 1e-12 <= threshold < 1.0:
        raise _ffi.ArgumentError(-1, f"threshold must be in [1e-12, 1) (got {threshold})")
    ctx = ctx or default_context()
    lib = _ffi.greedy_lib()
    nbytes = C.c_int64()
    if lib.agpl_greedy_bytes(n, M, C.byref(nbytes)):
        raise _ffi.ArgumentError(-1, f"no work area for n = {n} points and M = {M}")
    work = torch.empty(nbytes.value // 8, dtype=torch.int64, device=x.device)
    z = torch.zeros((M, D), dtype=torch.float64, device=x.device)

    def result(m, idx, maxres, trace):
        if not return_info:
            return z[:m]
        return z[:m], {"selected": m, "indices": np.asarray(idx[:m], dtype=np.int64), "max_residual": np.asarray(maxres[:m], dtype=np.float64),
                       "trace": np.asarray(trace[:m], dtype=np.float64)}

    if group is None:
        if n < 1:
            raise _ffi.ArgumentError(-1, "x has no points")
        idx = torch.empty(M, dtype=torch.int64, device=x.device)
        info = torch.empty(1 + 2 * M, dtype=torch.float64, device=x.device)
        h = ctx.bind()
        _ffi.check(h, lib.agpl_select_inducing_greedy(h, n, M, D, kind, kparam, x.data_ptr(), ellp, variance, threshold, work.data_ptr(),
                                                      nbytes.value, z.data_ptr(), idx.data_ptr(), info.data_ptr()))
        info = info.cpu().numpy()
        return result(int(info[0]), idx.cpu().numpy(), info[1:1 + M], info[1 + M:])

    dist = _dist()
    rank, world = dist.get_rank(group), dist.get_world_size(group)
    sizes = torch.zeros(world, dtype=torch.int64, device=x.device)
    sizes[rank] = n
    dist.all_reduce(sizes, op=dist.ReduceOp.SUM, group=group)
    sizes = sizes.cpu().tolist()
    N_total, i0 = int(sum(sizes)), int(sum(sizes[:rank]))
    if N_total < 1:
        raise _ffi.ArgumentError(-1, "x has no points")
    h = ctx.bind()
    xp = _ptr(x if n else None)
    wp, wb = work.data_ptr(), nbytes.value
    cand = torch.zeros(2, dtype=torch.int64, device=x.device)
    err = None
    try:
        _ffi.check(h, lib.agpl_greedy_begin(h, N_total, i0, n, M, D, xp, variance, wp, wb, cand.data_ptr()))
    except _ffi.AGPLError as e:
        err = e
    flag = torch.full((1,), 0 if err is None else 1, dtype=torch.int32, device=x.device)
    dist.all_reduce(flag, op=dist.ReduceOp.MAX, group=group)  # a refusal is shared: all ranks raise together
    if err is not None:
        raise err
    if int(flag.item()):
        raise _ffi.DomainError(_ffi.ERR_DOMAIN, "another rank's shard was refused (a non-finite input?)")
    none = torch.iinfo(torch.int64).max
    trace_acc = torch.zeros(M, dtype=torch.int64, device=x.device)
    pivot = torch.empty(D + 1 + M, dtype=torch.float64, device=x.device)
    idx, maxres = [], []
    for j in range(M):
        top = cand[:1].clone()
        dist.all_reduce(top, op=dist.ReduceOp.MAX, group=group)  # non-negative doubles order as their bit patterns
        first = torch.where(cand[:1] == top, cand[1:], torch.full_like(top, none))
        dist.all_reduce(first, op=dist.ReduceOp.MIN, group=group)  # the lowest index among the holders
        dp = float(top.view(torch.float64).item())
        if int(top.item()) < 0 or dp <= threshold * variance:
            break
        rec = pivot[:D + 1 + j]
        _ffi.check(h, lib.agpl_greedy_pivot(h, N_total, i0, n, M, D, j, xp, wp, wb, first.data_ptr(), rec.data_ptr()))
        dist.all_reduce(rec, op=dist.ReduceOp.SUM, group=group)  # one owner, the others add zeros: exact
        z[j] = rec[:D]
        idx.append(int(first.item()))
        maxres.append(dp / variance)
        _ffi.check(h, lib.agpl_greedy_step(h, N_total, i0, n, M, D, kind, kparam, j, xp, ellp, variance, first.data_ptr(), rec.data_ptr(),
                                           wp, wb, cand.data_ptr(), trace_acc.data_ptr()))
    dist.all_reduce(trace_acc, op=dist.ReduceOp.SUM, group=group)  # int64: the sum is exact, whatever the order
    shift = 61 - max(N_total - 1, 0).bit_length()  # 61 - ceil(log2 N_total)
    trace = [float(int(t)) * 2.0 ** -shift for t in trace_acc.cpu().tolist()]
    return result(len(idx), idx, maxres, trace)


class Plan:
    """agpl_plan (include/agpl.h): the two split-float16 images of Phi (one scale), the Nystrom residual and q(v) in factor form,
    in ONE torch-owned block of device memory; the float32 features are not referenced after construction.  ANY feature count M:
    the plan pads to ``Mp = plan_padded(M)`` itself (round 6); ``U_colmajor`` / ``v`` are the Mp-sized state (checkpoints),
    ``U_lead`` / ``v_lead`` their leading M x M / M blocks -- the caller's q(v)."""

    NO_MARGINALS = 1  # AGPL_PLAN_NO_MARGINALS: Gibbs passes only (no marginal image)

    def __init__(self, Phi, resid, L, ctx: Context, flags: int = 0):
        N, M = Phi.shape
        nbytes = _ffi.lib().agpl_plan_bytes(C.c_int64(N), C.c_int32(M), C.c_int32(L), C.c_uint32(flags))
        self._create(ctx, N, M, L, flags, nbytes, Phi.device,
                     lambda: ctx.call("agpl_plan_create", C.c_int64(N), C.c_int32(M), C.c_int32(L), _ptr(Phi), _ptr(resid),
                                      C.c_uint32(flags), _ptr(self.mem), C.byref(self._h)))

    def _create(self, ctx, N, M, L, flags, nbytes, device, create, storage=None, D=None, variance=None, kernel=None,
                kernel_param=None, lengthscale=None):
        """What both routes into a plan end in: every attribute of a plan, its block of ``nbytes`` bytes (``storage``, if given),
        ``create()`` -- the library's constructor, which reads ``self.mem`` and fills ``self._h`` -- and the views of ``_bind``.
        ``D``, ``variance``, ``kernel``, ``kernel_param`` and ``lengthscale`` (host [D]) are those of a plan made from inputs (``se``), else None."""
        torch = _torch()
        self.ctx = ctx
        self.N, self.M, self.L, self.flags = N, M, L, flags
        self.Mp = plan_padded(M)
        self.se = D is not None
        self.D, self.variance, self.kernel, self.kernel_param = D, variance, kernel, kernel_param
        self.lengthscale = lengthscale  # (the periodic and cosine kinds' spectral measure depends on it: sample_paths)
        if nbytes <= 0:
            raise _ffi.ArgumentError(-1, f"a plan needs N >= 1 points, M >= 1 features (got {N}, {M}) and at most 64 "
                                         f"latents (got {L})")
        self._h = C.c_void_p()
        if storage is not None and (storage.dtype != torch.uint8 or storage.numel() < nbytes or storage.device != device):
            raise _ffi.ArgumentError(-1, f"storage must be a uint8 tensor of at least {nbytes} bytes on the inputs' device")
        self.mem = torch.empty(nbytes, dtype=torch.uint8, device=device) if storage is None else storage
        create()
        self._bind(nbytes)

    @classmethod
    def from_inputs(cls, x, z, lengthscale, variance: float = 1.0, jitter: float = 1e-8, L: int = 1, ctx: Context | None = None,
                    flags: int = 0, kernel="se", storage=None):
        """The plan of a stationary-kernel model straight from its raw inputs: x [N] or [N, D], z [M] or [M, D] (float64 CUDA
        tensors), ``lengthscale`` a number or D numbers, k(x, x') = variance kappa(|(x - x')/ell|), features Phi = L^-1 K_ZX with
        K_ZZ + jitter I = L L' -- all on the device in one pass over the points: no float32 Phi is formed.  ``kernel``
        (KernelFunctions.jl's conventions): ``"se"`` (the default, kappa = exp(-r^2 / 2): agpl_plan_create_se), ``"matern12"``
        (alias ``"exponential"``), ``"matern32"``, ``"matern52"``, ``("rq", alpha)``, ``("periodic", p)``, ``("se_periodic", p)`` or ``("se_cosine", p)`` (agpl_plan_create_stationary of
        include/agpl_kernels.h).  Such a plan also predicts (``predict``).
        ``select_inducing`` chooses z from the data.  ``storage``: the ``mem`` of a closed plan (``close``) of the same sizes, to
        build into: ``learn_hyperparameters`` rebuilds its plan in place."""
        torch = _torch()
        kind, kparam = kernel_kind(kernel)
        ctx = ctx or default_context()
        x = _prep(x, torch.float64, "x")
        z = _prep(z, torch.float64, "z")
        if x.dim() == 1:
            x = x.unsqueeze(1)
        if z.dim() == 1:
            z = z.unsqueeze(1)
        if x.dim() != 2 or z.dim() != 2 or x.shape[1] != z.shape[1]:
            raise _ffi.ArgumentError(-1, f"x [N, D] and z [M, D] must have the same D (got {tuple(x.shape)}, {tuple(z.shape)})")
        N, M, L, D = int(x.shape[0]), int(z.shape[0]), int(L), int(x.shape[1])
        ell = _lengthscales(lengthscale, D)
        _check_variance(variance)
        _check_jitter(jitter)
        self = cls.__new__(cls)

        def create():
            ell_dev = ell.contiguous().to(x.device)
            h = ctx.bind()
            sizes = (h, C.c_int64(N), C.c_int32(M), C.c_int32(L), C.c_int32(D))
            given = (_ptr(x), _ptr(z), _ptr(ell_dev), C.c_double(variance), C.c_double(jitter), C.c_uint32(flags), _ptr(self.mem),
                     C.byref(self._h))
            if kind == _ffi.KERNEL_SE:  # the default keeps its entry point (and loads no further library)
                rc = _ffi.se_lib().agpl_plan_create_se(*sizes, *given)
            else:
                rc = _ffi.kernels_lib().agpl_plan_create_stationary(*sizes, C.c_int32(kind), C.c_double(kparam), *given)
            _ffi.check(h, rc)

        nbytes = _ffi.se_lib().agpl_plan_se_bytes(C.c_int64(N), C.c_int32(M), C.c_int32(L), C.c_int32(D), C.c_uint32(flags))
        self._create(ctx, N, M, L, flags, nbytes, x.device, create, storage=storage, D=D, variance=float(variance),
                     kernel=_KERNEL_NAMES[kind], kernel_param=kparam, lengthscale=ell)
        return self

    def features(self, i0: int = 0, n: int | None = None):
        """The features the plan holds for points i0 .. i0 + n - 1, decoded from its accumulate image (agpl_plan_features):
        float32 [n, M]."""
        torch = _torch()
        n = self.N - i0 if n is None else n
        out = torch.empty((max(n, 0), self.M), dtype=torch.float32, device=self.mem.device)
        self.call("agpl_plan_features", C.c_int64(i0), C.c_int64(n), _ptr(out), lib=_ffi.se_lib())
        return out

    def predict(self, x_s, mu0_s=None):
        """q(f) of the plan's q(v) at new inputs (agpl_plan_predict; plans from ``from_inputs`` with the marginal image):
        (mu, var), float32 [L][Ns]."""
        torch = _torch()
        x_s = self._inputs_at(x_s, "x_s", "predict")
        Ns = int(x_s.shape[0])
        mu = torch.empty((self.L, Ns), dtype=torch.float32, device=x_s.device)
        var = torch.empty_like(mu)
        self.call("agpl_plan_predict", C.c_int64(Ns), _ptr(x_s), _ptr(_mu0_at(mu0_s, self.L, Ns)), _ptr(mu), _ptr(var),
                  lib=_ffi.se_lib())
        return mu, var

    def _qf_at(self, x_s, mu0_s=None):
        """``predict`` in the layout of the float64 operators: (mu, var) float64 [Ns] (one latent) or [Ns, L]."""
        return _point_major(*self.predict(x_s, mu0_s), self.L)

    def predict_y(self, lik, x_s, y_s=None, mu0_s=None, nsamples: int = 0, sweep: int | None = None, trials=None):
        """The predictive distribution of y at new inputs: ``operators.predictive`` of ``predict(x_s)`` -- (mean, var, logp),
        float64 [Ns] (categorical: (probs [Ns, K], None, logp)); logp needs the held-out observations ``y_s``.  ``trials`` [Ns]:
        the trial counts at the new inputs, required for ``BinomialTrialsLikelihood`` (``y_s`` is then the successes [Ns]) and
        refused for every other likelihood."""
        from . import operators as ops

        y, want = ops.obs_at(lik, y_s, trials, "predict_y")
        return ops._predictive(lik, self._qf_at(x_s, mu0_s), y, nsamples, sweep, self.ctx, want_logp=want)[:3]

    def heldout_logp(self, lik, x_s, y_s, mu0_s=None, nsamples: int = 0, sweep: int | None = None, trials=None) -> float:
        """Σ log p(y_s | x_s) under the plan's q(v): the device sum of agpl_predictive.  ``trials``: as ``predict_y``."""
        from . import operators as ops

        if y_s is None:
            raise _ffi.ArgumentError(-1, "heldout_logp needs the observations y_s")
        y = ops.obs_at(lik, y_s, trials, "heldout_logp")[0]
        return ops.log_predictive_density(lik, self._qf_at(x_s, mu0_s), y, nsamples=nsamples, sweep=sweep, ctx=self.ctx)

    def predict_cdf(self, lik, x_s, y_s, mu0_s=None, trials=None):
        """P(Y ≤ y_s) and P(Y > y_s) of the predictive of y at new inputs: ``operators.predictive_cdf`` of ``predict(x_s)`` --
        (cdf, sf), float64 [Ns]; cdf at held-out observations is their probability integral transform.  ``trials``: as ``predict_y``."""
        from . import operators as ops

        return ops.predictive_cdf(lik, self._qf_at(x_s, mu0_s), ops.obs_at(lik, y_s, trials, "predict_cdf")[0], ctx=self.ctx)

    def predict_quantiles(self, lik, x_s, probs=(0.025, 0.5, 0.975), mu0_s=None):
        """Quantiles of the predictive of y at new inputs: ``operators.predictive_quantile`` of ``predict(x_s)`` -- float64
        [Ns, len(probs)]; the default is the median with the central 95 % prediction interval."""
        from . import operators as ops

        return ops.predictive_quantile(lik, self._qf_at(x_s, mu0_s), probs, ctx=self.ctx)

    def predict_chain(self, V, x_s, mu0_s=None, samples: bool = False):
        """The posterior of f at new inputs from a chain of inducing draws ``V`` [T, L, M] (``SparseGibbs.run``'s output, or draws
        of q(v)): the equal-weight mixture over t of N(mu0 + phi' v_t, resid) (agpl_plan_predict_chain; plans from ``from_inputs``,
        with or without the marginal image).  Returns ``(mean, var, resid)``: mean and var = resid + spread of the mixture, float32
        [L][Ns], and the Nystrom residual [Ns]; with ``samples`` also ``F`` [T, L, Ns], the per-draw conditional means."""
        torch = _torch()
        x_s = self._inputs_at(x_s, "x_s", "predict_chain")
        V = self._chain(V, "the chain")
        T, Ns = int(V.shape[0]), int(x_s.shape[0])
        if T < 1:
            raise _ffi.ArgumentError(-1, "the chain needs at least one draw")
        mu0_s = _mu0_at(mu0_s, self.L, Ns)
        f32, dev = torch.float32, x_s.device
        mean = torch.empty((self.L, Ns), dtype=f32, device=dev)
        spread = torch.empty_like(mean)
        resid = torch.empty(Ns, dtype=f32, device=dev)
        F = torch.empty((T, self.L, Ns), dtype=f32, device=dev) if samples else None
        self.call("agpl_plan_predict_chain", C.c_int32(T), _ptr(V), C.c_int64(Ns), _ptr(x_s), _ptr(mu0_s), _ptr(mean), _ptr(spread),
                  _ptr(resid), _ptr(F), lib=_ffi.chain_lib())
        var = spread.add_(resid)
        return (mean, var, resid, F) if samples else (mean, var, resid)

    def _need_se(self, what):
        if not self.se:
            raise _ffi.ArgumentError(-1, f"{what} needs a plan made by Plan.from_inputs")

    def _inputs_at(self, x, name, what):
        """Inputs ``x`` [Ns] or [Ns, D] for the method ``what`` of a plan made from inputs: float64 [Ns, D]."""
        self._need_se(what)
        x = _prep(x, _torch().float64, name)
        if x.dim() == 1:
            x = x.unsqueeze(1)
        if x.dim() != 2 or x.shape[1] != self.D:
            raise _ffi.ArgumentError(-1, f"{name} must be [Ns, {self.D}] (got {tuple(x.shape)})")
        return x

    def _chain(self, V, name, nonempty: bool = False):
        """Draws of the whitened inducing coordinates as float64 [T, L, M]; [T, M] is taken as L = 1."""
        V = _prep(V, _torch().float64, "V")
        if V.dim() == 2 and self.L == 1:
            V = V.unsqueeze(1)
        if V.dim() != 3 or tuple(V.shape[1:]) != (self.L, self.M) or (nonempty and V.shape[0] < 1):
            raise _ffi.ArgumentError(-1, f"{name} must be [{'T >= 1' if nonempty else 'T'}, {self.L}, {self.M}] (got {tuple(V.shape)})")
        return V

    def predict_cov(self, x_a, x_b=None):
        """The joint posterior of f under the plan's q(v): Cov_l[i][j] = k(x_a_i, x_b_j) + phi(x_a_i)' (U_l' U_l - I) phi(x_b_j)
        (agpl_plan_predict_cov, include/agpl_joint.h; ``cov`` of u_posterior(fz, m, S)(x_te); plans from ``from_inputs`` with
        the marginal image), float32 [L, Na, Nb].  ``x_b=None``: the symmetric form at x_b = x_a (symmetric bit for bit; its
        diagonal is ``predict``'s var).  Larger matrices are assembled block by block from calls on slices of the inputs: an
        entry does not depend on the block it was computed in.  Out of scope: the joint covariance from a Gibbs chain."""
        torch = _torch()
        x_a = self._inputs_at(x_a, "x_a", "predict_cov")
        x_b = None if x_b is None else self._inputs_at(x_b, "x_b", "predict_cov")
        Na = int(x_a.shape[0])
        Nb = Na if x_b is None else int(x_b.shape[0])
        cov = torch.empty((self.L, Na, Nb), dtype=torch.float32, device=x_a.device)
        if Na == 0 or Nb == 0:  # (an empty x_b may have no address: it is not the symmetric form)
            return cov
        self.call("agpl_plan_predict_cov", C.c_int64(Na), _ptr(x_a), C.c_int64(Nb), _ptr(x_b), _ptr(cov), C.c_int64(Nb),
                  lib=_ffi.joint_lib())
        return cov

    def predict_grad(self, x_s):
        """The posterior of the gradient of f under the plan's q(v) at new inputs (agpl_plan_predict_grad, include/agpl_grad.h;
        plans from ``from_inputs`` with the marginal image, any kernel but ``"matern12"``, which is not differentiable):
        ``(dmu, dvar)``, float32 [L, D, Ns] -- the mean and the variance of d f_l / d x_d at every input, a closed-form Gaussian
        (no difference quotient of ``predict``).  The gradient of a prior mean function is the caller's to add to ``dmu``.
        Out of scope: derivatives from a Gibbs chain or of pathwise draws, the D x D covariance between the partial derivatives
        of a point, second derivatives."""
        torch = _torch()
        x_s = self._inputs_at(x_s, "x_s", "predict_grad")
        Ns = int(x_s.shape[0])
        dmu = torch.empty((self.L, self.D, Ns), dtype=torch.float32, device=x_s.device)
        dvar = torch.empty_like(dmu)
        self.call("agpl_plan_predict_grad", C.c_int64(Ns), _ptr(x_s), _ptr(dmu), _ptr(dvar), lib=_ffi.grad_lib())
        return dmu, dvar

    def sample_f(self, x_s, nsamples: int = 1, mu0_s=None, jitter: float = 1e-6, eps=None, generator=None):
        """Draws of f at x_s from the joint q(f) (``rand`` of u_posterior(fz, m, S)(x_te)), coherent across the inputs:
        f = mu + C eps, float64 [nsamples, L, Ns], with mu from ``predict``, C the lower Cholesky factor of
        float64(``predict_cov(x_s)``) + jitter variance I (factored on the device, agpl_dense_cholesky) and ``eps`` the given
        [nsamples, L, Ns] float64 standard normals (its first size then is ``nsamples``), else ``torch.randn`` on the device with ``generator``.  Not a hot path: the
        Ns x Ns factor and the triangular product are dense.  Out of scope: draws from a Gibbs chain's joint covariance.  Draws of y:
        ``sample_y``; sampling that avoids the Ns x Ns factor: ``sample_paths``."""
        torch = _torch()
        x_s = self._inputs_at(x_s, "x_s", "sample_f")
        Ns, L = int(x_s.shape[0]), self.L
        if nsamples < 0:
            raise _ffi.ArgumentError(-1, f"nsamples must be >= 0 (got {nsamples})")
        _check_jitter(jitter)
        if eps is None:
            eps = torch.randn((nsamples, L, Ns), dtype=torch.float64, device=x_s.device, generator=generator)
        else:
            eps = _prep(eps, torch.float64, "eps")
            if eps.dim() != 3 or tuple(eps.shape[1:]) != (L, Ns):
                raise _ffi.ArgumentError(-1, f"eps must be [nsamples, {L}, {Ns}] (got {tuple(eps.shape)})")
            nsamples = int(eps.shape[0])
        mu, _ = self.predict(x_s, mu0_s)
        if Ns == 0:
            return torch.empty((nsamples, L, 0), dtype=torch.float64, device=x_s.device)
        K = self.predict_cov(x_s).to(torch.float64)
        K.diagonal(dim1=1, dim2=2).add_(jitter * self.variance)
        out = torch.empty((nsamples, L, Ns), dtype=torch.float64, device=x_s.device)
        for l in range(L):
            try:
                self.ctx.call("agpl_dense_cholesky", C.c_int64(Ns), _ptr(K[l]), _ptr(K[l]))
            except _ffi.PosDefException as e:
                raise _ffi.PosDefException(e.code, f"the joint covariance of latent {l} at {Ns} inputs plus jitter = {jitter:g} "
                                                   f"x variance is not positive definite; raise the jitter") from e
            # the factor is the lower triangle of a column-major array: the upper triangle C' of this row-major view
            out[:, l] = mu[l].to(torch.float64) + eps[:, l] @ torch.triu(K[l])
        return out

    def sample_paths(self, nsamples=None, V=None, nfeatures: int = 2048, generator=None):
        """Pathwise draws of the posterior function (``Paths``): ``V`` [T, L, M] float64 are draws of the whitened inducing
        coordinates (a Gibbs chain gives one full posterior sample per draw); without ``V``, ``nsamples`` draws of the plan's
        q(v): V_t = U'(v + eps_t), the plan's S = U'U, m = U'v.  ``nfeatures`` random Fourier features of the plan's kernel
        (``spectral_frequencies``) carry the prior draw: the draws' covariance differs from the exact posterior's by
        O(variance / sqrt(nfeatures)).  ``generator`` (a torch generator on the plan's device) makes the draws reproducible.
        Plans from ``from_inputs``, with or without the marginal image."""
        torch = _torch()
        self._need_se("sample_paths")
        dev, f64 = self.mem.device, torch.float64
        if V is None:
            if nsamples is None or int(nsamples) < 1:
                raise _ffi.ArgumentError(-1, f"sample_paths needs V or nsamples >= 1 (got nsamples = {nsamples})")
            eps = torch.randn((int(nsamples), self.L, self.M), dtype=f64, device=dev, generator=generator)
            Ut = torch.triu(self.U_lead)  # the row-major view of the column-major lower triangle U: U'
            V = torch.einsum("lab,tlb->tla", Ut, self.v_lead.unsqueeze(0) + eps).contiguous()
        else:
            V = self._chain(V, "V", nonempty=True)
            if nsamples is not None and int(nsamples) != V.shape[0]:
                raise _ffi.ArgumentError(-1, f"nsamples = {nsamples}, V holds {V.shape[0]} draws")
        T = int(V.shape[0])
        kernel = (self.kernel, self.kernel_param) if self.kernel in _KERNEL_PARAMS else self.kernel
        omega, phase = spectral_frequencies(kernel, nfeatures, self.D, generator=generator, device=dev,
                                            lengthscale=self.lengthscale)
        W = torch.randn((T, self.L, int(nfeatures)), dtype=f64, device=dev, generator=generator)
        Xi = torch.randn((T, self.L, self.M), dtype=f64, device=dev, generator=generator)
        return Paths(self, V, omega, phase, W, Xi)

    def sample_y(self, lik, x_s, nsamples: int, mu0_s=None, method: str = "paths", nfeatures: int = 2048, generator=None,
                 sweep: int | None = None):
        """``nsamples`` posterior-predictive draws of y at new inputs under the plan's q(v) (``rand(lik(f))`` of the reference's
        examples): ``operators.sample_y`` of function draws -- ``method="paths"``: ``sample_paths`` (any Ns, ``nfeatures`` random
        features); ``method="joint"``: ``sample_f`` (the exact joint covariance, dense in Ns).  uint8 / int32 / float64
        [nsamples, Ns], one-hot uint8 [nsamples, Ns, L] for the categorical kinds."""
        from . import operators as ops

        if lik._nlatent != self.L:
            raise _ffi.ArgumentError(-1, f"the likelihood has {lik._nlatent} latents, the plan {self.L}")
        if method == "paths":
            return self.sample_paths(nsamples, nfeatures=nfeatures, generator=generator).sample_y(lik, x_s, mu0_s, sweep=sweep)
        if method != "joint":
            raise _ffi.ArgumentError(-1, f"method must be 'paths' or 'joint' (got {method!r})")
        return ops.sample_y(lik, self.sample_f(x_s, nsamples, mu0_s, generator=generator), sweep=sweep, ctx=self.ctx)

    _MIX_CHUNK = 1 << 15  # points per step of the mixture of y (T L float32 conditional means per point)

    def predict_y_chain(self, lik, V, x_s, y_s=None, mu0_s=None, nsamples: int = 0, sweep: int | None = None, trials=None):
        """The predictive distribution of y at new inputs under a chain of inducing draws, Rao-Blackwellised: ``operators.predictive``
        of every draw's N(F[t], resid), combined over t in float64 on the device --
        E[y] = mean_t E_t, Var[y] = mean_t (Var_t + E_t^2) - E[y]^2, log p(y*) = logsumexp_t log p_t - log T.
        ``(mean, var, logp)``, float64 [Ns] (categorical: (probs [Ns, K], None, logp)); logp needs ``y_s``."""
        from . import operators as ops

        torch = _torch()
        x_s = self._inputs_at(x_s, "x_s", "predict_chain")  # (the entry point every chunk goes through)
        Ns, L = int(x_s.shape[0]), self.L
        mu0_s = _mu0_at(mu0_s, L, Ns)
        if mu0_s is not None:
            mu0_s = mu0_s.reshape(L, Ns)
        y_s, want = ops.obs_at(lik, y_s, trials, "predict_y")  # (trials [Ns]: the per-point Binomial's, refused otherwise)
        y_s = _prep_y(lik, y_s, torch.float64)
        means, variances, logps = [], [], []
        for c0 in range(0, Ns, self._MIX_CHUNK):
            c1 = min(Ns, c0 + self._MIX_CHUNK)
            _, _, resid, F = self.predict_chain(V, x_s[c0:c1], None if mu0_s is None else mu0_s[:, c0:c1].contiguous(), samples=True)
            T = F.shape[0]
            d = resid.to(torch.float64)
            d = d if L == 1 else d.unsqueeze(1).expand(c1 - c0, L).contiguous()
            yc = None if y_s is None else y_s[c0:c1]
            e1 = e2 = None
            lp = []
            for t in range(T):
                f = F[t, 0].to(torch.float64) if L == 1 else F[t].t().contiguous().to(torch.float64)
                m, v, lg = ops._predictive(lik, (f, d), yc, nsamples, sweep, self.ctx, want_logp=want)[:3]
                e1 = m.clone() if e1 is None else e1.add_(m)
                if v is not None:
                    e2 = v + m * m if e2 is None else e2.add_(v + m * m)
                if lg is not None:
                    lp.append(lg)
            e1 /= T
            means.append(e1)
            if e2 is not None:
                variances.append(e2 / T - e1 * e1)
            if lp:
                logps.append(torch.logsumexp(torch.stack(lp), dim=0) - float(np.log(T)))
        cat = lambda parts: torch.cat(parts) if parts else None
        return cat(means), cat(variances), cat(logps)

    def hyper_grad(self, x, beta, gamma, mu0=None, G=None, g=None):
        """The gradient of the sweep's bound at the plan's q(v) with respect to (log lengthscale_1 .. log lengthscale_D, log variance)
        (agpl_plan_hyper_grad, include/agpl_hyper.h): float64 [D + 1] on the device.  ``x``: the inputs the plan was made from;
        ``beta``, ``gamma`` [L][N] float32 (and ``mu0``): a pass's expected potential / precision; ``G``, ``g``: that pass's
        naturals summed over ranks -- given, the K_ZZ part is added to the points' part (one rank of a sharded run passes them,
        and the D + 1 numbers are summed over ranks)."""
        torch = _torch()
        N, x, *sites = self._grad_args("hyper_grad", x, beta, gamma, mu0, G, g)
        out = torch.empty(self.D + 1, dtype=torch.float64, device=x.device)
        self.call("agpl_plan_hyper_grad", C.c_int64(N), _ptr(x), *map(_ptr, sites), _ptr(out), lib=_ffi.hyper_lib())
        return out

    def _grad_args(self, what, x, beta, gamma, mu0, G, g):
        """The arguments ``hyper_grad`` and ``inducing_grad`` share, prepared and checked, in the order agpl_plan_hyper_grad and
        agpl_plan_inducing_grad take them: (N, x, mu0, beta, gamma, G, g)."""
        torch = _torch()
        x = self._inputs_at(x, "x", what)
        beta, gamma, mu0 = (_prep(t, torch.float32, n) for t, n in ((beta, "beta"), (gamma, "gamma"), (mu0, "mu0")))
        G, g = _prep(G, torch.float64, "G"), _prep(g, torch.float64, "g")
        N = int(x.shape[0])
        _check_sites(self.L, N, beta=beta, gamma=gamma, mu0=mu0)
        if (G is None) != (g is None) or (G is not None and (G.numel() != self.L * self.M * self.M or g.numel() != self.L * self.M)):
            raise _ffi.ArgumentError(-1, f"G [{self.L}, {self.M}, {self.M}] and g [{self.L}, {self.M}] are given together")
        return N, x, mu0, beta, gamma, G, g

    def inducing_grad(self, x, beta, gamma, mu0=None, G=None, g=None, with_theta: bool = False):
        """The gradient of the sweep's bound at the plan's q(v) with respect to the inducing inputs z, in the caller's units
        (agpl_plan_inducing_grad, include/agpl_zgrad.h): float64 [M, D] on the device.  Arguments as ``hyper_grad``; ``G``, ``g``
        given, the K_ZZ part is added (one rank of a sharded run passes them, and the numbers are summed over ranks).
        ``with_theta``: return ``(theta [D + 1], z [M, D])`` -- ``theta`` is ``hyper_grad``'s result, bit for bit, from the same
        pass over the points."""
        torch = _torch()
        N, x, *sites = self._grad_args("inducing_grad", x, beta, gamma, mu0, G, g)
        theta = torch.empty(self.D + 1, dtype=torch.float64, device=x.device) if with_theta else None
        out = torch.empty((self.M, self.D), dtype=torch.float64, device=x.device)
        self.call("agpl_plan_inducing_grad", C.c_int64(N), _ptr(x), *map(_ptr, sites), _ptr(theta), _ptr(out), lib=_ffi.zgrad_lib())
        return (theta, out) if with_theta else out

    def loo_cavity(self, gamma, beta, mu0=None):
        """The leave-one-out cavity of the plan's q(v) at its own points (agpl_plan_loo, include/agpl_loo.h): site i taken out of
        q(v) by a rank-one downdate, from one marginal pass.  ``gamma``, ``beta`` [L][N] float32: the sites of the q(v) the plan
        holds (the gamma / beta of the pass whose G, g the last update was given); ``mu0`` as ``agpl_marginals_plan`` takes it.
        Returns ``(mu, var, lev, lev_sum, n_bad, first_bad)``: the cavity's mean and variance and the leverages h = gamma q, float64
        [N] (one latent) or [N, L] -- the layout ``operators.predictive`` / ``predictive_cdf`` take --, Σᵢ h per latent (float64
        [L] on the device), and the number and the lowest flat index l N + i (-1: none) of the pairs without a cavity (NaN in the
        three outputs; h >= 1 means the sites are not this q(v)'s).  Reading the two counts waits for the stream."""
        torch = _torch()
        gamma, beta, mu0 = (_prep(t, torch.float32, n) for t, n in ((gamma, "gamma"), (beta, "beta"), (mu0, "mu0")))
        _check_sites(self.L, self.N, gamma=gamma, beta=beta, mu0=mu0)
        lib = _ffi.loo_lib()
        dev, f64 = self.mem.device, torch.float64
        nbytes = lib.agpl_plan_loo_bytes(self.N, self.L)
        work = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        shape = (self.N,) if self.L == 1 else (self.N, self.L)
        mu, var, lev = (torch.empty(shape, dtype=f64, device=dev) for _ in range(3))
        lev_sum = torch.empty(self.L, dtype=f64, device=dev)
        info = torch.empty(2, dtype=torch.int64, device=dev)
        self.call("agpl_plan_loo", _ptr(mu0), _ptr(gamma), _ptr(beta), _ptr(work), nbytes, _ptr(mu), _ptr(var), _ptr(lev), _ptr(lev_sum),
                  _ptr(info), lib=lib)
        n_bad, first_bad = (int(t) for t in info.cpu().tolist())
        return mu, var, lev, lev_sum, n_bad, first_bad

    def close(self):
        """Destroy the plan now (its ``mem`` may then back a new plan of the same sizes: ``from_inputs(storage=...)``)."""
        if self._h:
            self.ctx.synchronize()
            _ffi.check(self.ctx._h, _ffi.lib().agpl_plan_destroy(self._h))
            self._h = None
            for k in self._STATE + ("resid", "U_lead", "v_lead"):  # (views into storage a new plan may now overwrite)
                setattr(self, k, None)

    def _bind(self, nbytes):
        """Views of the plan's state inside its memory block."""
        torch = _torch()
        L, ctx = self.L, self.ctx
        U, v, uh, ul, v32, ld, rs = (C.c_void_p() for _ in range(7))
        _ffi.check(ctx._h, _ffi.lib().agpl_plan_state(self._h, C.byref(U), C.byref(v), C.byref(uh), C.byref(ul), C.byref(v32),
                                                      C.byref(ld), C.byref(rs)))
        base = self.mem.data_ptr()
        M = self.Mp  # the state arrays are sized by the padded feature count
        view = lambda ptr, nb, dt: self.mem[ptr.value - base: ptr.value - base + nb].view(dt)
        self.U_colmajor = view(U, 8 * L * M * M, torch.float64).view(L, M, M)
        self.v = view(v, 8 * L * M, torch.float64).view(L, M)
        self.U_hi, self.U_lo = view(uh, 2 * L * M * M, torch.float16), view(ul, 2 * L * M * M, torch.float16)
        self.v32 = view(v32, 4 * L * M, torch.float32).view(L, M)
        self.logdet = view(ld, 8 * L, torch.float64)
        self.resid = view(rs, 4 * self.N, torch.float32)  # the plan's residual copy d_i
        e = C.c_int32()
        _ffi.check(ctx._h, _ffi.lib().agpl_plan_info(self._h, None, None, None, C.byref(e), None))
        self.scale_exp = e.value
        self.nbytes = nbytes
        self.U_lead = self.U_colmajor[:, : self.M, : self.M]
        self.v_lead = self.v[:, : self.M]

    def call(self, name, *args, lib=None):
        self.ctx.bind()
        _ffi.check(self.ctx._h, getattr(lib or _ffi.lib(), name)(self._h, *args))

    _STATE = ("U_colmajor", "v", "U_hi", "U_lo", "v32", "logdet")

    def state(self):
        """Checkpoint of what an update rewrites (agpl_plan_state: U, v, their float16 / float32 images,
        log det(I + G)) as host tensors.  The images of Phi are static: a restoring process rebuilds them from the same features."""
        self.ctx.synchronize()
        return {k: getattr(self, k).detach().cpu().clone() for k in self._STATE}

    def load_state(self, st):
        """Restore a checkpoint into a plan created for the same data: the next pass is bit for bit the saved run's."""
        self.ctx.synchronize()
        for k in self._STATE:
            dst = getattr(self, k)
            if tuple(st[k].shape) != tuple(dst.shape) or st[k].dtype != dst.dtype:
                raise _ffi.ArgumentError(-1, f"checkpoint field {k}: {tuple(st[k].shape)} {st[k].dtype}, the plan holds "
                                             f"{tuple(dst.shape)} {dst.dtype}")
            dst.copy_(st[k])

    def __del__(self):
        try:
            if self._h:
                _ffi.lib().agpl_plan_destroy(self._h)
                self._h = None
        except Exception:
            pass


def exchange_natural_parameters(G, g, group=None, flat=None):
    """The one exchange step of a sweep: sum the per-rank partials of the M x M natural-parameter
    accumulators over the ranks that shard N (torch.distributed all-reduce; backend "nccl" = RCCL over
    xGMI on the GPU box, "gloo" in the CPU tests).  float64 on the wire; in place.  ``flat``: the buffer G and g are
    views of (natural_parameter_buffers) -- one collective instead of two."""
    for t in (G, g) if flat is None else (flat,):
        _all_reduce_sum(t, group)
    return G, g


class LooResult:
    """What ``SparseCAVI.loo`` returns: ``logp`` (log p(yᵢ | y₋ᵢ), float64 [N] on the device), ``elpd`` (their sum, a float),
    ``leverage`` (float64 [N] or [N, L] on the device), ``p_eff`` (Σᵢ h per latent, float64 host tensor [L]), ``n_bad`` (pairs without
    a cavity)."""

    __slots__ = ("logp", "elpd", "leverage", "p_eff", "n_bad")

    def __init__(self, logp, elpd, leverage, p_eff, n_bad):
        self.logp, self.elpd, self.leverage, self.p_eff, self.n_bad = logp, elpd, leverage, p_eff, n_bad

    def __repr__(self):
        return f"LooResult(elpd={self.elpd!r}, p_eff={self.p_eff.tolist()}, n_bad={self.n_bad})"


class SparseCAVI:
    """CAVI sweeps over N local points and M features.

    Phi: float32 [N, M] CUDA tensor (any M on the plan path, which pads to a multiple of 256 itself; M % 128 == 0 for the
    float32-input pair); kdiag: float32 [N] (d_i above); y as the likelihood
    wants it (real-valued y: float32); mu0: optional prior mean at the data, float32 [L][N].
    ``group``: a torch.distributed process group over which N is sharded (None = single GPU).
    """

    def __init__(self, lik, Phi, kdiag, y, mu0=None, ctx: Context | None = None, group=None, keep_points=False,
                 marginal_precision: str = "auto", accumulate_precision: str = "auto", track_elbo: bool = False):
        """Two arithmetics, chosen for both contractions together:
          * the shipped path ("f16x2-factor" marginals + "f16x2" accumulation; "auto"): ONE plan (agpl_plan_create: both
            split-float16 images of Phi with one scale, q(v) in factor form; any feature count -- the plan zero-pads to a multiple
            of 256 itself, G / g / S / m stay M-sized) and agpl_cavi_pass_plan / agpl_plan_update per sweep;
          * "f32" / "f32" (on request): the float32-input MFMA kernels (agpl_cavi_pass + agpl_gaussian_update), the
            arithmetic SURVEY.md 8(d) prices; feature count a multiple of 128.
        ``track_elbo``: the per-point ELBO terms ride the pass and the Gaussian KL the update (plan path only); see
        ``elbo_entering``."""
        torch = _torch()
        Phi, kdiag = _prep(Phi, torch.float32, "Phi"), _prep(kdiag, torch.float32, "kdiag")
        split_names = ("f16x2", "f16x2-factor")
        if marginal_precision == "auto":
            marginal_precision = "f32" if accumulate_precision == "f32" else "f16x2-factor"
        if accumulate_precision == "auto":
            accumulate_precision = "f32" if marginal_precision == "f32" else "f16x2"
        if marginal_precision not in ("f32", "f16x2-factor") or accumulate_precision not in ("f32", "f16x2"):
            raise _ffi.ArgumentError(-1, "marginal_precision must be 'auto', 'f32' or 'f16x2-factor', accumulate_precision 'auto', "
                                         "'f32' or 'f16x2'")
        if (marginal_precision in split_names) != (accumulate_precision == "f16x2"):
            # the entry points come in two arithmetics: float32-input MFMA for both contractions (agpl_cavi_pass), or
            # split-float16 for both (the plan)
            raise _ffi.ArgumentError(-1, "marginal_precision and accumulate_precision must both be 'f32' or both be split-float16")
        if marginal_precision == "f32" and Phi.shape[1] % PAD:
            raise _ffi.ArgumentError(-1, f"the float32-input kernels need a feature count that is a multiple of {PAD} (got {Phi.shape[1]}; "
                                         "zero-pad, or take the plan path)")
        self._setup(lik, ctx or default_context(), Phi, kdiag, None, y, mu0, group, keep_points, track_elbo, marginal_precision)

    def _setup(self, lik, ctx, Phi, kdiag, plan, y, mu0, group, keep_points, track_elbo, marginal_precision="f16x2-factor", x=None):
        """What both constructors end in, and the one place that names the attributes of a SparseCAVI.  ``Phi`` (float32 features;
        on the plan path their plan is made here) or ``plan`` (made from inputs: ``Phi`` is None); ``kdiag``: the residual d_i;
        ``x``: the inputs ``hyper_grad`` regenerates the features from, if they are kept."""
        torch = _torch()
        self.ctx, self.lik, self.x = ctx, lik, x
        self.Phi, self.kdiag = Phi, kdiag
        self.N, self.M = (plan.N, plan.M) if Phi is None else Phi.shape
        self.L = lik._nlatent
        self.y = _prep_y(lik, y, torch.float32)
        self.mu0 = _prep(mu0, torch.float32, "mu0")
        self.group = group
        self.marginal_precision = marginal_precision
        self.factor = marginal_precision == "f16x2-factor"
        dev = plan.mem.device if Phi is None else Phi.device
        L, M = self.L, self.M
        f64, f32 = torch.float64, torch.float32
        self.track_elbo = bool(track_elbo)
        self.gamma = self.beta = self.c = None
        if keep_points:
            self.gamma = torch.empty((L, self.N), dtype=f32, device=dev)
            self.beta = torch.empty((L, self.N), dtype=f32, device=dev)
            self.c = torch.empty((self.N,) if L == 1 else (self.N, L), dtype=f32, device=dev)
        self.nsweeps = 0
        self._sites_of = None  # the sweep count at which gamma / beta were the sites behind q(v) (sweep(); read by loo())
        self._Gg, self.G, self.g = natural_parameter_buffers(L, M, dev, extra=1 if (self.track_elbo and self.factor) else 0)
        self._kl = torch.zeros(2, dtype=f64, device=dev)  # KL(q(v) || p(v)) of the last two updates (q = N(0, I) at start)
        self.resid = kdiag  # kdiag is already d_i = k_ii - |phi_i|^2 (agpl_feature_residual / nystrom_residual)
        self.plan = self._elbo_terms = self.A_work = self.v = self._S = self._m = self.Wpack = self.alpha = None
        if self.factor:
            self.plan = Plan(Phi, kdiag, L, ctx) if plan is None else plan
            self._elbo_terms = self._Gg[-1:] if self.track_elbo else None
            self.A_work, self.v = self.plan.U_lead, self.plan.v_lead  # (views of the plan's state: the caller's M x M / M blocks)
            return
        if self.track_elbo:
            raise _ffi.ArgumentError(-1, "track_elbo rides the plan path (the default arithmetic)")
        # q(v) = N(0, I) (script.jl:41-42): the update of G = 0, g = 0 gives S = I, m = 0 and the packed -I the first pass reads
        self._S = torch.empty((L, M, M), dtype=f64, device=dev)
        self._m = torch.empty((L, M), dtype=f64, device=dev)
        self.Wpack = torch.empty((L, M, M), dtype=f32, device=dev)
        self.alpha = torch.empty((L, M), dtype=f32, device=dev)
        self.update()

    @classmethod
    def from_inputs(cls, lik, x, y, z, lengthscale, variance: float = 1.0, jitter: float = 1e-8, mu0=None, ctx: Context | None = None,
                    group=None, keep_points=False, track_elbo: bool = False, kernel="se", keep_inputs: bool = False, storage=None):
        """CAVI of a stationary-kernel model from its raw inputs: the plan is built by ``Plan.from_inputs`` (x: this rank's
        points, float64 [N] or [N, D]; z [M] or [M, D]; ``kernel``: ``"se"``, ``"matern12"`` / ``"exponential"``, ``"matern32"``,
        ``"matern52"`` or ``("rq", alpha)``); no float32 features are held.  ``predict`` gives q(f) at new inputs.
        ``select_inducing`` chooses z from the data.  ``keep_inputs``: keep a reference to ``x`` (``hyper_grad`` regenerates the
        features from it); ``storage``: as ``Plan.from_inputs``."""
        kernel_kind(kernel)  # (refused before any device work)
        ctx = ctx or default_context()
        plan = Plan.from_inputs(x, z, lengthscale, variance, jitter, L=lik._nlatent, ctx=ctx, kernel=kernel, storage=storage)
        self = cls.__new__(cls)
        self._setup(lik, ctx, None, plan.resid, plan, y, mu0, group, keep_points, track_elbo, x=x if keep_inputs else None)
        return self

    def _se_plan(self, what, inputs: bool = False):
        """The plan, if it can take new inputs (``inputs``: and the training inputs were kept); ``what`` asks for it."""
        if self.plan is None or not self.plan.se or (inputs and self.x is None):
            raise _ffi.ArgumentError(-1, f"{what} needs a SparseCAVI made by SparseCAVI.from_inputs"
                                         + ("(..., keep_inputs=True)" if inputs else ""))
        return self.plan

    def predict(self, x_s, mu0_s=None):
        """q(f) at new inputs for the current q(v) (u_posterior(fz, m, S)(x_te), examples/bernoulli/script.jl:46-56):
        (mu, var) float32 [L][Ns].  Needs an object made by ``from_inputs``."""
        return self._se_plan("predict").predict(x_s, mu0_s)

    def predict_cov(self, x_a, x_b=None):
        """The joint posterior covariance of f between new inputs for the current q(v) (``cov`` of u_posterior(fz, m, S)(x_te)):
        float32 [L, Na, Nb] of ``Plan.predict_cov``; ``x_b=None`` is the symmetric form.  Needs an object made by ``from_inputs``.
        Out of scope: the joint covariance from a Gibbs chain."""
        return self._se_plan("predict_cov").predict_cov(x_a, x_b)

    def predict_grad(self, x_s):
        """The posterior of the gradient of f at new inputs for the current q(v): ``(dmu, dvar)``, float32 [L, D, Ns] of
        ``Plan.predict_grad`` (mean and variance of d f_l / d x_d).  Needs an object made by ``from_inputs``."""
        return self._se_plan("predict_grad").predict_grad(x_s)

    def sample_f(self, x_s, nsamples: int = 1, mu0_s=None, jitter: float = 1e-6, eps=None, generator=None):
        """Function draws from the joint q(f) at new inputs for the current q(v) (``rand`` of u_posterior(fz, m, S)(x_te)):
        float64 [nsamples, L, Ns] of ``Plan.sample_f``.  Needs an object made by ``from_inputs``.  Draws of y: ``sample_y``;
        draws from a Gibbs chain or without the Ns x Ns factor: ``sample_paths``."""
        return self._se_plan("sample_f").sample_f(x_s, nsamples, mu0_s, jitter=jitter, eps=eps, generator=generator)

    def sample_paths(self, nsamples: int, nfeatures: int = 2048, generator=None):
        """``nsamples`` pathwise draws of the posterior function for the current q(v) (``Plan.sample_paths``): a ``Paths`` object
        to evaluate at any inputs, float32 [nsamples, L, Ns] each time.  Needs an object made by ``from_inputs``."""
        plan = self._se_plan("sample_paths")
        self.check()
        return plan.sample_paths(nsamples, nfeatures=nfeatures, generator=generator)

    def sample_y(self, x_s, nsamples: int, mu0_s=None, method: str = "paths", nfeatures: int = 2048, generator=None,
                 sweep: int | None = None):
        """``nsamples`` posterior-predictive draws of y at new inputs for the current q(v) and this object's likelihood
        (``Plan.sample_y``): [nsamples, Ns] (categorical: one-hot [nsamples, Ns, L]).  Needs an object made by ``from_inputs``."""
        plan = self._se_plan("sample_y")
        self.check()
        return plan.sample_y(self.lik, x_s, nsamples, mu0_s, method=method, nfeatures=nfeatures, generator=generator, sweep=sweep)

    def predict_y(self, x_s, y_s=None, mu0_s=None, nsamples: int = 0, sweep: int | None = None, trials=None):
        """p(y*) at new inputs for the current q(v): (mean, var, logp) of ``operators.predictive`` on ``predict(x_s)`` (categorical:
        (probs, None, logp)); logp = log ∫ p(y_s | f) q(f) df needs ``y_s``.  Needs an object made by ``from_inputs``.  ``trials``
        [Ns]: required for ``BinomialTrialsLikelihood``, refused otherwise (``Plan.predict_y``)."""
        return self._se_plan("predict_y").predict_y(self.lik, x_s, y_s, mu0_s, nsamples=nsamples, sweep=sweep, trials=trials)

    def predict_cdf(self, x_s, y_s, mu0_s=None, trials=None):
        """P(Y ≤ y_s) and P(Y > y_s) of p(y*) at new inputs for the current q(v) and this object's likelihood (``Plan.predict_cdf``):
        (cdf, sf), float64 [Ns].  Needs an object made by ``from_inputs``.  Out of scope: a Gibbs chain (it has ``sample_y``)."""
        return self._se_plan("predict_cdf").predict_cdf(self.lik, x_s, y_s, mu0_s, trials=trials)

    def predict_quantiles(self, x_s, probs=(0.025, 0.5, 0.975), mu0_s=None):
        """Quantiles of p(y*) at new inputs for the current q(v) and this object's likelihood (``Plan.predict_quantiles``): float64
        [Ns, len(probs)], by default the median with the central 95 % prediction interval.  Needs an object made by ``from_inputs``."""
        return self._se_plan("predict_quantiles").predict_quantiles(self.lik, x_s, probs, mu0_s)

    def heldout_logp(self, x_s, y_s, mu0_s=None, nsamples: int = 0, sweep: int | None = None, trials=None) -> float:
        """Σ log p(y_s | x_s) of held-out data under the current q(v) (summed on the device).  ``trials``: as ``predict_y``."""
        return self._se_plan("heldout_logp").heldout_logp(self.lik, x_s, y_s, mu0_s, nsamples=nsamples, sweep=sweep, trials=trials)

    def hyper_grad(self, inducing: bool = False):
        """The gradient of the bound the sweep maximises, at the current q(v), with respect to the kernel's hyperparameters:
        ``{"log_lengthscale": [D] float64 (host), "log_variance": float}``; with ``inducing=True`` also ``"z"``: float64 [M, D]
        (host), the gradient for the inducing inputs, from the same pass over the points (``Plan.inducing_grad(with_theta=True)``
        in place of ``Plan.hyper_grad``; one all-reduce of the D + 1 + M D numbers).  One pass that keeps beta / gamma (its G, g go to
        buffers of their own and are summed over ``group``: the sweep's state is untouched), ``Plan.hyper_grad`` on this rank's
        points -- rank 0 adds the K_ZZ part -- and one all-reduce of the D + 1 numbers.  beta / gamma of this pass go to buffers of
        their own too (``keep_points`` keeps the last sweep's).  Needs ``from_inputs(keep_inputs=True)``."""
        plan = self._se_plan("hyper_grad", inputs=True)
        gamma, beta, flat, G, g = self._fresh_pass()
        exchange_natural_parameters(G, g, self.group, flat=flat)
        if self.group is not None and _dist().get_rank(self.group) != 0:
            G = g = None  # (the K_ZZ part is counted once)
        if inducing:
            theta, gz = plan.inducing_grad(self.x, beta, gamma, self.mu0, G, g, with_theta=True)
            both = _torch().cat([theta, gz.reshape(-1)])
            _all_reduce_sum(both, self.group)
            both = both.cpu()
            D1 = theta.numel()
            return {"log_lengthscale": both[: D1 - 1].clone(), "log_variance": float(both[D1 - 1]),
                    "z": both[D1:].reshape(gz.shape).clone()}
        grad = plan.hyper_grad(self.x, beta, gamma, self.mu0, G, g)
        _all_reduce_sum(grad, self.group)
        grad = grad.cpu()
        return {"log_lengthscale": grad[:-1].clone(), "log_variance": float(grad[-1])}

    def _fresh_pass(self):
        """One pass like ``accumulate()``'s at the current q(v) into buffers of its own -- the sweep's G, g, gamma, beta and ELBO
        terms stay untouched: ``(gamma, beta, flat, G, g)``, G and g views of ``flat`` (``natural_parameter_buffers``), this
        rank's partials.  Plan path only."""
        torch = _torch()
        dev, f32 = self.plan.mem.device, torch.float32
        gamma = torch.empty((self.L, self.N), dtype=f32, device=dev)
        beta = torch.empty((self.L, self.N), dtype=f32, device=dev)
        flat, G, g = natural_parameter_buffers(self.L, self.M, dev)
        d = self.lik.desc()
        self.plan.call("agpl_cavi_pass_plan", C.byref(d), _ptr(self.mu0), _ptr(self.y), _ptr(G), _ptr(g), C.c_void_p(0),
                       _ptr(gamma), _ptr(beta), C.c_void_p(0))
        return gamma, beta, flat, G, g

    @property
    def S(self):
        """Covariance of q(v).  In the factor form it is materialised on demand: S = U'U, U' = triu of A_work viewed
        row-major (the column-major lower triangle holds U)."""
        if not self.factor:
            return self._S
        self.check()
        Ut = _torch().triu(self.A_work)
        return Ut @ Ut.transpose(1, 2)

    @property
    def m(self):
        if not self.factor:
            return self._m
        self.check()
        return (_torch().triu(self.A_work) @ self.v.unsqueeze(-1)).squeeze(-1)

    def accumulate(self):
        """marginals -> aux_posterior! -> expected potential/precision -> local (G, g)."""
        d = self.lik.desc()
        if self.plan is not None:  # the shipped path
            self.plan.call("agpl_cavi_pass_plan", C.byref(d), _ptr(self.mu0), _ptr(self.y), _ptr(self.G), _ptr(self.g),
                           _ptr(self.c), _ptr(self.gamma), _ptr(self.beta), _ptr(self._elbo_terms))
            return
        self.ctx.call("agpl_cavi_pass", C.byref(d), C.c_int64(self.N), C.c_int32(self.M), _ptr(self.Phi),
                      _ptr(self.kdiag), _ptr(self.mu0), _ptr(self.y), _ptr(self.Wpack), _ptr(self.alpha),
                      _ptr(self.G), _ptr(self.g), _ptr(self.c), _ptr(self.gamma), _ptr(self.beta))

    exchange_timing = None  # a list: exchange() appends a (start, stop) pair of timing events per call (bench.py)

    def exchange(self):
        """Sum (G, g) over the ranks that shard N; every rank then performs the identical M x M update."""
        timed = self.exchange_timing is not None and self.group is not None
        if timed:
            torch = _torch()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
        exchange_natural_parameters(self.G, self.g, self.group, flat=self._Gg)
        if timed:
            e1.record()
            self.exchange_timing.append((e0, e1))

    def update(self):
        """S = (I + G)^-1, m = S g (examples/bernoulli/script.jl:35-36 in sparse whitened form); the plan keeps
        U = chol(I + G)^-1 and v = U g (S = U'U, m = U'v) and the images of U."""
        if self.plan is not None:
            # enqueue only: a failed factorisation surfaces in the next accumulate() (once its kernels are queued),
            # in check(), or when S / m / elbo() are read -- the host never idles the GPU between update and pass
            kl = self._kl[self.nsweeps & 1:(self.nsweeps & 1) + 1] if self.track_elbo else None
            self.plan.call("agpl_plan_update", _ptr(self.G), _ptr(self.g), C.c_void_p(0), _ptr(kl))
            return
        self.ctx.call("agpl_gaussian_update", C.c_int32(self.M), C.c_int32(self.L), _ptr(self.G), _ptr(self.g),
                      C.c_void_p(0), _ptr(self._S), _ptr(self._m), _ptr(self.Wpack), _ptr(self.alpha), _ptr(self._kl[:1]))

    def sweep(self):
        self.accumulate()
        self.exchange()
        self.update()
        self.nsweeps += 1
        self._sites_of = self.nsweeps  # gamma / beta (keep_points) are now the sites behind q(v): what loo() reads

    def check(self):
        """Wait for the stream and raise what a deferred factorisation has to report (PosDefException, ...)."""
        self.ctx.synchronize()

    def state_dict(self):
        """Checkpoint of the sweep loop (SURVEY.md 5 "checkpoint / resume"; the reference's state is the (m, S, qΩ) of
        examples/bernoulli/script.jl:41-43): q(v) in the plan's factor form, the reduced (G, g) of the last sweep, the sweep count
        and the context's Philox key / draw counter.  qΩ is a function of q(v) and is not stored.  Plan path only."""
        if self.plan is None:
            raise _ffi.ArgumentError(-1, "state_dict is the plan path's (the default arithmetic)")
        self.check()
        return {"plan": self.plan.state(), "Gg": self._Gg.detach().cpu().clone(), "kl": self._kl.detach().cpu().clone(),
                "nsweeps": self.nsweeps, "seed": int(self.ctx.seed), "sweep_counter": int(self.ctx.sweep),
                "shape": (self.N, self.M, self.L)}

    def load_state_dict(self, st, restore_rng: bool = True):
        if self.plan is None:
            raise _ffi.ArgumentError(-1, "load_state_dict is the plan path's")
        if tuple(st["shape"]) != (self.N, self.M, self.L):
            raise _ffi.ArgumentError(-1, f"the checkpoint is of a {tuple(st['shape'])} problem, this one is {(self.N, self.M, self.L)}")
        self.plan.load_state(st["plan"])
        self._Gg[: st["Gg"].numel()].copy_(st["Gg"][: self._Gg.numel()])
        self._kl.copy_(st["kl"])
        self.nsweeps = int(st["nsweeps"])
        self._sites_of = None  # (the checkpoint holds no per-point sites: loo() re-forms them)
        if restore_rng:
            self.ctx.set_seed(int(st["seed"]))
            self.ctx.sweep = int(st["sweep_counter"])

    def elbo_entering(self):
        """aug_elbo (examples/bernoulli/script.jl:65-70) of the q(v) that ENTERED the last sweep, at no extra pass over the
        features (``track_elbo=True``): the per-point terms expected_logtilt - aux_kldivergence rode that sweep's per-point kernel
        (summed over ranks by the sweep's one all-reduce), and KL(q(v) || p(v)) rode the update that produced that q(v).
        After sweep k this is the ELBO after k - 1 updates: a convergence monitor that lags one sweep."""
        if not self.track_elbo or self.nsweeps == 0:
            raise _ffi.ArgumentError(-1, "elbo_entering needs track_elbo=True and at least one sweep")
        self.check()
        # sweep k (1-based) wrote kl[(k - 1) & 1] for its NEW q(v); the q(v) that entered it was made by sweep k - 1 -> kl[k & 1]
        # (k = 1: the initial N(0, I), whose slot still holds 0)
        return float(self._elbo_terms.item()) - float(self._kl[self.nsweeps & 1].item())

    def run(self, niter: int = 10):
        for _ in range(niter):
            self.sweep()
        self.check()
        return self.m, self.S

    def elbo(self):
        """aug_elbo of examples/bernoulli/script.jl:65-70 for the current q(v):
        expected_logtilt(lik, qΩ, y, qf) - aux_kldivergence(lik, qΩ, y) - KL(q(v) || p(v)), with qf the current
        marginals and qΩ = aux_posterior(lik, y, qf) (float64 operator kernels; the Gaussian KL from the factor).  Local points
        only: with N sharded, sum the first two terms over ranks and count the KL once."""
        from . import operators as ops

        torch = _torch()
        qf = _point_major(*self.marginals(), self.L)
        y = self.y.to(torch.float64) if self.lik.ykind == "real" else self.y
        qΩ = ops.aux_posterior(self.lik, y, qf, ctx=self.ctx)
        elt = ops.expected_logtilt(self.lik, qΩ, y, qf, ctx=self.ctx)
        kl_aux = ops.aux_kldivergence(self.lik, qΩ, y, ctx=self.ctx)
        return elt - kl_aux - self._kl_v()

    def _kl_v(self):
        """KL(q(v) || p(v)) of the current q(v): from the factor on the plan path, the last update's own value otherwise."""
        torch = _torch()
        if self.plan is not None:
            self.check()
            Ut = torch.triu(self.A_work)  # U' (row-major view of the column-major lower triangle)
            m = (Ut @ self.v.unsqueeze(-1)).squeeze(-1)
            return 0.5 * float(((Ut * Ut).sum() + (m * m).sum() - self.L * self.M + self.plan.logdet.sum()).item())
        return float(self._kl[0].item())  # of the last agpl_gaussian_update (its kl_out)

    def expected_loglik(self, grad: bool = True):
        """Σᵢ E_{q(fᵢ)} log p(yᵢ | fᵢ; θ) over the points of every rank, at the current q(v), and its gradient for the logarithms of
        the likelihood's parameters (``operators.expected_loglik`` on ``marginals()``, converted to the float64 point-major layout
        on the device): ``(ell, grad)``, a float and a float64 host tensor [P] (None without ``grad``).  With ``group`` set the
        1 + P numbers are all-reduced over it.  The categorical kinds are refused."""
        from . import operators as ops

        mu, var = _point_major(*self.marginals(), self.L)
        sums, _, _ = ops._expected_loglik(self.lik, mu, var, self.y, self.ctx, False, grad)
        _all_reduce_sum(sums, self.group)
        sums = sums.cpu()
        return float(sums[0]), (sums[1:].clone() if grad else None)

    def bound(self):
        """The un-augmented sparse-GP bound F = Σᵢ E_{q(fᵢ)} log p(yᵢ | fᵢ) - KL(q(v) || p(v)) of the current q(v): the first term
        from ``expected_loglik`` (all ranks' points), the KL from the quantities ``elbo()`` uses.  The augmentation only loosens
        it: ``bound() >= elbo()`` (on one rank) -- up to the Student-t / Laplace quirks of DESIGN.md 7b, which ``elbo()`` follows
        as the reference codes them and this bound does not have."""
        return self.expected_loglik(grad=False)[0] - self._kl_v()

    def _loo_cavity(self):
        """``Plan.loo_cavity`` at the sites behind the current q(v).  After a ``sweep()`` of an object made with ``keep_points=True``
        those are ``self.gamma`` / ``self.beta``: the pass that made them also made the G, g of the update.  Otherwise (no sweep has
        run on this object, e.g. after ``load_state_dict``; or the points' values are not kept) ONE pass like ``accumulate()``'s is
        run first, at the current q(v), into buffers of its own -- the sweep's G, g, gamma, beta and ELBO terms stay untouched.  Its
        sites are those of the NEXT update: at a converged q(v) they are the current ones up to the float32 round-off of the pass,
        before convergence they differ by what one more sweep would change."""
        if self.plan is None:
            raise _ffi.ArgumentError(-1, "the leave-one-out cavity is the plan path's (the default arithmetic)")
        self.check()
        if self.gamma is not None and self.nsweeps > 0 and self._sites_of == self.nsweeps:
            gamma, beta = self.gamma, self.beta
        else:
            gamma, beta, *_ = self._fresh_pass()
        return self.plan.loo_cavity(gamma, beta, self.mu0)

    def loo(self, nsamples: int = 0, sweep: int | None = None):
        """Leave-one-out predictive densities of the observations the model was fitted to, from the cavity of the current q(v)
        (``Plan.loo_cavity``; the sites: ``_loo_cavity`` -- ``self.gamma`` / ``self.beta`` of the last sweep with
        ``keep_points=True``, else one pass like ``accumulate()``'s is run first to obtain them, which leaves the sweep's state as it
        is).  Returns a ``LooResult``: ``logp`` float64 [N], log p(yᵢ | y₋ᵢ) = ``operators.predictive`` at the cavity with this rank's
        y (``nsamples``, ``sweep``: its Monte Carlo arguments, categorical only); ``elpd``: Σᵢ logp, agpl_predictive's device sum
        (two-level, fixed order) of the same call; ``leverage`` float64 [N] or [N, L]; ``p_eff``: Σᵢ h per latent, a float64 host
        tensor [L]; ``n_bad``: the pairs without a cavity (their logp is NaN, and so is elpd).  With ``group`` set, ``elpd``, ``p_eff``
        and ``n_bad`` are all-reduced over it (one float64 SUM of the 2 + L numbers: each rank's device sums, then the ranks' sum)."""
        from . import operators as ops

        torch = _torch()
        mu, var, lev, lev_sum, n_bad, _ = self._loo_cavity()
        _, _, logp, total = ops._predictive(self.lik, (mu, var), self.y, nsamples, sweep, self.ctx, want_points=True, want_sum=True)
        sums = torch.cat([total, lev_sum, torch.tensor([float(n_bad)], dtype=torch.float64, device=total.device)])
        _all_reduce_sum(sums, self.group)
        sums = sums.cpu()
        return LooResult(logp, float(sums[0]), lev, sums[1:1 + self.L].clone(), int(sums[-1]))

    def loo_predict_y(self):
        """Mean and variance of yᵢ under the leave-one-out cavity (``operators.predictive`` at ``Plan.loo_cavity``): ``(mean, var)``
        float64 [N]; categorical: ``(probs [N, K], None)``.  The sites as ``loo`` takes them."""
        from . import operators as ops

        mu, var = self._loo_cavity()[:2]
        if self.lik.ykind == "i32x2":  # the moments need the training trials: column 1 of the stored y (column 0 is not read)
            return ops._predictive(self.lik, (mu, var), self.y, 0, None, self.ctx, want_logp=False)[:2]
        return ops.predictive(self.lik, (mu, var), ctx=self.ctx)[:2]

    def loo_cdf(self):
        """``(cdf, sf)`` of the leave-one-out predictive at the observations, float64 [N]: P(Y ≤ yᵢ | y₋ᵢ) is the LOO probability
        integral transform (``operators.predictive_cdf`` at ``Plan.loo_cavity``; the categorical kinds are refused there).  The
        sites as ``loo`` takes them."""
        from . import operators as ops

        mu, var = self._loo_cavity()[:2]
        return ops.predictive_cdf(self.lik, (mu, var), self.y, ctx=self.ctx)

    def natural_parameters(self):
        """(Lambda_v, eta_v) = (I + G, g): the whitened natural parameters of q(v)."""
        torch = _torch()
        eye = torch.eye(self.M, dtype=torch.float64, device=self.G.device)
        return self.G + eye, self.g

    def marginals(self):
        """q(f_i) for the current (m, S): (mu, var) float32 [L][N]."""
        torch = _torch()
        mu = torch.empty((self.L, self.N), dtype=torch.float32, device=self.y.device)
        var = torch.empty_like(mu)
        if self.plan is not None:
            self.plan.call("agpl_marginals_plan", _ptr(self.mu0), _ptr(mu), _ptr(var))
            return mu, var
        self.ctx.call("agpl_marginals", C.c_int64(self.N), C.c_int32(self.M), C.c_int32(self.L), _ptr(self.Phi),
                      _ptr(self.kdiag), _ptr(self.mu0), _ptr(self.Wpack), _ptr(self.alpha), _ptr(mu), _ptr(var))
        return mu, var


def learn_hyperparameters(lik, x, y, z, lengthscale, variance: float = 1.0, kernel="se", nouter: int = 10, nsweeps: int = 3,
                          lr: float = 0.05, jitter: float = 1e-8, mu0=None, ctx: Context | None = None, group=None,
                          learn_inducing: bool = False, lr_z: float | None = None, learn_likelihood: bool = False,
                          lr_lik: float | None = None):
    """Learn the ARD lengthscales and the variance of a stationary kernel by ascent on the sweep's bound.  Each outer step: ``nsweeps``
    CAVI sweeps, one ``hyper_grad``, one Adam step (beta 0.9 / 0.999, eps 1e-8) on (log lengthscale, log variance); the plan is then
    rebuilt for the new kernel INTO THE SAME STORAGE and q(v) carried over (``Plan.state`` / ``load_state``: whitened coordinates).
    Returns ``(cavi, trace)``: the final ``SparseCAVI`` and ``{"log_lengthscale": [nouter + 1, D], "log_variance": [nouter + 1],
    "elbo": [nouter]}`` -- the hyperparameters before each step and after the last; ``elbo()`` (this rank's points) at each gradient,
    i.e. after that step's sweeps at that step's hyperparameters.
    ``learn_inducing``: the same Adam step also moves the inducing inputs (``hyper_grad(inducing=True)``: one pass over the points
    for both gradients).  The parameter is z itself, in the inputs' units, with step ``lr_z`` (default ``lr``): standardise the
    inputs, so that one step size suits every coordinate.  The trace gains ``"z"``: [nouter + 1, M, D].
    ``learn_likelihood``: the logarithms of the likelihood's own parameters (Student-t nu and sigma, Laplace beta, negative-binomial
    r, the Poisson / heteroscedastic lambda) join the Adam vector with step ``lr_lik`` (default ``lr``).  Their gradient is that of
    Σ E_q log p(y | f) (``SparseCAVI.expected_loglik``: the un-augmented bound's likelihood term, not ``elbo()``'s), taken in the same
    outer step as ``hyper_grad``; the next plan's object gets ``dataclasses.replace(lik, ...)``.  The trace gains ``"lik"``:
    [nouter + 1, P] log-parameters and ``"ell"``: [nouter].  A likelihood without parameters or a categorical one: ArgumentError."""
    torch = _torch()
    if learn_likelihood and not getattr(lik, "_param_names", ()):
        raise _ffi.ArgumentError(-1, f"learn_likelihood: {type(lik).__name__} has no parameter that expected_loglik differentiates")
    D = 1 if x.dim() == 1 else int(x.shape[1])
    theta = torch.cat([_lengthscales(lengthscale, D), torch.tensor([float(variance)], dtype=torch.float64)]).log()
    make = lambda th, zz, mem, lk=lik: SparseCAVI.from_inputs(lk, x, y, zz, th[:-1].exp(), float(th[-1].exp()), jitter, mu0=mu0, ctx=ctx,
                                                              group=group, kernel=kernel, keep_inputs=True, storage=mem)
    # the parameters of the Adam step: theta, then (learn_inducing) z itself, on the host as theta is; one step size per block
    par, step = theta, lr
    if learn_inducing:
        zh = z.detach().to(torch.float64).cpu().reshape(-1, D)
        par = torch.cat([theta, zh.reshape(-1)])
        step = torch.cat([torch.full_like(theta, lr), torch.full((zh.numel(),), float(lr if lr_z is None else lr_z), dtype=torch.float64)])
    if learn_likelihood:  # the last P entries of the Adam vector
        names = lik._param_names
        tl = torch.tensor([float(getattr(lik, k)) for k in names], dtype=torch.float64).log()
        if not torch.is_tensor(step):
            step = torch.full_like(par, lr)
        par = torch.cat([par, tl])
        step = torch.cat([step, torch.full_like(tl, float(lr if lr_lik is None else lr_lik))])
    cavi = make(theta, z, None)
    m1, m2 = torch.zeros_like(par), torch.zeros_like(par)
    trace = {"log_lengthscale": [theta[:-1].clone()], "log_variance": [float(theta[-1])], "elbo": []}
    if learn_inducing:
        trace["z"] = [zh.clone()]
    if learn_likelihood:
        trace["lik"], trace["ell"] = [tl.clone()], []
    for it in range(1, nouter + 1):
        for _ in range(nsweeps):
            cavi.sweep()
        gr = cavi.hyper_grad(inducing=True) if learn_inducing else cavi.hyper_grad()
        trace["elbo"].append(cavi.elbo())
        grad = torch.cat([gr["log_lengthscale"], torch.tensor([gr["log_variance"]], dtype=torch.float64)])
        if learn_inducing:
            grad = torch.cat([grad, gr["z"].reshape(-1)])
        if learn_likelihood:
            ell, gl = cavi.expected_loglik()
            trace["ell"].append(ell)
            grad = torch.cat([grad, gl])
        par, m1, m2 = _adam_step(par, grad, m1, m2, it, step)
        theta = par[: D + 1]
        trace["log_lengthscale"].append(theta[:-1].clone())
        trace["log_variance"].append(float(theta[-1]))
        if learn_inducing:
            zh = par[D + 1:par.numel() - (len(names) if learn_likelihood else 0)].reshape(-1, D)
            trace["z"].append(zh.clone())
        if learn_likelihood:
            tl = par[par.numel() - len(names):]
            trace["lik"].append(tl.clone())
            lik = dataclasses.replace(lik, **{k: float(v) for k, v in zip(names, tl.exp())})
        st, mem, nsw = cavi.plan.state(), cavi.plan.mem, cavi.nsweeps
        cavi.plan.close()
        cavi = make(theta, zh.to(z.device) if learn_inducing else z, mem, lik)
        cavi.plan.load_state(st)
        cavi.nsweeps = nsw
    trace["log_lengthscale"] = torch.stack(trace["log_lengthscale"])
    if learn_inducing:
        trace["z"] = torch.stack(trace["z"])
    if learn_likelihood:
        trace["lik"] = torch.stack(trace["lik"])
    return cavi, trace


def learn_likelihood(cavi, nouter: int = 10, nsweeps: int = 3, lr: float = 0.05):
    """Learn the likelihood's own parameters of a ``SparseCAVI`` with the kernel fixed: each outer step runs ``nsweeps`` sweeps, takes
    ``cavi.expected_loglik()`` and makes one Adam ascent step (beta 0.9 / 0.999, eps 1e-8) on the log-parameters.  No plan is rebuilt:
    the sweep forms its descriptor from ``cavi.lik`` at every pass, so ``cavi.lik`` is replaced (``dataclasses.replace``) and nothing
    else.  Returns ``{"lik": [nouter + 1, P] log-parameters before each step and after the last, "ell": [nouter]}``.  A likelihood
    without parameters or a categorical one: ArgumentError."""
    torch = _torch()
    names = getattr(cavi.lik, "_param_names", ())
    if not names:
        raise _ffi.ArgumentError(-1, f"learn_likelihood: {type(cavi.lik).__name__} has no parameter that expected_loglik differentiates")
    par = torch.tensor([float(getattr(cavi.lik, k)) for k in names], dtype=torch.float64).log()
    m1, m2 = torch.zeros_like(par), torch.zeros_like(par)
    trace = {"lik": [par.clone()], "ell": []}
    for it in range(1, nouter + 1):
        for _ in range(nsweeps):
            cavi.sweep()
        ell, grad = cavi.expected_loglik()
        trace["ell"].append(ell)
        par, m1, m2 = _adam_step(par, grad, m1, m2, it, lr)
        trace["lik"].append(par.clone())
        cavi.lik = dataclasses.replace(cavi.lik, **{k: float(v) for k, v in zip(names, par.exp())})
    trace["lik"] = torch.stack(trace["lik"])
    return trace


def nystrom_residual(Phi, kxx, ctx: Context | None = None):
    """d_i = k_ii - |phi_i|^2 (agpl_feature_residual: float64 accumulation), the `resid` of a plan / `kdiag` of the sweeps."""
    torch = _torch()
    ctx = ctx or default_context()
    Phi = _prep(Phi, torch.float32, "Phi")
    N, M = Phi.shape
    kxx = _prep(kxx, torch.float32, "kxx")
    out = torch.empty(N, dtype=torch.float32, device=Phi.device)
    ctx.call("agpl_feature_residual", C.c_int64(N), C.c_int32(M), _ptr(Phi), _ptr(kxx), _ptr(out))
    return out


class SparseGibbs:
    """Gibbs sweeps of the sparse model (``gibbs_sample`` of examples/bernoulli/script.jl:76-87 restated for M
    inducing coordinates in the whitened basis):

        f_i | v  ~ N(phi_i' v, d_i)            (agpl_gibbs_pass: projection + noise, per-point Philox stream)
        Ω_i | f_i ~ aux_full_conditional       (aux_sample!, same stream)
        v | Ω    ~ N(m, S), S = (I + G)^-1, m = S g,  G = Phi Diag(γ(Ω)) Phi', g = Phi β(Ω)   (agpl_gibbs_draw_v)

    N is sharded over ``group`` exactly as in SparseCAVI: (G, g) are all-reduced, every rank draws the identical v
    (same Philox key / counter: every rank's Context must carry the same seed and be at the same draw counter).
    ``point_offset`` = global index of this rank's first point (``shard_range(N, rank, world)[0]``): the per-point
    streams are keyed on the GLOBAL point index, so the sharded chain is the single-process chain.
    Real-valued y must be float64 here (the Gibbs operators are Float64).
    """

    def __init__(self, lik, Phi, kdiag, y, mu0=None, ctx: Context | None = None, group=None, keep_points=False,
                 accumulate_precision: str = "auto", point_offset: int = 0, plan: "Plan | None" = None):
        """``accumulate_precision``: "f16x2" (the plan's split-float16 image accumulation; "auto"; any feature count) or "f32"
        (agpl_gibbs_pass: float32-input MFMA, feature count a multiple of 128).  ``plan``: the plan of a SparseCAVI over the same
        features (its accumulate image and residual are shared); by default a plan without the marginal image is built here."""
        torch = _torch()
        if accumulate_precision == "auto":
            accumulate_precision = "f16x2"
        if accumulate_precision not in ("f32", "f16x2"):
            raise _ffi.ArgumentError(-1, "accumulate_precision must be 'auto', 'f32' or 'f16x2'")
        Phi = _prep(Phi, torch.float32, "Phi")
        if accumulate_precision == "f32" and Phi.shape[1] % PAD:
            raise _ffi.ArgumentError(-1, f"the float32-input kernels need a feature count that is a multiple of {PAD} (got {Phi.shape[1]}; "
                                         "zero-pad, or accumulate_precision='f16x2')")
        self._setup(lik, ctx or default_context(), Phi, _prep(kdiag, torch.float32, "kdiag"), plan, y, mu0, group, keep_points,
                    point_offset, acc_split=1 if accumulate_precision == "f16x2" else 0)

    def _setup(self, lik, ctx, Phi, kdiag, plan, y, mu0, group, keep_points, point_offset, acc_split=1):
        """What both constructors end in, and the one place that names the attributes of a SparseGibbs.  ``Phi`` (float32 features)
        or a ``plan`` made from inputs (``Phi`` is None); with features and ``acc_split``, ``plan`` may be a plan of the same
        features to share, else one is made here.  Ends with the prior draw of v."""
        torch = _torch()
        self.ctx, self.lik, self.acc_split = ctx, lik, acc_split
        self.Phi, self.kdiag = Phi, kdiag
        self.N, self.M = (plan.N, plan.M) if Phi is None else Phi.shape
        self.L = lik._nlatent
        self.y = _prep_y(lik, y, torch.float64)
        self.mu0 = _prep(mu0, torch.float32, "mu0")
        self.group = group
        dev = plan.mem.device if Phi is None else Phi.device
        L, M = self.L, self.M
        f64 = torch.float64
        self.plan = None
        if acc_split:
            if plan is not None and (plan.N, plan.M, plan.L) != (self.N, M, L):
                raise _ffi.ArgumentError(-1, "the plan was created for another problem size")
            if plan is not None and plan.ctx is not ctx:
                # the pass runs on the PLAN's context (its seed, its point offset): a plan from another Context would draw that
                # context's Philox streams while this object sets the offset on its own
                raise _ffi.ArgumentError(-1, "the plan belongs to another Context: pass ctx=plan.ctx (or build the plan on this one)")
            self.plan = plan if plan is not None else Plan(Phi, kdiag, L, ctx, flags=Plan.NO_MARGINALS)
        self._Gg, self.G, self.g = natural_parameter_buffers(L, M, dev)
        self.v = torch.empty((L, M), dtype=f64, device=dev)
        self.m = torch.empty((L, M), dtype=f64, device=dev)
        self.point_offset = int(point_offset)
        if group is not None and self.point_offset == 0 and _dist().get_rank(group) != 0:
            raise _ffi.ArgumentError(-1, "SparseGibbs(group=...) needs point_offset = the global index of this "
                                         "rank's first point on every rank but the first")
        self.f = self.omega = self.n = None
        if keep_points:
            Lo = 1 if lik.kind == 7 else L
            self.f = torch.empty((self.N, L), dtype=f64, device=dev)
            self.omega = torch.empty((self.N, Lo), dtype=f64, device=dev)
            self.n = torch.zeros((self.N, Lo), dtype=torch.int64, device=dev)
        self.sweep_index = self.ctx.next_sweep()  # draw counter of the sweep in flight (taken from the Context)
        self._check_ranks_agree()
        self.draw()  # G = 0, g = 0: v ~ N(0, I), the prior draw (script.jl:89 `f = randn(N)`)

    @classmethod
    def from_inputs(cls, lik, x, y, z, lengthscale, variance: float = 1.0, jitter: float = 1e-8, mu0=None, ctx: Context | None = None,
                    group=None, keep_points=False, point_offset: int = 0, kernel="se"):
        """Gibbs sweeps of a stationary-kernel model from its raw inputs: a plan without the marginal image
        (``Plan.from_inputs(..., flags=Plan.NO_MARGINALS)``) and no float32 features.  ``kernel``: ``"se"``, ``"matern12"`` /
        ``"exponential"``, ``"matern32"``, ``"matern52"`` or ``("rq", alpha)``.
        ``select_inducing`` chooses z from the data."""
        kernel_kind(kernel)  # (refused before any device work)
        ctx = ctx or default_context()
        plan = Plan.from_inputs(x, z, lengthscale, variance, jitter, L=lik._nlatent, ctx=ctx, flags=Plan.NO_MARGINALS, kernel=kernel)
        self = cls.__new__(cls)
        self._setup(lik, ctx, None, plan.resid, plan, y, mu0, group, keep_points, point_offset)
        return self

    def _check_ranks_agree(self):
        """Every rank draws v itself: the ranks' Philox key (seed) and draw counter must be the same, or the ranks sample
        different chains behind an all-reduce that still "works".  One tiny MIN / MAX exchange at construction."""
        if self.group is None:
            return
        torch, dist = _torch(), _dist()
        dev = self.v.device if dist.get_backend(self.group) == "nccl" else "cpu"
        seed = int(self.ctx.seed) & 0xFFFFFFFFFFFFFFFF
        mine = torch.tensor([seed & 0xFFFFFFFF, seed >> 32, int(self.sweep_index)], dtype=torch.int64, device=dev)
        lo, hi = mine.clone(), mine.clone()
        dist.all_reduce(lo, op=dist.ReduceOp.MIN, group=self.group)
        dist.all_reduce(hi, op=dist.ReduceOp.MAX, group=self.group)
        if not bool((lo == hi).all()):
            raise _ffi.ArgumentError(-1, "SparseGibbs(group=...): the ranks' Contexts differ in seed or draw counter "
                                         f"(this rank: seed {seed}, sweep {self.sweep_index}); create every rank's "
                                         "Context with the same seed and use them for the same sequence of draws")

    def draw(self):
        """v ~ N(m, S) on the streams (seed, l M + a, sweep_index | 2^31): identical on every rank."""
        self.ctx.call("agpl_gibbs_draw_v", C.c_int32(self.M), C.c_int32(self.L), _ptr(self.G), _ptr(self.g),
                      C.c_void_p(0), C.c_uint32(self.sweep_index), _ptr(self.v), _ptr(self.m))

    def accumulate(self):
        """Point pass of one sweep on the streams (seed, point_offset + i, sweep_index)."""
        d = self.lik.desc()
        self.sweep_index = self.ctx.next_sweep()
        prev_offset = self.ctx.point_offset
        self.ctx.set_point_offset(self.point_offset)
        try:  # (a raising pass must not leave the context's point offset shifted for its other users)
            if self.plan is not None:  # the shipped path
                self.plan.call("agpl_gibbs_pass_plan", C.byref(d), _ptr(self.mu0), _ptr(self.y), _ptr(self.v),
                               C.c_uint32(self.sweep_index), _ptr(self.G), _ptr(self.g), _ptr(self.f), _ptr(self.omega),
                               _ptr(self.n), C.c_void_p(0))
            else:
                self.ctx.call("agpl_gibbs_pass", C.byref(d), C.c_int64(self.N), C.c_int32(self.M), _ptr(self.Phi),
                              _ptr(self.kdiag), _ptr(self.mu0), _ptr(self.y), _ptr(self.v), C.c_uint32(self.sweep_index),
                              _ptr(self.G), _ptr(self.g), _ptr(self.f), _ptr(self.omega), _ptr(self.n), C.c_void_p(0))
        finally:
            self.ctx.set_point_offset(prev_offset)

    def exchange(self):
        exchange_natural_parameters(self.G, self.g, self.group, flat=self._Gg)

    def state_dict(self):
        """Checkpoint of the chain (the reference's state is the (f, Ω) of examples/bernoulli/script.jl:89-90; here f and Ω are
        redrawn from v every sweep): the inducing draw v, and the context's Philox key and draw counter -- counter-based streams
        make the resumed chain the uninterrupted one, bit for bit."""
        self.ctx.synchronize()
        return {"v": self.v.detach().cpu().clone(), "m": self.m.detach().cpu().clone(), "seed": int(self.ctx.seed),
                "sweep_counter": int(self.ctx.sweep), "sweep_index": int(self.sweep_index), "point_offset": self.point_offset,
                "shape": (self.N, self.M, self.L)}

    def load_state_dict(self, st):
        if tuple(st["shape"]) != (self.N, self.M, self.L):
            raise _ffi.ArgumentError(-1, f"the checkpoint is of a {tuple(st['shape'])} problem, this one is {(self.N, self.M, self.L)}")
        self.ctx.synchronize()
        self.v.copy_(st["v"])
        self.m.copy_(st["m"])
        self.ctx.set_seed(int(st["seed"]))
        self.ctx.sweep = int(st["sweep_counter"])
        self.sweep_index = int(st["sweep_index"])
        self._check_ranks_agree()

    def sweep(self):
        self.accumulate()
        self.exchange()
        self.draw()
        return self.v

    def _se_plan(self, what):
        if self.plan is None or not self.plan.se:
            raise _ffi.ArgumentError(-1, f"{what} needs a SparseGibbs made by SparseGibbs.from_inputs")
        return self.plan

    def predict(self, x_s, chain, mu0_s=None, samples: bool = False):
        """The posterior of f at new inputs from a chain of this sampler (``run``'s output, [T, L, M]): the Gibbs samples turned into
        a posterior at x_te as examples/bernoulli/script.jl does after ``gibbs_sample``.  ``(mean, var, resid[, F])`` of
        ``Plan.predict_chain``.  Needs an object made by ``from_inputs``."""
        return self._se_plan("predict").predict_chain(chain, x_s, mu0_s, samples=samples)

    def sample_paths(self, chain, nfeatures: int = 2048, generator=None):
        """One pathwise function draw per draw of ``chain`` [T, L, M] (``run``'s output): each is a full posterior sample from the
        chain, the residual that ``predict``'s conditional means leave out included (``Plan.sample_paths(V=chain)``)."""
        return self._se_plan("sample_paths").sample_paths(V=chain, nfeatures=nfeatures, generator=generator)

    def sample_y(self, x_s, chain, mu0_s=None, nfeatures: int = 2048, generator=None, sweep: int | None = None):
        """One posterior-predictive draw of y at new inputs per draw of ``chain`` [T, L, M], for this object's likelihood:
        ``sample_paths(chain).sample_y`` (the residual included): [T, Ns] (categorical: one-hot [T, Ns, L])."""
        paths = self._se_plan("sample_y").sample_paths(V=chain, nfeatures=nfeatures, generator=generator)
        return paths.sample_y(self.lik, x_s, mu0_s, sweep=sweep)

    def predict_y(self, x_s, chain, y_s=None, mu0_s=None, nsamples: int = 0, sweep: int | None = None, trials=None):
        """p(y*) at new inputs as the mixture over the chain's draws (``Plan.predict_y_chain``): (mean, var, logp), float64 [Ns].
        ``trials`` [Ns]: required for ``BinomialTrialsLikelihood``, refused otherwise."""
        return self._se_plan("predict_y").predict_y_chain(self.lik, chain, x_s, y_s, mu0_s, nsamples=nsamples, sweep=sweep, trials=trials)

    def heldout_logp(self, x_s, y_s, chain, mu0_s=None, nsamples: int = 0, sweep: int | None = None, trials=None) -> float:
        """Σ log p(y_s | x_s) of held-out data under the chain's mixture (float64 sum on the device)."""
        if y_s is None:
            raise _ffi.ArgumentError(-1, "heldout_logp needs the observations y_s")
        logp = self._se_plan("heldout_logp").predict_y_chain(self.lik, chain, x_s, y_s, mu0_s, nsamples=nsamples, sweep=sweep, trials=trials)[2]
        return float(logp.sum().item())

    def run(self, nsamples: int = 200):
        """Returns the [nsamples, L, M] chain of inducing draws."""
        torch = _torch()
        out = torch.empty((nsamples, self.L, self.M), dtype=torch.float64, device=self.v.device)
        for t in range(nsamples):
            out[t] = self.sweep()
        return out


class DenseGibbs:
    """``gibbs_sample(fz, f, Ω)`` of examples/bernoulli/script.jl:76-87 (studentt/script.jl is the same loop):
    full-rank Gibbs over N points with a dense prior covariance K [N, N] float64 (BASELINE config C5).
    One float64 Cholesky of I + D^1/2 K D^1/2 per sweep instead of the reference's two inverses + Cholesky."""

    def __init__(self, lik, K, y, mu0=None, f0=None, ctx: Context | None = None):
        torch = _torch()
        self.ctx = ctx or default_context()
        self.lik = lik
        self.K = _prep(K, torch.float64, "K")
        self.N = self.K.shape[0]
        self.y = _prep_y(lik, y, torch.float64)
        self.mu0 = _prep(mu0, torch.float64, "mu0")
        dev = self.K.device
        self.Lk = torch.empty_like(self.K)
        self.ctx.call("agpl_dense_cholesky", C.c_int64(self.N), _ptr(self.K), _ptr(self.Lk))  # script.jl:77
        self.B = torch.empty_like(self.K)
        self.f = (torch.zeros(self.N, dtype=torch.float64, device=dev) if f0 is None
                  else _prep(f0, torch.float64, "f0").clone())
        self.omega = torch.empty(self.N, dtype=torch.float64, device=dev)
        self.n = torch.zeros(self.N, dtype=torch.int64, device=dev) if lik.kind == 5 else None
        self.sweep_index = None

    def sweep(self):
        d = self.lik.desc()
        self.sweep_index = self.ctx.next_sweep()
        self.ctx.call("agpl_dense_gibbs_step", C.byref(d), C.c_int64(self.N), _ptr(self.K), _ptr(self.Lk),
                      _ptr(self.mu0), _ptr(self.y), _ptr(self.f), _ptr(self.B), C.c_uint32(self.sweep_index),
                      _ptr(self.omega), _ptr(self.n))
        return self.f

    def run(self, nsamples: int = 200):
        torch = _torch()
        out = torch.empty((nsamples, self.N), dtype=torch.float64, device=self.K.device)
        for t in range(nsamples):
            out[t] = self.sweep()
        return out
