"""ctypes binding of libagpl.so (include/agpl.h) and its extension libraries.  No fallback: if a HIP library is missing or fails
to load, every operator raises -- there is no CPU path in the product."""
from __future__ import annotations

import ctypes as C
import functools
import os
import subprocess
from typing import NamedTuple

_HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(_HERE, "csrc")

AGPL_OK = 0
ERR_INVALID_ARGUMENT, ERR_DOMAIN, ERR_UNSUPPORTED, ERR_HIP, ERR_NOT_POSDEF, ERR_OOM = -1, -2, -3, -4, -5, -6
F32, F64 = 0, 1
# agpl_kernel_kind of include/agpl_kernels.h
KERNEL_SE, KERNEL_MATERN12, KERNEL_MATERN32, KERNEL_MATERN52, KERNEL_RQ = 0, 1, 2, 3, 4
KERNEL_PERIODIC = 6  # (5 is no kind: include/agpl_kernels.h)
KERNEL_SE_PERIODIC = 8  # (7 is no kind either)
KERNEL_SE_COSINE = 10  # (nor is 9)


class Library(NamedTuple):
    """One shared library of the product.  For a record with key K and loader f the module has the public names K_LIB_PATH (the
    file, beside this module), K_SYMBOLS (its exported symbols) and f() (the loaded library); libagpl.so's own key is empty."""
    key: str
    loader: str
    file: str
    header: str  # under include/
    symbols: list  # every export; tests/test_abi_libraries.py checks the list against the header and the .so
    types: dict  # symbol -> (restype, argtypes) as set on load; None, or a symbol without an entry, is left to ctypes' default


def _typed(restype, **argtypes):
    """A library in which every export returns `restype` and has its argument types set."""
    return dict(symbols=list(argtypes), types={name: (restype, a) for name, a in argtypes.items()})


_P, _I64, _I32, _U32, _D = C.c_void_p, C.c_int64, C.c_int32, C.c_uint32, C.c_double

# The set of libraries, stated once: libagpl.so first, then its extensions (each resolves against it) in the order they were added.
LIBRARIES = [
    Library("", "lib", "libagpl.so", "agpl.h", [
        "agpl_version", "agpl_ctx_create", "agpl_ctx_destroy", "agpl_ctx_set_stream", "agpl_ctx_set_seed", "agpl_ctx_set_point_offset",
        "agpl_ctx_synchronize", "agpl_last_error",
        # the operator surface of src/AugmentedGPLikelihoods.jl:18-30
        "agpl_aux_sample", "agpl_rand_polyagamma", "agpl_potential_precision", "agpl_aux_posterior",
        "agpl_expected_potential_precision", "agpl_logtilt", "agpl_aux_prior_logpdf", "agpl_aug_loglik", "agpl_expected_logtilt",
        "agpl_aux_kldivergence", "agpl_expected_aug_loglik",
        # the sweep at SURVEY.md 8(d)'s float32-input arithmetic
        "agpl_marginals", "agpl_accumulate", "agpl_gaussian_update", "agpl_cavi_pass", "agpl_gibbs_pass", "agpl_gibbs_draw_v",
        # the shipped sweep: factor-form update + the plan (split-float16 images)
        "agpl_gaussian_factor", "agpl_feature_residual", "agpl_plan_bytes", "agpl_plan_create", "agpl_plan_destroy", "agpl_plan_info",
        "agpl_plan_state", "agpl_cavi_pass_plan", "agpl_plan_update", "agpl_marginals_plan", "agpl_gibbs_pass_plan",
        # full-rank Gibbs step, multi-GPU exchange, features / synthetic data, diagnostics
        "agpl_dense_cholesky", "agpl_dense_gibbs_step", "agpl_allreduce_nat", "agpl_se_features", "agpl_transform_features",
        "agpl_synth_xy", "agpl_probe_mfma", "agpl_timing", "agpl_debug_force_factor_rescue",
    ], {"agpl_last_error": (C.c_char_p, [_P]), "agpl_plan_bytes": (_I64, None)}),
    # plans from raw squared-exponential inputs, prediction
    Library("SE_", "se_lib", "libagpl_se.so", "agpl_se.h",
            ["agpl_plan_se_bytes", "agpl_plan_create_se", "agpl_plan_predict", "agpl_plan_features"], {"agpl_plan_se_bytes": (_I64, None)}),
    # predictive moments of y and held-out log density
    Library("PR_", "pr_lib", "libagpl_predictive.so", "agpl_predictive.h", ["agpl_predictive"], {}),
    # a chain of inducing draws projected at new inputs
    Library("CH_", "chain_lib", "libagpl_chain.so", "agpl_chain.h", ["agpl_plan_predict_chain"], {}),
    # plans from raw inputs for Matern / rational-quadratic kernels
    Library("KN_", "kernels_lib", "libagpl_kernels.so", "agpl_kernels.h", ["agpl_plan_create_stationary"], {}),
    # the posterior covariance between new inputs
    Library("JT_", "joint_lib", "libagpl_joint.so", "agpl_joint.h", **_typed(
        _I32, agpl_plan_predict_cov=[_P, _I64, _P, _I64, _P, _P, _I64])),
    # k-means inducing inputs, shard-exact
    Library("IN_", "inducing_lib", "libagpl_inducing.so", "agpl_inducing.h", **_typed(
        _I32,
        agpl_kmeans_quanta=[_P, _D, _I64, _I32, _P, _P],
        agpl_kmeans_seed=[_P, _I64, _I64, _I64, _I32, _I32, _P, _P, _P],
        agpl_kmeans_bound=[_P, _I64, _I32, _P, _P, _P],
        agpl_kmeans_step=[_P, _I64, _I64, _I32, _I32, _P, _P, _P, _D, _P, _P],
        agpl_kmeans_centres=[_P, _I64, _I32, _I32, _P, _D, _P, _P, _P],
        agpl_select_inducing_kmeans=[_P, _I64, _I32, _I32, _P, _P, _I32, _P, _P, _P])),
    # the bound's gradient for log lengthscales and log variance
    Library("HY_", "hyper_lib", "libagpl_hyper.so", "agpl_hyper.h", **_typed(_I32, agpl_plan_hyper_grad=[_P, _I64] + [_P] * 7)),
    # the bound's gradient for the inducing inputs, with the hyperparameters'
    Library("ZG_", "zgrad_lib", "libagpl_zgrad.so", "agpl_zgrad.h", **_typed(_I32, agpl_plan_inducing_grad=[_P, _I64] + [_P] * 8)),
    # pathwise draws of the posterior function at new inputs
    Library("PW_", "pathwise_lib", "libagpl_pathwise.so", "agpl_pathwise.h", **_typed(
        _I32, agpl_plan_sample_paths=[_P, _I32, _P, _I32, _P, _P, _P, _P, _I64, _P, _P, _P])),
    # posterior-predictive draws of y from a block of function draws
    Library("SY_", "sample_y_lib", "libagpl_sampley.so", "agpl_sample_y.h", **_typed(
        _I32, agpl_sample_y=[_P, _P, _I32, _I64, _I64, _P, _I64, _I32, _U32, _P])),
    # E_q log p(y | f) and its gradient for the likelihood's parameters
    Library("LG_", "likgrad_lib", "libagpl_likgrad.so", "agpl_likgrad.h", **_typed(
        _I32, agpl_expected_loglik=[_P, _P, _I64, _P, _P, _P, _P, _P, _P, _P])),
    # the posterior of d f / d x at new inputs
    Library("GR_", "grad_lib", "libagpl_grad.so", "agpl_grad.h", **_typed(_I32, agpl_plan_predict_grad=[_P, _I64, _P, _P, _P])),
    # P(Y <= y), P(Y > y) and the quantiles of the predictive of y
    Library("QT_", "quantile_lib", "libagpl_quantile.so", "agpl_quantile.h", **_typed(
        _I32,
        agpl_predictive_cdf=[_P, _P, _I64, _P, _P, _P, _P, _P],
        agpl_predictive_quantile=[_P, _P, _I64, _P, _P, _I32, _P, _P])),
    # greedy conditional-variance inducing inputs, shard-exact
    Library("GV_", "greedy_lib", "libagpl_greedy.so", "agpl_greedy.h", **_typed(
        _I32,
        agpl_greedy_bytes=[_I64, _I32, _P],
        agpl_greedy_begin=[_P, _I64, _I64, _I64, _I32, _I32, _P, _D, _P, _I64, _P],
        agpl_greedy_pivot=[_P, _I64, _I64, _I64, _I32, _I32, _I32, _P, _P, _I64, _P, _P],
        agpl_greedy_step=[_P, _I64, _I64, _I64, _I32, _I32, _I32, _D, _I32, _P, _P, _D, _P, _P, _P, _I64, _P, _P],
        agpl_select_inducing_greedy=[_P, _I64, _I32, _I32, _I32, _D, _P, _P, _D, _D, _P, _I64, _P, _P, _P])),
    # the leave-one-out cavity of a plan's q(v) at the training points
    Library("LO_", "loo_lib", "libagpl_loo.so", "agpl_loo.h", ["agpl_plan_loo_bytes", "agpl_plan_loo"], {
        "agpl_plan_loo_bytes": (_I64, [_I64, _I32]),
        "agpl_plan_loo": (_I32, [_P, _P, _P, _P, _P, _I64, _P, _P, _P, _P, _P])}),
]


class LikDesc(C.Structure):
    _fields_ = [("kind", C.c_int32), ("nlatent", C.c_int32), ("p", C.c_double * 4),
                ("logtheta", C.POINTER(C.c_double))]


class AGPLError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"libagpl status {code}: {msg}")
        self.code = code


class ArgumentError(AGPLError, ValueError):  # Julia ArgumentError
    pass


class DomainError(AGPLError, ValueError):  # Julia DomainError
    pass


class PosDefException(AGPLError, ArithmeticError):  # LinearAlgebra.PosDefException
    pass


_ERR_TYPES = {ERR_INVALID_ARGUMENT: ArgumentError, ERR_DOMAIN: DomainError, ERR_NOT_POSDEF: PosDefException}


def _path(rec: Library) -> str:
    """The file a library is loaded from: the public name's value now (tools assign LIB_PATH, LG_LIB_PATH before the first call)."""
    return globals()[rec.key + "LIB_PATH"]


def build(force: bool = False) -> str:
    """Compile libagpl.so and its extensions for gfx950 in-tree (hipcc cross-compiles without a GPU)."""
    srcs = [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith((".hip", ".h"))]
    srcs += [os.path.join(os.path.dirname(_HERE), "include", rec.header) for rec in LIBRARIES]
    stale = not all(os.path.exists(_path(rec)) for rec in LIBRARIES) or any(os.path.getmtime(s) > os.path.getmtime(LIB_PATH) for s in srcs)
    if force or stale:
        subprocess.check_call(["make", "-C", CSRC, "-s", "-j4"])
    return LIB_PATH


_loaded = {}


def _load(rec: Library) -> C.CDLL:
    so = _loaded.get(rec.key)
    if so is None:
        path = _path(rec)
        if rec is LIBRARIES[0]:
            if not os.path.exists(path):
                raise ImportError(
                    f"{path} is missing: the HIP extension has not been built "
                    "(run `python -c 'import __graft_entry__ as g; g.build()'`). There is no CPU fallback.")
            # torch bundles its own libamdhip64 / librocblas: load torch first so that libagpl.so's NEEDED
            # entries resolve (by SONAME) to the runtime already in the process.  Two HIP runtimes in one
            # process do not share a device context (hipGetDeviceCount fails in the second one).
            import torch  # noqa: F401
        else:
            lib()  # an extension is loaded after (and resolves against) libagpl.so
            if not os.path.exists(path):
                raise ImportError(f"{path} is missing: the HIP extension has not been built. There is no CPU fallback.")
        so = C.CDLL(path)
        for s in rec.symbols:
            getattr(so, s)  # raises AttributeError if the library does not export the ABI
        for s, (restype, argtypes) in rec.types.items():
            if restype is not None:
                getattr(so, s).restype = restype
            if argtypes is not None:
                getattr(so, s).argtypes = argtypes
        _loaded[rec.key] = so
    return so


# the public names of every record: LIB_PATH, SE_LIB_PATH ... LO_LIB_PATH; SYMBOLS, SE_SYMBOLS ... LO_SYMBOLS; lib(), se_lib() ... loo_lib()
for _rec in LIBRARIES:
    globals().update({_rec.key + "LIB_PATH": os.path.join(_HERE, _rec.file), _rec.key + "SYMBOLS": _rec.symbols,
                      _rec.loader: functools.partial(_load, _rec)})


def check(ctx_handle, rc):
    if rc != AGPL_OK:
        msg = lib().agpl_last_error(ctx_handle)
        msg = msg.decode() if msg else ""
        raise _ERR_TYPES.get(rc, AGPLError)(rc, msg)
