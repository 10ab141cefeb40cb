"""ctypes binding of libagpl.so (include/agpl.h).  No fallback: if the HIP library is missing or fails to
load, every operator raises -- there is no CPU path in the product."""
from __future__ import annotations

import ctypes as C
import os
import subprocess

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libagpl.so")
SE_LIB_PATH = os.path.join(_HERE, "libagpl_se.so")  # the squared-exponential extension (include/agpl_se.h)
PR_LIB_PATH = os.path.join(_HERE, "libagpl_predictive.so")  # the predictive distribution of y (include/agpl_predictive.h)
CH_LIB_PATH = os.path.join(_HERE, "libagpl_chain.so")  # the posterior of f from a chain of inducing draws (include/agpl_chain.h)
KN_LIB_PATH = os.path.join(_HERE, "libagpl_kernels.so")  # plans from raw inputs for the other stationary kernels (include/agpl_kernels.h)
JT_LIB_PATH = os.path.join(_HERE, "libagpl_joint.so")  # the joint posterior of f at new inputs (include/agpl_joint.h)
IN_LIB_PATH = os.path.join(_HERE, "libagpl_inducing.so")  # inducing inputs from the data by k-means (include/agpl_inducing.h)
HY_LIB_PATH = os.path.join(_HERE, "libagpl_hyper.so")  # the bound's gradient for the kernel hyperparameters (include/agpl_hyper.h)
ZG_LIB_PATH = os.path.join(_HERE, "libagpl_zgrad.so")  # the bound's gradient for the inducing inputs (include/agpl_zgrad.h)
PW_LIB_PATH = os.path.join(_HERE, "libagpl_pathwise.so")  # pathwise draws of the posterior function (include/agpl_pathwise.h)
SY_LIB_PATH = os.path.join(_HERE, "libagpl_sampley.so")  # posterior-predictive draws of y (include/agpl_sample_y.h)
LG_LIB_PATH = os.path.join(_HERE, "libagpl_likgrad.so")  # the expected log-likelihood and its gradient for the likelihood's parameters (include/agpl_likgrad.h)
GR_LIB_PATH = os.path.join(_HERE, "libagpl_grad.so")  # the posterior of the gradient of f at new inputs (include/agpl_grad.h)
QT_LIB_PATH = os.path.join(_HERE, "libagpl_quantile.so")  # the predictive distribution function of y and its quantiles (include/agpl_quantile.h)
GV_LIB_PATH = os.path.join(_HERE, "libagpl_greedy.so")  # inducing inputs by greedy conditional variance (include/agpl_greedy.h)
LO_LIB_PATH = os.path.join(_HERE, "libagpl_loo.so")  # the leave-one-out cavity at the training points (include/agpl_loo.h)
CSRC = os.path.join(_HERE, "csrc")

AGPL_OK = 0
ERR_INVALID_ARGUMENT, ERR_DOMAIN, ERR_UNSUPPORTED, ERR_HIP, ERR_NOT_POSDEF, ERR_OOM = -1, -2, -3, -4, -5, -6
F32, F64 = 0, 1

# exported symbols of include/agpl.h (tests/test_abi.py checks this list against the header and the .so)
SYMBOLS = [
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
]


# exported symbols of include/agpl_se.h (libagpl_se.so: plans from raw squared-exponential inputs, prediction)
SE_SYMBOLS = ["agpl_plan_se_bytes", "agpl_plan_create_se", "agpl_plan_predict", "agpl_plan_features"]

# exported symbols of include/agpl_predictive.h (libagpl_predictive.so: predictive moments and held-out log density)
PR_SYMBOLS = ["agpl_predictive"]

# exported symbols of include/agpl_chain.h (libagpl_chain.so: a chain of inducing draws projected at new inputs)
CH_SYMBOLS = ["agpl_plan_predict_chain"]

# exported symbols of include/agpl_kernels.h (libagpl_kernels.so: plans from raw inputs for Matern / rational-quadratic kernels)
KN_SYMBOLS = ["agpl_plan_create_stationary"]
# exported symbols of include/agpl_joint.h (libagpl_joint.so: the posterior covariance between new inputs)
JT_SYMBOLS = ["agpl_plan_predict_cov"]
# exported symbols of include/agpl_inducing.h (libagpl_inducing.so: k-means inducing inputs, shard-exact)
IN_SYMBOLS = ["agpl_kmeans_quanta", "agpl_kmeans_seed", "agpl_kmeans_bound", "agpl_kmeans_step", "agpl_kmeans_centres",
              "agpl_select_inducing_kmeans"]
# exported symbols of include/agpl_hyper.h (libagpl_hyper.so: the bound's gradient for log lengthscales and log variance)
HY_SYMBOLS = ["agpl_plan_hyper_grad"]
# exported symbols of include/agpl_zgrad.h (libagpl_zgrad.so: the bound's gradient for the inducing inputs, with the hyperparameters')
ZG_SYMBOLS = ["agpl_plan_inducing_grad"]
# exported symbols of include/agpl_pathwise.h (libagpl_pathwise.so: pathwise draws of the posterior function at new inputs)
PW_SYMBOLS = ["agpl_plan_sample_paths"]
# exported symbols of include/agpl_sample_y.h (libagpl_sampley.so: draws of y from a block of function draws)
SY_SYMBOLS = ["agpl_sample_y"]
# exported symbols of include/agpl_likgrad.h (libagpl_likgrad.so: E_q log p(y | f) and its gradient for the likelihood's parameters)
LG_SYMBOLS = ["agpl_expected_loglik"]
# exported symbols of include/agpl_grad.h (libagpl_grad.so: the posterior of d f / d x at new inputs)
GR_SYMBOLS = ["agpl_plan_predict_grad"]
# exported symbols of include/agpl_quantile.h (libagpl_quantile.so: P(Y <= y), P(Y > y) and the quantiles of the predictive of y)
QT_SYMBOLS = ["agpl_predictive_cdf", "agpl_predictive_quantile"]
# exported symbols of include/agpl_greedy.h (libagpl_greedy.so: greedy conditional-variance inducing inputs, shard-exact)
GV_SYMBOLS = ["agpl_greedy_bytes", "agpl_greedy_begin", "agpl_greedy_pivot", "agpl_greedy_step", "agpl_select_inducing_greedy"]
# exported symbols of include/agpl_loo.h (libagpl_loo.so: the leave-one-out cavity of a plan's q(v) at the training points)
LO_SYMBOLS = ["agpl_plan_loo_bytes", "agpl_plan_loo"]
# agpl_kernel_kind of include/agpl_kernels.h
KERNEL_SE, KERNEL_MATERN12, KERNEL_MATERN32, KERNEL_MATERN52, KERNEL_RQ = 0, 1, 2, 3, 4


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


def build(force: bool = False) -> str:
    """Compile libagpl.so for gfx950 in-tree (hipcc cross-compiles without a GPU)."""
    srcs = [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith((".hip", ".h"))]
    srcs += [os.path.join(os.path.dirname(_HERE), "include", h) for h in ("agpl.h", "agpl_se.h", "agpl_predictive.h", "agpl_chain.h", "agpl_kernels.h", "agpl_joint.h", "agpl_inducing.h", "agpl_hyper.h", "agpl_zgrad.h", "agpl_pathwise.h", "agpl_sample_y.h", "agpl_likgrad.h", "agpl_grad.h", "agpl_quantile.h", "agpl_greedy.h", "agpl_loo.h")]
    stale = not all(os.path.exists(p) for p in (LIB_PATH, SE_LIB_PATH, PR_LIB_PATH, CH_LIB_PATH, KN_LIB_PATH, JT_LIB_PATH, IN_LIB_PATH, HY_LIB_PATH, ZG_LIB_PATH, PW_LIB_PATH, SY_LIB_PATH, LG_LIB_PATH, GR_LIB_PATH, QT_LIB_PATH, GV_LIB_PATH, LO_LIB_PATH)) or any(os.path.getmtime(s) > os.path.getmtime(LIB_PATH) for s in srcs)
    if force or stale:
        subprocess.check_call(["make", "-C", CSRC, "-s", "-j4"])
    return LIB_PATH


_lib = None


def lib() -> C.CDLL:
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError(
                f"{LIB_PATH} is missing: the HIP extension has not been built "
                "(run `python -c 'import __graft_entry__ as g; g.build()'`). There is no CPU fallback.")
        # torch bundles its own libamdhip64 / librocblas: load torch first so that libagpl.so's NEEDED
        # entries resolve (by SONAME) to the runtime already in the process.  Two HIP runtimes in one
        # process do not share a device context (hipGetDeviceCount fails in the second one).
        import torch  # noqa: F401

        _lib = C.CDLL(LIB_PATH)
        _lib.agpl_last_error.restype = C.c_char_p
        _lib.agpl_last_error.argtypes = [C.c_void_p]
        _lib.agpl_plan_bytes.restype = C.c_int64
        for s in SYMBOLS:
            getattr(_lib, s)  # raises AttributeError if the library does not export the ABI
    return _lib


_se_lib = None


def se_lib() -> C.CDLL:
    """libagpl_se.so, loaded after (and resolving against) libagpl.so."""
    global _se_lib
    if _se_lib is None:
        lib()
        if not os.path.exists(SE_LIB_PATH):
            raise ImportError(f"{SE_LIB_PATH} is missing: the HIP extension has not been built. There is no CPU fallback.")
        _se_lib = C.CDLL(SE_LIB_PATH)
        _se_lib.agpl_plan_se_bytes.restype = C.c_int64
        for s in SE_SYMBOLS:
            getattr(_se_lib, s)
    return _se_lib


_pr_lib = None


def pr_lib() -> C.CDLL:
    """libagpl_predictive.so, loaded after (and resolving against) libagpl.so."""
    global _pr_lib
    if _pr_lib is None:
        lib()
        if not os.path.exists(PR_LIB_PATH):
            raise ImportError(f"{PR_LIB_PATH} is missing: the HIP extension has not been built. There is no CPU fallback.")
        _pr_lib = C.CDLL(PR_LIB_PATH)
        for s in PR_SYMBOLS:
            getattr(_pr_lib, s)
    return _pr_lib


_ch_lib = None


def chain_lib() -> C.CDLL:
    """libagpl_chain.so, loaded after (and resolving against) libagpl.so."""
    global _ch_lib
    if _ch_lib is None:
        lib()
        if not os.path.exists(CH_LIB_PATH):
            raise ImportError(f"{CH_LIB_PATH} is missing: the HIP extension has not been built. There is no CPU fallback.")
        _ch_lib = C.CDLL(CH_LIB_PATH)
        for s in CH_SYMBOLS:
            getattr(_ch_lib, s)
    return _ch_lib


_kn_lib = None


def kernels_lib() -> C.CDLL:
    """libagpl_kernels.so, loaded after (and resolving against) libagpl.so."""
    global _kn_lib
    if _kn_lib is None:
        lib()
        if not os.path.exists(KN_LIB_PATH):
            raise ImportError(f"{KN_LIB_PATH} is missing: the HIP extension has not been built. There is no CPU fallback.")
        _kn_lib = C.CDLL(KN_LIB_PATH)
        for s in KN_SYMBOLS:
            getattr(_kn_lib, s)
    return _kn_lib


_jt_lib = None


def joint_lib() -> C.CDLL:
    """libagpl_joint.so, loaded after (and resolving against) libagpl.so."""
    global _jt_lib
    if _jt_lib is None:
        lib()
        if not os.path.exists(JT_LIB_PATH):
            raise ImportError(f"{JT_LIB_PATH} is missing: the HIP extension has not been built. There is no CPU fallback.")
        _jt_lib = C.CDLL(JT_LIB_PATH)
        for s in JT_SYMBOLS:
            getattr(_jt_lib, s)
        _jt_lib.agpl_plan_predict_cov.restype = C.c_int32
        _jt_lib.agpl_plan_predict_cov.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64]
    return _jt_lib


_in_lib = None


def inducing_lib() -> C.CDLL:
    """libagpl_inducing.so, loaded after (and resolving against) libagpl.so."""
    global _in_lib
    if _in_lib is None:
        lib()
        if not os.path.exists(IN_LIB_PATH):
            raise ImportError(f"{IN_LIB_PATH} is missing: the HIP extension has not been built. There is no CPU fallback.")
        _in_lib = C.CDLL(IN_LIB_PATH)
        for s in IN_SYMBOLS:
            getattr(_in_lib, s).restype = C.c_int32
        P, I64, I32, F64 = C.c_void_p, C.c_int64, C.c_int32, C.c_double
        _in_lib.agpl_kmeans_quanta.argtypes = [P, F64, I64, I32, P, P]
        _in_lib.agpl_kmeans_seed.argtypes = [P, I64, I64, I64, I32, I32, P, P, P]
        _in_lib.agpl_kmeans_bound.argtypes = [P, I64, I32, P, P, P]
        _in_lib.agpl_kmeans_step.argtypes = [P, I64, I64, I32, I32, P, P, P, F64, P, P]
        _in_lib.agpl_kmeans_centres.argtypes = [P, I64, I32, I32, P, F64, P, P, P]
        _in_lib.agpl_select_inducing_kmeans.argtypes = [P, I64, I32, I32, P, P, I32, P, P, P]
    return _in_lib


_hy_lib = None


def hyper_lib() -> C.CDLL:
    """libagpl_hyper.so, loaded after (and resolving against) libagpl.so."""
    global _hy_lib
    if _hy_lib is None:
        lib()
        if not os.path.exists(HY_LIB_PATH):
            raise ImportError(f"{HY_LIB_PATH} is missing: the HIP extension has not been built. There is no CPU fallback.")
        _hy_lib = C.CDLL(HY_LIB_PATH)
        for s in HY_SYMBOLS:
            getattr(_hy_lib, s).restype = C.c_int32
        _hy_lib.agpl_plan_hyper_grad.argtypes = [C.c_void_p, C.c_int64] + [C.c_void_p] * 7
    return _hy_lib


_zg_lib = None


def zgrad_lib() -> C.CDLL:
    """libagpl_zgrad.so, loaded after (and resolving against) libagpl.so."""
    global _zg_lib
    if _zg_lib is None:
        lib()
        if not os.path.exists(ZG_LIB_PATH):
            raise ImportError(f"{ZG_LIB_PATH} is missing: the HIP extension has not been built. There is no CPU fallback.")
        _zg_lib = C.CDLL(ZG_LIB_PATH)
        for s in ZG_SYMBOLS:
            getattr(_zg_lib, s).restype = C.c_int32
        _zg_lib.agpl_plan_inducing_grad.argtypes = [C.c_void_p, C.c_int64] + [C.c_void_p] * 8
    return _zg_lib


_pw_lib = None


def pathwise_lib() -> C.CDLL:
    """libagpl_pathwise.so, loaded after (and resolving against) libagpl.so."""
    global _pw_lib
    if _pw_lib is None:
        lib()
        if not os.path.exists(PW_LIB_PATH):
            raise ImportError(f"{PW_LIB_PATH} is missing: the HIP extension has not been built. There is no CPU fallback.")
        _pw_lib = C.CDLL(PW_LIB_PATH)
        for s in PW_SYMBOLS:
            getattr(_pw_lib, s).restype = C.c_int32
        P = C.c_void_p
        _pw_lib.agpl_plan_sample_paths.argtypes = [P, C.c_int32, P, C.c_int32, P, P, P, P, C.c_int64, P, P, P]
    return _pw_lib


_sy_lib = None


def sample_y_lib() -> C.CDLL:
    """libagpl_sampley.so, loaded after (and resolving against) libagpl.so."""
    global _sy_lib
    if _sy_lib is None:
        lib()
        if not os.path.exists(SY_LIB_PATH):
            raise ImportError(f"{SY_LIB_PATH} is missing: the HIP extension has not been built. There is no CPU fallback.")
        _sy_lib = C.CDLL(SY_LIB_PATH)
        for s in SY_SYMBOLS:
            getattr(_sy_lib, s).restype = C.c_int32
        P = C.c_void_p
        _sy_lib.agpl_sample_y.argtypes = [P, P, C.c_int32, C.c_int64, C.c_int64, P, C.c_int64, C.c_int32, C.c_uint32, P]
    return _sy_lib


_lg_lib = None


def likgrad_lib() -> C.CDLL:
    """libagpl_likgrad.so, loaded after (and resolving against) libagpl.so."""
    global _lg_lib
    if _lg_lib is None:
        lib()
        if not os.path.exists(LG_LIB_PATH):
            raise ImportError(f"{LG_LIB_PATH} is missing: the HIP extension has not been built. There is no CPU fallback.")
        _lg_lib = C.CDLL(LG_LIB_PATH)
        for s in LG_SYMBOLS:
            getattr(_lg_lib, s).restype = C.c_int32
        P = C.c_void_p
        _lg_lib.agpl_expected_loglik.argtypes = [P, P, C.c_int64, P, P, P, P, P, P, P]
    return _lg_lib


_gr_lib = None


def grad_lib() -> C.CDLL:
    """libagpl_grad.so, loaded after (and resolving against) libagpl.so."""
    global _gr_lib
    if _gr_lib is None:
        lib()
        if not os.path.exists(GR_LIB_PATH):
            raise ImportError(f"{GR_LIB_PATH} is missing: the HIP extension has not been built. There is no CPU fallback.")
        _gr_lib = C.CDLL(GR_LIB_PATH)
        for s in GR_SYMBOLS:
            getattr(_gr_lib, s).restype = C.c_int32
        P = C.c_void_p
        _gr_lib.agpl_plan_predict_grad.argtypes = [P, C.c_int64, P, P, P]
    return _gr_lib


_qt_lib = None


def quantile_lib() -> C.CDLL:
    """libagpl_quantile.so, loaded after (and resolving against) libagpl.so."""
    global _qt_lib
    if _qt_lib is None:
        lib()
        if not os.path.exists(QT_LIB_PATH):
            raise ImportError(f"{QT_LIB_PATH} is missing: the HIP extension has not been built. There is no CPU fallback.")
        _qt_lib = C.CDLL(QT_LIB_PATH)
        for s in QT_SYMBOLS:
            getattr(_qt_lib, s).restype = C.c_int32
        P = C.c_void_p
        _qt_lib.agpl_predictive_cdf.argtypes = [P, P, C.c_int64, P, P, P, P, P]
        _qt_lib.agpl_predictive_quantile.argtypes = [P, P, C.c_int64, P, P, C.c_int32, P, P]
    return _qt_lib


_gv_lib = None


def greedy_lib() -> C.CDLL:
    """libagpl_greedy.so, loaded after (and resolving against) libagpl.so."""
    global _gv_lib
    if _gv_lib is None:
        lib()
        if not os.path.exists(GV_LIB_PATH):
            raise ImportError(f"{GV_LIB_PATH} is missing: the HIP extension has not been built. There is no CPU fallback.")
        _gv_lib = C.CDLL(GV_LIB_PATH)
        for s in GV_SYMBOLS:
            getattr(_gv_lib, s).restype = C.c_int32
        P, I64, I32, F64 = C.c_void_p, C.c_int64, C.c_int32, C.c_double
        _gv_lib.agpl_greedy_bytes.argtypes = [I64, I32, P]
        _gv_lib.agpl_greedy_begin.argtypes = [P, I64, I64, I64, I32, I32, P, F64, P, I64, P]
        _gv_lib.agpl_greedy_pivot.argtypes = [P, I64, I64, I64, I32, I32, I32, P, P, I64, P, P]
        _gv_lib.agpl_greedy_step.argtypes = [P, I64, I64, I64, I32, I32, I32, F64, I32, P, P, F64, P, P, P, I64, P, P]
        _gv_lib.agpl_select_inducing_greedy.argtypes = [P, I64, I32, I32, I32, F64, P, P, F64, F64, P, I64, P, P, P]
    return _gv_lib


_lo_lib = None


def loo_lib() -> C.CDLL:
    """libagpl_loo.so, loaded after (and resolving against) libagpl.so."""
    global _lo_lib
    if _lo_lib is None:
        lib()
        if not os.path.exists(LO_LIB_PATH):
            raise ImportError(f"{LO_LIB_PATH} is missing: the HIP extension has not been built. There is no CPU fallback.")
        _lo_lib = C.CDLL(LO_LIB_PATH)
        for s in LO_SYMBOLS:
            getattr(_lo_lib, s)
        P, I64, I32 = C.c_void_p, C.c_int64, C.c_int32
        _lo_lib.agpl_plan_loo_bytes.restype = I64
        _lo_lib.agpl_plan_loo_bytes.argtypes = [I64, I32]
        _lo_lib.agpl_plan_loo.restype = I32
        _lo_lib.agpl_plan_loo.argtypes = [P, P, P, P, P, I64, P, P, P, P, P]
    return _lo_lib


def check(ctx_handle, rc):
    if rc != AGPL_OK:
        msg = lib().agpl_last_error(ctx_handle)
        msg = msg.decode() if msg else ""
        raise _ERR_TYPES.get(rc, AGPLError)(rc, msg)
