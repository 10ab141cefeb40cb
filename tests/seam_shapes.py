"""The shapes of tests/test_gpu_seams.py and the compile-time constants that decide where the "new inputs" entry points cut their
points: read from the sources, so that the shapes can be held against the code (tests/test_seam_shapes_cpu.py does that without a
GPU).  The shapes are plain numbers, NOT functions of the constants: a constant that moves makes the CPU test fail, instead of the
GPU tests quietly following it to a shape nobody looked at.  No GPU, no library code."""
import os
import re

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "augmentedgplikelihoods.jl_amd", "csrc")
# name -> the file that states it
WHERE = {"kPredictChunk": "agpl_features.hip", "kPathChunk": "agpl_pathwise.hip", "kPsiBudget": "agpl_pathwise.hip",
         "kHyperChunk": "agpl_hyper_impl.h", "kZPartBudget": "agpl_hyper_impl.h", "kMaxBlocks": "agpl_predictive.hip",
         "BS": "agpl_se_build.h", "KT": "agpl_se_build.h", "kBlock": "agpl_predictive.hip"}


def constant(name):
    """The value of ``constexpr <type> name = <integer expression>;`` in its file (casts dropped); LookupError if it is not there."""
    src = open(os.path.join(CSRC, WHERE[name])).read()
    m = re.search(r"^\s*constexpr\s+\w+\s+" + name + r"\s*=\s*([^;]+);", src, flags=re.M)
    if not m:
        raise LookupError(f"{name} is not stated in {WHERE[name]}")
    expr = re.sub(r"\(\s*(size_t|int64_t|int)\s*\)", "", m.group(1))
    if not re.fullmatch(r"[\d\s<>()+*/-]+", expr):
        raise LookupError(f"{name} = {m.group(1)!r} is not an integer expression")
    return int(eval(expr.replace("/", "//"), {"__builtins__": {}}))  # (digits, shifts and arithmetic only: the match above)


def cdiv(a, b):
    return -(-a // b)


# ---- what the launch code does with its constants, restated ----------------------------------------------------------------------------

def chunks(N, chunk):
    """[(c0, n)] of a loop ``for (c0 = 0; c0 < N; c0 += C)`` with C = min(N, chunk)."""
    C = min(N, chunk)
    return [(c0, min(C, N - c0)) for c0 in range(0, N, C)]


def path_sub(F, Ns):
    """Points of a sub-chunk of agpl_plan_sample_paths: the Psi image (two float16 planes of Fp = F rounded up to KT columns) within
    kPsiBudget, a multiple of BS, at least one tile and at most the chunk."""
    BS, KT = constant("BS"), constant("KT")
    Fp = cdiv(F, KT) * KT
    sub = constant("kPsiBudget") // (4 * Fp) // BS * BS
    return min(max(sub, BS), cdiv(min(Ns, constant("kPathChunk")), BS) * BS)


def path_launches(F, Ns):
    """[(c0, q0, nq)]: the (chunk, sub-chunk) steps of agpl_plan_sample_paths."""
    sub = path_sub(F, Ns)
    return [(c0, q0, min(sub, n - q0)) for c0, n in chunks(Ns, constant("kPathChunk")) for q0 in range(0, n, sub)]


def zgrad_groups(N, M, D):
    """Per chunk of agpl_plan_inducing_grad, the tile counts of its launches of the points kernel: groups of
    gtiles = kZPartBudget / (8 M D) tiles (at least 1, at most the chunk's tiles).  M: the live count Mc."""
    BS = constant("BS")
    C = min(N, constant("kHyperChunk"))
    gtiles = min(max(constant("kZPartBudget") // (8 * M * D), 1), cdiv(C, BS))
    return [[min(gtiles, cdiv(n, BS) - t0) for t0 in range(0, cdiv(n, BS), gtiles)] for _, n in chunks(N, constant("kHyperChunk"))]


# ---- the shapes --------------------------------------------------------------------------------------------------------------------------

CHUNK = 65536  # what the three chunk constants are today (the CPU test holds them to it: the index lists below straddle it)

# 1. agpl_plan_predict
PREDICT_M, PREDICT_D, PREDICT_LS = 64, 2, (1, 3)
PREDICT_NS = 65536 + 129
PREDICT_WINDOW = 65536 - 200  # [this, Ns): not tile-aligned, the seam inside
PREDICT_HEAD = 129
PREDICT_GATHER = [65664, 0, 65536, 127, 5, 128, 65535, 4097, 65537, 300]

# 2. agpl_plan_sample_paths: (F, Ns, gather)
PATHS_SMALL = (100, 65536 + 129, [65664, 0, 65536, 127, 5, 65535, 4097, 65537, 300])
PATHS_LARGE = (8192, 65536 + 8192 + 129, [65536 + 8192 + 128, 0, 65536, 65536 + 8191, 5, 65535, 65536 + 8193, 8192, 65537, 65536 + 8192, 8191])
PATHS_WINDOW = 65536 - 200
PATHS_ZERO_NS = 129

# 3. agpl_plan_inducing_grad: (N, M, D); the first shard of the shard identity is exactly the first group of chunk one
ZGRAD_N, ZGRAD_M, ZGRAD_D = 65536 + 300, 300, 16
ZGRAD_GROUPS = [[436, 76], [3]]
ZGRAD_CUT = 436 * 128

# 4. agpl_plan_hyper_grad, L = 2, a prior mean, two chunks
HYPER_N, HYPER_CUT = 65536 + 300, 65536

# 5. agpl_predictive
PRED_SCALAR_N = 262144 + 257
PRED_SCALAR_SLICES = [(0, 300), (262000, 262401), (262144, 262401)]
PRED_CAT_N = 4096 + 5
PRED_CAT_SLICES = [(0, 9), (2047, 2060), (4090, 4101)]
