"""CPU checks of the stationary-kernel plan surface (include/agpl_kernels.h, libagpl_kernels.so: agpl_plan_create_stationary): the
header, the library's export list, the binding and the Julia shim agree, the header shares nothing with the other four and stands
alone, the Makefile builds and links the library as it does the other extensions, every instantiation of the feature generator keeps
the squared exponential's register budget, the ``kernel`` argument is refused before any device work, and the float64 numpy
reference of tests/test_gpu_kernels.py reproduces closed-form values and stays inside that file's conditions at its shapes."""
import os
import re
import subprocess

import numpy as np
import pytest

import abi_support as S
import kernels_reference as K
from test_julia_artifacts import header_prototypes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "augmentedgplikelihoods.jl_amd", "csrc")
INC = os.path.join(ROOT, "include")
KN_HEADER = os.path.join(INC, "agpl_kernels.h")
EXT = os.path.join(ROOT, "julia", "AGPLDeviceExt.jl")
HIPCC = "/opt/rocm/bin/hipcc"
NAME = "agpl_plan_create_stationary"


def test_header_declares_exactly_the_exported_symbol():
    import agpl_amd  # noqa: F401
    from agpl_amd import _ffi

    protos = S.arities(KN_HEADER)
    assert protos == {NAME: 15}
    assert S.exports(_ffi.KN_LIB_PATH) == [NAME]
    assert _ffi.KN_SYMBOLS == [NAME]
    _ffi.kernels_lib()  # loads, resolving against libagpl.so
    # the kinds of the header's enum are the binding's and the reference's
    enum = dict(re.findall(r"\b(AGPL_KERNEL_\w+)\s*=\s*(\d+)", re.sub(r"/\*.*?\*/", "", open(KN_HEADER).read(), flags=re.S)))
    assert {k: int(v) for k, v in enum.items()} == {"AGPL_KERNEL_SE": 0, "AGPL_KERNEL_MATERN12": 1, "AGPL_KERNEL_MATERN32": 2,
                                                    "AGPL_KERNEL_MATERN52": 3, "AGPL_KERNEL_RQ": 4}
    assert (_ffi.KERNEL_SE, _ffi.KERNEL_MATERN12, _ffi.KERNEL_MATERN32, _ffi.KERNEL_MATERN52, _ffi.KERNEL_RQ) == K.KINDS


def test_header_shares_no_symbol_with_the_other_four():
    protos = set(S.arities(KN_HEADER))
    assert len(header_prototypes()) == 45 and not protos & set(header_prototypes())
    for other, count in (("agpl_se.h", 4), ("agpl_predictive.h", 1), ("agpl_chain.h", 1)):
        theirs = S.arities(os.path.join(INC, other))
        assert len(theirs) == count and not protos & set(theirs), other
    includes = re.findall(r'#include\s+[<"]([^>"]+)[>"]', open(KN_HEADER).read())
    assert includes == ["agpl.h"]


def test_header_compiles_alone(tmp_path):
    S.header_compiles_alone("agpl_kernels.h",
                            "return agpl_plan_create_stationary(0, 0, 0, 0, 0, AGPL_KERNEL_RQ, 2.0, 0, 0, 0, 1.0, 0.0, 0, 0, 0)"
                            " == AGPL_ERR_INVALID_ARGUMENT ? 0 : 1;", tmp_path)


def test_julia_ccall_has_the_prototypes_arity():
    src = open(EXT).read()
    m = re.search(r"ccall\(\(:" + NAME + r",\s*libagpl_kernels\),\s*\w+,\s*\(([^)]*)\)", src)
    assert m and len([t for t in m.group(1).split(",") if t.strip()]) == S.arities(KN_HEADER)[NAME] == 15
    assert re.search(r'^const libagpl_kernels\s*=.*"libagpl_kernels\.so"', src, flags=re.M)
    # one method maps the KernelFunctions.jl kernels to (kind, param)
    kinds = dict(re.findall(r"^kernel_kind\(\w*::(\w+)\) = \(Int32\((\d)\)", src, flags=re.M))
    assert kinds == {"SqExponentialKernel": "0", "ExponentialKernel": "1", "Matern32Kernel": "2", "Matern52Kernel": "3",
                     "RationalQuadraticKernel": "4"}
    assert re.search(r"^kernel_kind\(k::RationalQuadraticKernel\).*k\.α", src, flags=re.M)


def test_makefile_builds_and_links_the_library_as_the_other_extensions():
    assert S.links_exactly("../libagpl_kernels.so", "agpl_kernels.o")  # by default, in none of the other libraries, cleaned
    assert S.linked_like("../libagpl_kernels.so", "../libagpl_se.so", "../libagpl_predictive.so", "../libagpl_chain.so")
    # the new headers are prerequisites of the objects that include them, as the ones that were there and the Makefile
    for h in ("../../include/agpl_chain.h", "agpl_kernel_rules.h", "agpl_se_create.h", "../../include/agpl_kernels.h", "Makefile"):
        assert {"agpl_kernels.o", "agpl_features.o"} <= S.recompiled_by(h), h
    # the rules are stated once and the entry points' body exists once
    assert '#include "agpl_kernel_rules.h"' in open(os.path.join(CSRC, "agpl_se_build.h")).read()
    for f in ("agpl_features.hip", "agpl_kernels.hip"):
        src = open(os.path.join(CSRC, f)).read()
        assert '#include "agpl_se_create.h"' in src and "hipMalloc((void **)&tmp" not in src, f
    assert open(os.path.join(CSRC, "agpl_se_create.h")).read().count("static int32_t agpl_se_create(") == 1


@pytest.mark.parametrize("source", ["agpl_features.hip", "agpl_chain.hip", "agpl_kernels.hip"])
def test_every_generator_instantiation_keeps_two_workgroups_per_cu(tmp_path, source):
    """The code-object metadata of every se_build_kernel<kind> in every library that carries it: no private segment, no spilled
    VGPR, at most 256 VGPRs (two 256-thread workgroups per CU, as __launch_bounds__(256, 2) states), and the whitening on the
    matrix cores."""
    if not os.path.exists(HIPCC):
        pytest.skip("no hipcc")
    flags = re.search(r"^COMMON\s*:=\s*(.*)$", open(os.path.join(CSRC, "Makefile")).read(), flags=re.M).group(1)
    flags = flags.replace("$(ARCH)", "gfx950").split()
    subprocess.check_call([HIPCC] + flags + ["--cuda-device-only", "-S", os.path.join(CSRC, source), "-o", "k.s"],
                          cwd=tmp_path, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    asm = open(os.path.join(tmp_path, "k.s")).read()
    lines = asm.splitlines()
    blocks = re.findall(r"\.name:\s+(_Z\w*se_build_kernelILi\d+E\w*)(.*?)(?=\n  - |\Z)", asm, flags=re.S)
    assert len(blocks) >= 5, [b[0] for b in blocks]
    assert sorted(int(re.search(r"se_build_kernelILi(\d+)E", name).group(1)) for name, _ in blocks) == list(K.KINDS)
    for name, meta in blocks:
        assert re.search(r"\.private_segment_fixed_size:\s+0\b", meta), name
        assert re.search(r"\.vgpr_spill_count:\s+0\b", meta), name
        vgprs = int(re.search(r"\.vgpr_count:\s+(\d+)", meta).group(1))
        print(source, name[:48], "vgpr_count", vgprs)
        assert 0 < vgprs <= 256, (name, vgprs)
        start = next(i for i, ln in enumerate(lines) if ln.startswith(name + ":"))
        end = next(i for i in range(start, len(lines)) if "s_endpgm" in lines[i])
        assert any("v_mfma_f32_32x32x2" in ln.split(";")[0] for ln in lines[start:end + 1]), name


def test_kernel_argument_is_checked_before_any_device_work():
    import agpl_amd as A

    lik = A.BernoulliLikelihood()
    for bad in ("cubic", ("rq", 0.0), ("rq", -1.0), ("rq", float("nan")), ("rq",), ("matern32", 1.0), None, 2):
        with pytest.raises(A.ArgumentError):
            A.Plan.from_inputs(None, None, 1.0, kernel=bad)
        with pytest.raises(A.ArgumentError):
            A.SparseCAVI.from_inputs(lik, None, None, None, 1.0, kernel=bad)
        with pytest.raises(A.ArgumentError):
            A.SparseGibbs.from_inputs(lik, None, None, None, 1.0, kernel=bad)
    from agpl_amd.sparse import kernel_kind

    assert kernel_kind("se") == (0, 0.0) and kernel_kind("matern12") == kernel_kind("exponential") == (1, 0.0)
    assert kernel_kind("matern32") == (2, 0.0) and kernel_kind("matern52") == (3, 0.0) and kernel_kind(("rq", 2)) == (4, 2.0)


def test_reference_reproduces_closed_forms():
    one, ell = np.zeros((1, 1)), np.ones(1)
    at = lambda kind, r, s2=1.0, param=0.0: K.kernel(kind, one, one + r, ell, s2, param)[0, 0]
    assert abs(at(K.MATERN32, 1.0) - 2.7320508 * np.exp(-np.sqrt(3.0))) < 1e-8
    assert abs(at(K.RQ, np.sqrt(2.0), param=1.0) - 0.5) < 1e-15
    assert abs(at(K.SE, 2.0) - np.exp(-2.0)) < 1e-16 and abs(at(K.MATERN12, 2.0) - np.exp(-2.0)) < 1e-16
    assert abs(at(K.MATERN52, 1.0) - (1 + np.sqrt(5.0) + 5.0 / 3.0) * np.exp(-np.sqrt(5.0))) < 1e-15
    for kind in K.KINDS:
        for s2 in (1.0, 2.5):
            assert at(kind, 0.0, s2, K.param_of(kind)) == s2
    # ARD: each coordinate is divided by its own lengthscale
    a, b, l3 = np.array([[0.3, -1.0, 2.0]]), np.array([[1.3, 0.4, 0.2]]), np.array([1.0, 1.4, 1.8])
    r2 = 1.0 + 1.0 + 1.0
    assert abs(K.kernel(K.RQ, a, b, l3, 2.5, 2.0)[0, 0] - 2.5 * (1 + r2 / 4.0) ** -2.0) < 1e-15
    # the rational quadratic tends to the squared exponential as alpha grows: the difference is k r^4 / (8 alpha) to first order
    assert abs(at(K.RQ, 1.3, param=1e4) - at(K.SE, 1.3)) < 2 * at(K.SE, 1.3) * 1.3 ** 4 / 8e4


@pytest.mark.parametrize("kind", K.KINDS, ids=[K.NAMES[k] for k in K.KINDS])
def test_reference_stays_inside_the_gpu_tests_conditions(kind):
    """At the shapes of tests/test_gpu_kernels.py the float64 reference alone has a moderately conditioned K_ZZ + jitter I, a
    residual that is >= 1e-8 s2 (so >= 0 with room for float32 round-off of the clamp) and max |phi| <= sigma (the scale rule).
    The largest condition number is the squared exponential's at M = 300, D = 1: 33099.6, i.e. 3.3e4 to the two figures it is
    quoted with (asserted as < 3.35e4)."""
    for M, D, s2 in K.SHAPES:
        x, z, ell = K.workload(K.N, M, D)
        param = K.param_of(kind)
        cond = np.linalg.cond(K.kernel(kind, z, z, ell, s2, param) + K.JITTER * np.eye(M))
        Phi, _, _ = K.phi_f64(kind, x, z, ell, s2, K.JITTER, param)
        raw = s2 - (Phi * Phi).sum(1)
        print(K.NAMES[kind], M, D, s2, f"cond {cond:.6g} min residual / s2 {raw.min() / s2:.4g} max |phi| / sigma "
              f"{np.abs(Phi).max() / np.sqrt(s2):.4f}")
        assert cond < 3.35e4, (M, D, s2, cond)
        assert raw.min() >= 1e-8 * s2, (M, D, s2, raw.min())
        assert np.abs(Phi).max() <= np.sqrt(s2), (M, D, s2)
