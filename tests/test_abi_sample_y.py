"""The surface of libagpl_sampley.so (include/agpl_sample_y.h), CPU-only: the header's one prototype, the library's exports and the
binding's list agree; the binding's argument types follow the header; the library holds a gfx950 code object with the sampling
kernel; the Makefile builds and links it as the other extensions, its object without fused multiply-add; libagpl.so keeps its 45
exports, the predictive and pathwise libraries their one each; the Python surface exists; the header compiles alone."""
import ctypes as C
import os
import re
import subprocess

import abi_support as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "augmentedgplikelihoods.jl_amd", "csrc")
INC = os.path.join(ROOT, "include")
HEADER = os.path.join(INC, "agpl_sample_y.h")


def test_header_exports_and_binding_agree():
    import agpl_amd  # noqa: F401
    from agpl_amd import _ffi

    protos = S.arguments(HEADER)
    assert sorted(protos) == ["agpl_sample_y"]
    assert len(protos["agpl_sample_y"]) == 10
    out = subprocess.check_output(["nm", "-D", "--defined-only", _ffi.SY_LIB_PATH]).decode()
    assert sorted(set(re.findall(r" T (agpl_\w+)", out))) == sorted(protos) == sorted(_ffi.SY_SYMBOLS)
    lib = _ffi.sample_y_lib()  # loads, resolving against libagpl.so
    for name, args in protos.items():
        fn = getattr(lib, name)
        assert list(fn.argtypes) == [S.ctype(a) for a in args], name
        assert fn.restype is C.c_int32


def test_library_holds_a_gfx950_code_object():
    from agpl_amd import _ffi

    blob = open(_ffi.SY_LIB_PATH, "rb").read()
    assert b"amdgcn-amd-amdhsa--gfx950" in blob
    # one instantiation per likelihood kind: sample_y_kernel<0> .. sample_y_kernel<7>
    for kind in range(8):
        assert b"15sample_y_kernelILi%dEE" % kind in blob, kind


def test_the_other_libraries_keep_their_exports():
    from agpl_amd import _ffi

    out = subprocess.check_output(["nm", "-D", "--defined-only", _ffi.LIB_PATH]).decode()
    assert len(set(re.findall(r" T (agpl_\w+)", out))) == 45 == len(_ffi.SYMBOLS)
    assert "sample_y" not in out
    assert len(S.arguments(os.path.join(INC, "agpl.h"))) == 45
    for path, syms in ((_ffi.PR_LIB_PATH, _ffi.PR_SYMBOLS), (_ffi.PW_LIB_PATH, _ffi.PW_SYMBOLS), (_ffi.CH_LIB_PATH, _ffi.CH_SYMBOLS)):
        out = subprocess.check_output(["nm", "-D", "--defined-only", path]).decode()
        assert sorted(set(re.findall(r" T (agpl_\w+)", out))) == sorted(syms)
    assert re.search(r"#define\s+AGPL_VERSION\s+121\b", open(os.path.join(INC, "agpl.h")).read())


def test_makefile_builds_and_links_the_library_as_the_other_extensions():
    assert S.links_exactly("../libagpl_sampley.so", "agpl_sample_y.o")  # by default, in none of the other libraries, cleaned
    assert S.linked_like("../libagpl_sampley.so", "../libagpl_predictive.so")
    assert "agpl_sample_y.o" in S.recompiled_by("agpl_random.h") & S.recompiled_by("../../include/agpl_sample_y.h")
    # compared draw for draw against a float64 host evaluation: no fused-multiply-add contraction
    assert S.contraction_off("agpl_sample_y.o")
    src = open(os.path.join(CSRC, "agpl_sample_y.hip")).read()
    # the generator and the scalar samplers are agpl_random.h's, not restated; the descriptor is read here (libagpl.so's helper is hidden)
    assert '#include "agpl_random.h"' in src and "agpl::rand_poisson(" in src and "agpl::rand_gamma(" in src
    assert "agpl_lik_to_device" not in src and "hipMalloc" not in src and "Synchronize" not in src
    assert "atomic" not in src and "__shared__" not in src


def test_python_surface_exists():
    import agpl_amd

    assert callable(agpl_amd.sample_y) and agpl_amd.sample_y is agpl_amd.operators.sample_y
    assert callable(agpl_amd.Paths.sample_y) and callable(agpl_amd.Plan.sample_y)
    assert callable(agpl_amd.SparseCAVI.sample_y) and callable(agpl_amd.SparseGibbs.sample_y)
    assert isinstance(agpl_amd.Paths._Y_CHUNK, int)
    assert "sample_y" in agpl_amd.__all__


def test_header_compiles_alone(tmp_path):
    S.header_compiles_alone("agpl_sample_y.h",
                            "return agpl_sample_y(0, 0, 0, 0, 0, 0, 0, 0, 0, 0) == AGPL_ERR_INVALID_ARGUMENT ? 0 : 1;", tmp_path)
