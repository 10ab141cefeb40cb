"""The surface of libagpl_likgrad.so (include/agpl_likgrad.h), CPU-only: the header's one prototype, the library's exports and the
binding's list agree; the binding's argument types follow the header; the library holds a gfx950 code object with one kernel per
non-categorical kind; the Makefile builds and links it as the other extensions, its object without fused multiply-add; libagpl.so
keeps its 45 exports, the predictive and sample-y libraries their one each; the Python surface exists; the header compiles alone."""
import ctypes as C
import os
import re
import subprocess

import abi_support as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "augmentedgplikelihoods.jl_amd", "csrc")
INC = os.path.join(ROOT, "include")
HEADER = os.path.join(INC, "agpl_likgrad.h")


def test_header_exports_and_binding_agree():
    import agpl_amd  # noqa: F401
    from agpl_amd import _ffi

    protos = S.arguments(HEADER)
    assert sorted(protos) == ["agpl_expected_loglik"]
    assert len(protos["agpl_expected_loglik"]) == 10
    out = subprocess.check_output(["nm", "-D", "--defined-only", _ffi.LG_LIB_PATH]).decode()
    assert sorted(set(re.findall(r" T (agpl_\w+)", out))) == sorted(protos) == sorted(_ffi.LG_SYMBOLS)
    lib = _ffi.likgrad_lib()  # loads, resolving against libagpl.so
    for name, args in protos.items():
        fn = getattr(lib, name)
        assert list(fn.argtypes) == [S.ctype(a) for a in args], name
        assert fn.restype is C.c_int32


def test_library_holds_a_gfx950_code_object():
    from agpl_amd import _ffi

    blob = open(_ffi.LG_LIB_PATH, "rb").read()
    assert b"amdgcn-amd-amdhsa--gfx950" in blob
    # one instantiation per non-categorical kind, none for the categorical ones (3, 4)
    for kind in range(8):
        assert (b"22expected_loglik_kernelILi%dEE" % kind in blob) == (kind not in (3, 4)), kind


def test_the_other_libraries_keep_their_exports():
    from agpl_amd import _ffi

    out = subprocess.check_output(["nm", "-D", "--defined-only", _ffi.LIB_PATH]).decode()
    assert len(set(re.findall(r" T (agpl_\w+)", out))) == 45 == len(_ffi.SYMBOLS)
    assert "expected_loglik" not in out
    assert len(S.arguments(os.path.join(INC, "agpl.h"))) == 45
    for path, syms in ((_ffi.PR_LIB_PATH, _ffi.PR_SYMBOLS), (_ffi.SY_LIB_PATH, _ffi.SY_SYMBOLS)):
        out = subprocess.check_output(["nm", "-D", "--defined-only", path]).decode()
        assert sorted(set(re.findall(r" T (agpl_\w+)", out))) == sorted(syms)
    assert re.search(r"#define\s+AGPL_VERSION\s+121\b", open(os.path.join(INC, "agpl.h")).read())


def test_makefile_builds_and_links_the_library_as_the_other_extensions():
    assert S.links_exactly("../libagpl_likgrad.so", "agpl_likgrad.o")  # by default, in none of the other libraries, cleaned
    assert S.linked_like("../libagpl_likgrad.so", "../libagpl_predictive.so")
    assert "agpl_likgrad.o" in S.recompiled_by("agpl_digamma.h") & S.recompiled_by("../../include/agpl_likgrad.h")
    # compared point by point against float64 host integration: no fused-multiply-add contraction
    assert S.contraction_off("agpl_likgrad.o")
    src = open(os.path.join(CSRC, "agpl_likgrad.hip")).read()
    # digamma is agpl_digamma.h's, stated once; the sums are fixed-order (no atomics); the call stays asynchronous
    assert '#include "agpl_digamma.h"' in src and "agpl::digamma(" in src
    assert "atomic" not in src and "Synchronize" not in src
    assert "digamma" not in re.sub(r"agpl::digamma|agpl_digamma", "", src)


def test_python_surface_exists():
    import agpl_amd

    assert callable(agpl_amd.expected_loglik) and agpl_amd.expected_loglik is agpl_amd.operators.expected_loglik
    assert callable(agpl_amd.SparseCAVI.expected_loglik) and callable(agpl_amd.SparseCAVI.bound)
    assert callable(agpl_amd.learn_likelihood) and agpl_amd.learn_likelihood is agpl_amd.sparse.learn_likelihood
    assert not hasattr(agpl_amd.SparseGibbs, "expected_loglik")
    assert "expected_loglik" in agpl_amd.__all__ and "learn_likelihood" in agpl_amd.__all__
    assert agpl_amd.StudentTLikelihood._param_names == ("nu", "sigma") and agpl_amd.BernoulliLikelihood._param_names == ()


def test_header_compiles_alone(tmp_path):
    S.header_compiles_alone("agpl_likgrad.h",
                            "return agpl_expected_loglik(0, 0, 0, 0, 0, 0, 0, 0, 0, 0) == AGPL_ERR_INVALID_ARGUMENT ? 0 : 1;", tmp_path)
