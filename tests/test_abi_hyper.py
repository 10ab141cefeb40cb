"""The surface of libagpl_hyper.so (include/agpl_hyper.h), CPU-only: the header's prototypes, the library's exports and the binding's
list agree; the binding's argument types follow the header; the library holds a gfx950 code object with the gradient's kernels; the
Makefile builds and links it as the other extensions; libagpl.so keeps its 45 exports; the header compiles alone."""
import ctypes as C
import os
import re
import subprocess

import abi_support as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "augmentedgplikelihoods.jl_amd", "csrc")
INC = os.path.join(ROOT, "include")
HEADER = os.path.join(INC, "agpl_hyper.h")


def test_header_exports_and_binding_agree():
    import agpl_amd  # noqa: F401
    from agpl_amd import _ffi

    protos = S.arguments(HEADER)
    assert sorted(protos) == ["agpl_plan_hyper_grad"]
    out = subprocess.check_output(["nm", "-D", "--defined-only", _ffi.HY_LIB_PATH]).decode()
    assert sorted(set(re.findall(r" T (agpl_\w+)", out))) == sorted(protos) == sorted(_ffi.HY_SYMBOLS)
    lib = _ffi.hyper_lib()  # loads, resolving against libagpl.so
    for name, args in protos.items():
        fn = getattr(lib, name)
        assert list(fn.argtypes) == [S.ctype(a) for a in args], name
        assert fn.restype is C.c_int32


def test_library_holds_a_gfx950_code_object():
    from agpl_amd import _ffi

    blob = open(_ffi.HY_LIB_PATH, "rb").read()
    assert b"amdgcn-amd-amdhsa--gfx950" in blob
    assert b"hy_points_kernel" in blob and b"hy_kzz_grad_kernel" in blob


def test_libagpl_keeps_its_exports():
    from agpl_amd import _ffi

    out = subprocess.check_output(["nm", "-D", "--defined-only", _ffi.LIB_PATH]).decode()
    assert len(set(re.findall(r" T (agpl_\w+)", out))) == 45 == len(_ffi.SYMBOLS)
    assert "hyper" not in out
    assert re.search(r"#define\s+AGPL_VERSION\s+121\b", open(os.path.join(INC, "agpl.h")).read())


def test_makefile_builds_and_links_the_library_as_the_other_extensions():
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert S.links_exactly("../libagpl_hyper.so", "agpl_hyper.o")  # by default, in none of the other libraries, cleaned
    assert S.linked_like("../libagpl_hyper.so", "../libagpl_chain.so")
    assert "agpl_hyper.o" in S.recompiled_by("agpl_kernel_rules.h") & S.recompiled_by("../../include/agpl_hyper.h")
    assert re.search(r"^COMMON\s*:=\s*-O3 -std=c\+\+17 -fPIC --offload-arch=\$\(ARCH\) -fvisibility=hidden -Wall -Wno-unused-function "
                     r"-fno-slp-vectorize\s*$", mk, flags=re.M)


def test_header_compiles_alone(tmp_path):
    S.header_compiles_alone("agpl_hyper.h",
                            "return agpl_plan_hyper_grad(0, 0, 0, 0, 0, 0, 0, 0, 0) == AGPL_ERR_INVALID_ARGUMENT ? 0 : 1;", tmp_path)
