"""The surface of libagpl_zgrad.so (include/agpl_zgrad.h), CPU-only: the header's prototypes, the library's exports and the binding's
list agree; the binding's argument types follow the header; the library holds a gfx950 code object with the gradient's kernels; the
Makefile builds and links it as the other extensions, from the shared agpl_hyper_impl.h and without agpl_hyper.hip; libagpl.so keeps
its 45 exports and libagpl_hyper.so its one; the header compiles alone."""
import ctypes as C
import os
import re
import subprocess

import abi_support as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "augmentedgplikelihoods.jl_amd", "csrc")
INC = os.path.join(ROOT, "include")
HEADER = os.path.join(INC, "agpl_zgrad.h")


def test_header_exports_and_binding_agree():
    import agpl_amd  # noqa: F401
    from agpl_amd import _ffi

    protos = S.arguments(HEADER)
    assert sorted(protos) == ["agpl_plan_inducing_grad"]
    out = subprocess.check_output(["nm", "-D", "--defined-only", _ffi.ZG_LIB_PATH]).decode()
    assert sorted(set(re.findall(r" T (agpl_\w+)", out))) == sorted(protos) == sorted(_ffi.ZG_SYMBOLS)
    lib = _ffi.zgrad_lib()  # loads, resolving against libagpl.so
    for name, args in protos.items():
        fn = getattr(lib, name)
        assert list(fn.argtypes) == [S.ctype(a) for a in args], name
        assert fn.restype is C.c_int32


def test_library_holds_a_gfx950_code_object():
    from agpl_amd import _ffi

    blob = open(_ffi.ZG_LIB_PATH, "rb").read()
    assert b"amdgcn-amd-amdhsa--gfx950" in blob
    assert b"hy_points_kernel" in blob and b"hy_kzz_grad_kernel" in blob
    assert b"hy_kzz_zgrad_kernel" in blob and b"hy_zreduce_kernel" in blob and b"hy_zfinal_kernel" in blob


def test_libagpl_and_libagpl_hyper_keep_their_exports():
    from agpl_amd import _ffi

    out = subprocess.check_output(["nm", "-D", "--defined-only", _ffi.LIB_PATH]).decode()
    assert len(set(re.findall(r" T (agpl_\w+)", out))) == 45 == len(_ffi.SYMBOLS)
    assert "inducing_grad" not in out
    out = subprocess.check_output(["nm", "-D", "--defined-only", _ffi.HY_LIB_PATH]).decode()
    assert sorted(set(re.findall(r" T (agpl_\w+)", out))) == ["agpl_plan_hyper_grad"] == _ffi.HY_SYMBOLS
    assert re.search(r"#define\s+AGPL_VERSION\s+121\b", open(os.path.join(INC, "agpl.h")).read())


def test_makefile_builds_and_links_the_library_as_the_other_extensions():
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert S.links_exactly("../libagpl_zgrad.so", "agpl_zgrad.o")  # (and so not agpl_hyper.o) by default, in no other library, cleaned
    assert S.linked_like("../libagpl_zgrad.so", "../libagpl_chain.so")
    for h in ("agpl_kernel_rules.h", "../../include/agpl_hyper.h", "agpl_hyper_impl.h", "../../include/agpl_zgrad.h"):
        assert "agpl_zgrad.o" in S.recompiled_by(h), h
    srcs = lambda f: open(os.path.join(CSRC, f)).read()
    assert '#include "agpl_hyper_impl.h"' in srcs("agpl_hyper.hip") and '#include "agpl_hyper_impl.h"' in srcs("agpl_zgrad.hip")
    assert "__global__" not in srcs("agpl_hyper.hip") + srcs("agpl_zgrad.hip")  # (the kernels are stated once, in the header)
    assert re.search(r"^COMMON\s*:=\s*-O3 -std=c\+\+17 -fPIC --offload-arch=\$\(ARCH\) -fvisibility=hidden -Wall -Wno-unused-function "
                     r"-fno-slp-vectorize\s*$", mk, flags=re.M)


def test_header_compiles_alone(tmp_path):
    S.header_compiles_alone("agpl_zgrad.h",
                            "return agpl_plan_inducing_grad(0, 0, 0, 0, 0, 0, 0, 0, 0, 0) == AGPL_ERR_INVALID_ARGUMENT ? 0 : 1;", tmp_path)
