"""The surface of libagpl_pathwise.so (include/agpl_pathwise.h), CPU-only: the header's one prototype, the library's exports and the
binding's list agree; the binding's argument types follow the header; the library holds a gfx950 code object with the pathwise
kernels; the Makefile builds and links it as the other extensions; libagpl.so keeps its 45 exports, libagpl_hyper.so and
libagpl_zgrad.so their one each; the Python surface exists; the header compiles alone."""
import ctypes as C
import os
import re
import subprocess

import abi_support as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "augmentedgplikelihoods.jl_amd", "csrc")
INC = os.path.join(ROOT, "include")
HEADER = os.path.join(INC, "agpl_pathwise.h")


def test_header_exports_and_binding_agree():
    import agpl_amd  # noqa: F401
    from agpl_amd import _ffi

    protos = S.arguments(HEADER)
    assert sorted(protos) == ["agpl_plan_sample_paths"]
    assert len(protos["agpl_plan_sample_paths"]) == 12
    out = subprocess.check_output(["nm", "-D", "--defined-only", _ffi.PW_LIB_PATH]).decode()
    assert sorted(set(re.findall(r" T (agpl_\w+)", out))) == sorted(protos) == sorted(_ffi.PW_SYMBOLS)
    lib = _ffi.pathwise_lib()  # loads, resolving against libagpl.so
    for name, args in protos.items():
        fn = getattr(lib, name)
        assert list(fn.argtypes) == [S.ctype(a) for a in args], name
        assert fn.restype is C.c_int32


def test_library_holds_a_gfx950_code_object():
    from agpl_amd import _ffi

    blob = open(_ffi.PW_LIB_PATH, "rb").read()
    assert b"amdgcn-amd-amdhsa--gfx950" in blob
    for k in (b"pw_feature_kernel", b"pw_pack_kernel", b"pw_project_kernel", b"pw_check_kernel", b"se_build_kernel", b"se_kzz_kernel"):
        assert k in blob, k


def test_the_other_libraries_keep_their_exports():
    from agpl_amd import _ffi

    out = subprocess.check_output(["nm", "-D", "--defined-only", _ffi.LIB_PATH]).decode()
    assert len(set(re.findall(r" T (agpl_\w+)", out))) == 45 == len(_ffi.SYMBOLS)
    assert "sample_paths" not in out
    assert len(S.arguments(os.path.join(INC, "agpl.h"))) == 45
    for path, syms in ((_ffi.HY_LIB_PATH, _ffi.HY_SYMBOLS), (_ffi.ZG_LIB_PATH, _ffi.ZG_SYMBOLS), (_ffi.CH_LIB_PATH, _ffi.CH_SYMBOLS)):
        out = subprocess.check_output(["nm", "-D", "--defined-only", path]).decode()
        assert sorted(set(re.findall(r" T (agpl_\w+)", out))) == sorted(syms)
    assert re.search(r"#define\s+AGPL_VERSION\s+121\b", open(os.path.join(INC, "agpl.h")).read())


def test_makefile_builds_and_links_the_library_as_the_other_extensions():
    assert S.links_exactly("../libagpl_pathwise.so", "agpl_pathwise.o")  # by default, in none of the other libraries, cleaned
    assert S.linked_like("../libagpl_pathwise.so", "../libagpl_chain.so")
    assert "agpl_pathwise.o" in S.recompiled_by("agpl_hyper_impl.h") & S.recompiled_by("../../include/agpl_pathwise.h")
    src = open(os.path.join(CSRC, "agpl_pathwise.hip")).read()
    # the float64 set-up (L^-1) is the one agpl_hyper_impl.h states, the generator the one of agpl_se_build.h: neither is restated
    assert '#include "agpl_hyper_impl.h"' in src and "hy_linv(" in src and "agpl_se_build(" in src
    assert "se_kzz_kernel" not in src.replace("se_kzz_kernel's", "") and "agpl_gaussian_factor(" not in src
    impl = open(os.path.join(CSRC, "agpl_hyper_impl.h")).read()
    assert impl.count("agpl_gaussian_factor(") == 1 and impl.count("hy_linv(") == 2


def test_python_surface_exists():
    import agpl_amd

    assert callable(agpl_amd.spectral_frequencies) and callable(agpl_amd.Plan.sample_paths)
    assert callable(agpl_amd.SparseCAVI.sample_paths) and callable(agpl_amd.SparseGibbs.sample_paths)
    assert callable(agpl_amd.Paths.__call__)


def test_header_compiles_alone(tmp_path):
    S.header_compiles_alone("agpl_pathwise.h",
                            "return agpl_plan_sample_paths(0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0) == AGPL_ERR_INVALID_ARGUMENT ? 0 : 1;", tmp_path)
