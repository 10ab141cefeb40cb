"""The surface of libagpl_grad.so (include/agpl_grad.h), CPU-only: the header's one prototype, the library's exports and the binding's
list agree; the binding's argument types follow the header; the library holds a gfx950 code object with the generator's derivative
mode for the four differentiable kinds and none of the plans' own mode; the sources that build plans carry no derivative
instantiation; the Makefile builds and links it as the other extensions; libagpl.so keeps its 45 exports, the libraries that share
the generator their own; the Python surface exists; the header compiles alone."""
import ctypes as C
import os
import re

import abi_support as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "augmentedgplikelihoods.jl_amd", "csrc")
INC = os.path.join(ROOT, "include")
HEADER = os.path.join(INC, "agpl_grad.h")


def test_header_exports_and_binding_agree():
    import agpl_amd  # noqa: F401
    from agpl_amd import _ffi

    protos = S.arguments(HEADER)
    assert sorted(protos) == ["agpl_plan_predict_grad"]
    assert len(protos["agpl_plan_predict_grad"]) == 5
    assert S.exports(_ffi.GR_LIB_PATH) == sorted(protos) == sorted(_ffi.GR_SYMBOLS)
    lib = _ffi.grad_lib()  # loads, resolving against libagpl.so
    for name, args in protos.items():
        fn = getattr(lib, name)
        assert list(fn.argtypes) == [S.ctype(a) for a in args], name
        assert fn.restype is C.c_int32


def test_library_holds_a_gfx950_code_object_with_the_derivative_mode_only():
    from agpl_amd import _ffi

    blob = open(_ffi.GR_LIB_PATH, "rb").read()
    assert b"amdgcn-amd-amdhsa--gfx950" in blob and b"grad_scale_kernel" in blob
    # se_build_kernel<kind, true> for every kind but Matern-1/2 (1); the plans' own mode <kind, false> is not carried here
    for kind in range(5):
        assert (b"15se_build_kernelILi%dELb1EE" % kind in blob) == (kind != 1), kind
        assert b"15se_build_kernelILi%dELb0EE" % kind not in blob, kind
    # and the libraries that build or predict from plans carry the plans' own mode only
    for path in (_ffi.SE_LIB_PATH, _ffi.KN_LIB_PATH, _ffi.CH_LIB_PATH, _ffi.JT_LIB_PATH, _ffi.PW_LIB_PATH, _ffi.HY_LIB_PATH):
        other = open(path, "rb").read()
        assert b"se_build_kernelILi0ELb0EE" in other and b"ELb1EE" not in other, path


def test_the_other_libraries_keep_their_exports():
    from agpl_amd import _ffi

    assert len(S.exports(_ffi.LIB_PATH)) == 45 == len(_ffi.SYMBOLS)
    assert "agpl_plan_predict_grad" not in S.exports(_ffi.LIB_PATH)
    assert len(S.arguments(os.path.join(INC, "agpl.h"))) == 45
    for path, syms in ((_ffi.SE_LIB_PATH, _ffi.SE_SYMBOLS), (_ffi.KN_LIB_PATH, _ffi.KN_SYMBOLS), (_ffi.CH_LIB_PATH, _ffi.CH_SYMBOLS),
                       (_ffi.JT_LIB_PATH, _ffi.JT_SYMBOLS), (_ffi.PW_LIB_PATH, _ffi.PW_SYMBOLS)):
        assert S.exports(path) == sorted(syms), path
    assert re.search(r"#define\s+AGPL_VERSION\s+121\b", open(os.path.join(INC, "agpl.h")).read())


def test_makefile_builds_and_links_the_library_as_the_other_extensions():
    assert S.links_exactly("../libagpl_grad.so", "agpl_grad.o")  # by default, in none of the other libraries, cleaned
    assert S.linked_like("../libagpl_grad.so", "../libagpl_predictive.so")
    for h in ("agpl_se_build.h", "agpl_kernel_rules.h", "../../include/agpl_grad.h"):
        assert "agpl_grad.o" in S.recompiled_by(h), h
    src = open(os.path.join(CSRC, "agpl_grad.hip")).read()
    # the generator and the rule are the shared ones, stated once; c is the rule's own limit; fixed orders; the call stays asynchronous
    assert '#include "agpl_se_build.h"' in src and "agpl_se_build_mode<true>(" in src and "agpl_marginals_plan(" in src
    assert "kernel_dvalue<double>(p->kind, 0.0" in src and "exp(" not in src
    assert "atomic" not in src and "DeviceSynchronize" not in src and "agpl_ctx_synchronize" not in src
    gen = open(os.path.join(CSRC, "agpl_se_build.h")).read()
    assert gen.count("agpl::kernel_drule<KIND, float>(") == 1 and gen.count("agpl::kernel_rule<KIND, float>(") == 1


def test_python_surface_exists():
    import agpl_amd

    assert callable(agpl_amd.Plan.predict_grad) and callable(agpl_amd.SparseCAVI.predict_grad)
    assert not hasattr(agpl_amd.SparseGibbs, "predict_grad")  # (derivatives from a chain are out of scope)


def test_julia_shim_and_documents_name_the_entry_point():
    jl = open(os.path.join(ROOT, "julia", "AGPLDeviceExt.jl")).read()
    m = re.search(r"ccall\(\(:agpl_plan_predict_grad,\s*libagpl_grad\),\s*\w+,\s*\(([^)]*)\)", jl)
    assert m and len([t for t in m.group(1).split(",") if t.strip()]) == 5
    assert "device_predict_grad" in jl
    for doc in ("INTEGRATION.md", "DESIGN.md", "README.md"):
        assert "agpl_plan_predict_grad" in open(os.path.join(ROOT, doc)).read(), doc


def test_header_compiles_alone(tmp_path):
    S.header_compiles_alone("agpl_grad.h",
                            "return agpl_plan_predict_grad(0, 0, 0, 0, 0) == AGPL_ERR_INVALID_ARGUMENT ? 0 : 1;", tmp_path)
