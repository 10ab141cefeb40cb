"""CPU checks of the predictive-distribution surface (include/agpl_predictive.h, libagpl_predictive.so): the header, the library's
export list and the binding agree, the header stands alone, and the build's default target builds the library."""
import os
import re

import abi_support as S
from test_julia_artifacts import header_prototypes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PR_HEADER = os.path.join(ROOT, "include", "agpl_predictive.h")
SE_HEADER = os.path.join(ROOT, "include", "agpl_se.h")
EXT = os.path.join(ROOT, "julia", "AGPLDeviceExt.jl")


def test_header_library_binding_and_julia_agree():
    import agpl_amd  # noqa: F401
    from agpl_amd import _ffi

    protos = S.arities(PR_HEADER)
    assert protos == {"agpl_predictive": 12}
    assert S.exports(_ffi.PR_LIB_PATH) == sorted(protos)
    assert sorted(_ffi.PR_SYMBOLS) == sorted(protos)
    assert not set(protos) & set(header_prototypes())  # agpl.h keeps its 45 entry points
    assert not set(protos) & set(S.prototypes(SE_HEADER))  # agpl_se.h its four
    m = re.search(r"ccall\(\(:agpl_predictive,\s*libagpl_predictive\),\s*\w+,\s*\(([^)]*)\)", open(EXT).read())
    assert m and len([t for t in m.group(1).split(",") if t.strip()]) == protos["agpl_predictive"]


def test_header_compiles_alone(tmp_path):
    S.header_compiles_alone("agpl_predictive.h",
                            "return agpl_predictive(0, 0, 0, 0, 0, 0, 0u, 0u, 0, 0, 0, 0) == AGPL_ERR_INVALID_ARGUMENT ? 0 : 1;", tmp_path)


def test_makefile_builds_the_library_by_default():
    assert S.links_exactly("../libagpl_predictive.so", "agpl_predictive.o")  # by default, in neither of the other libraries, cleaned
    assert S.linked_like("../libagpl_predictive.so", "../libagpl_se.so")
    assert S.contraction_off("agpl_predictive.o")
