"""CPU checks of the chain-prediction surface (include/agpl_chain.h, libagpl_chain.so): the header, the library's export list, the
binding and the Julia shim agree, the header shares nothing with the other three and stands alone, and the Makefile builds and
links the library as it does the other two extensions."""
import os
import re

import abi_support as S
from test_julia_artifacts import header_prototypes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "augmentedgplikelihoods.jl_amd", "csrc")
INC = os.path.join(ROOT, "include")
CH_HEADER = os.path.join(INC, "agpl_chain.h")
EXT = os.path.join(ROOT, "julia", "AGPLDeviceExt.jl")


def test_header_declares_exactly_the_exported_symbols():
    import agpl_amd  # noqa: F401
    from agpl_amd import _ffi

    protos = S.arities(CH_HEADER)
    assert protos == {"agpl_plan_predict_chain": 10}
    assert S.exports(_ffi.CH_LIB_PATH) == sorted(protos)
    assert sorted(_ffi.CH_SYMBOLS) == sorted(protos)
    _ffi.chain_lib()  # loads, resolving against libagpl.so


def test_header_shares_no_symbol_with_the_other_three():
    protos = set(S.arities(CH_HEADER))
    assert len(header_prototypes()) == 45 and not protos & set(header_prototypes())
    for other, count in (("agpl_se.h", 4), ("agpl_predictive.h", 1)):
        theirs = S.arities(os.path.join(INC, other))
        assert len(theirs) == count and not protos & set(theirs), other


def test_header_compiles_alone(tmp_path):
    S.header_compiles_alone("agpl_chain.h",
                            "return agpl_plan_predict_chain(0, 0, 0, 0, 0, 0, 0, 0, 0, 0) == AGPL_ERR_INVALID_ARGUMENT ? 0 : 1;", tmp_path)


def test_julia_ccall_has_the_prototypes_arity():
    src = open(EXT).read()
    m = re.search(r"ccall\(\(:agpl_plan_predict_chain,\s*libagpl_chain\),\s*\w+,\s*\(([^)]*)\)", src)
    assert m and len([t for t in m.group(1).split(",") if t.strip()]) == S.arities(CH_HEADER)["agpl_plan_predict_chain"]
    assert re.search(r"^function device_predict_chain\(", src, flags=re.M)
    assert re.search(r'^const libagpl_chain\s*=.*"libagpl_chain\.so"', src, flags=re.M)


def test_makefile_builds_and_links_the_library_as_the_other_extensions():
    assert S.links_exactly("../libagpl_chain.so", "agpl_chain.o")  # by default, in none of the other libraries, cleaned
    assert S.linked_like("../libagpl_chain.so", "../libagpl_se.so", "../libagpl_predictive.so")
    # the generator both libraries build their images with is an internal header their objects depend on
    assert {"agpl_chain.o", "agpl_features.o"} <= S.recompiled_by("agpl_se_build.h") & S.recompiled_by("../../include/agpl_chain.h")
    for f in ("agpl_features.hip", "agpl_chain.hip"):
        assert '#include "agpl_se_build.h"' in open(os.path.join(CSRC, f)).read(), f
