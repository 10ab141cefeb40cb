"""The surface of libagpl_quantile.so (include/agpl_quantile.h), CPU-only: the header's two prototypes, the library's exports and the
binding's list agree; the binding's argument types follow the header; the library holds a gfx950 code object with both kernels; the
rules over q(f) are stated once, in the header both translation units include, and their constants once, in agpl_predictive.hip; the
Makefile builds and links it as the other extensions; libagpl.so keeps its 45 exports and AGPL_VERSION 121; the Python and Julia
surfaces exist; the header compiles alone."""
import ctypes as C
import os
import re

import abi_support as S
import seam_shapes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "augmentedgplikelihoods.jl_amd", "csrc")
INC = os.path.join(ROOT, "include")
HEADER = os.path.join(INC, "agpl_quantile.h")
NAMES = ["agpl_predictive_cdf", "agpl_predictive_quantile"]


def test_header_exports_and_binding_agree():
    import agpl_amd  # noqa: F401
    from agpl_amd import _ffi

    protos = S.arguments(HEADER)
    assert sorted(protos) == NAMES
    assert len(protos["agpl_predictive_cdf"]) == 8 and len(protos["agpl_predictive_quantile"]) == 8
    assert [a.split()[0] for a in protos["agpl_predictive_quantile"] if "*" not in a] == ["int64_t", "int32_t"]
    assert S.exports(_ffi.QT_LIB_PATH) == sorted(protos) == sorted(_ffi.QT_SYMBOLS)
    lib = _ffi.quantile_lib()  # loads, resolving against libagpl.so
    for name, args in protos.items():
        fn = getattr(lib, name)
        assert list(fn.argtypes) == [S.ctype(a) for a in args], name
        assert fn.restype is C.c_int32


def test_library_holds_a_gfx950_code_object_with_both_kernels():
    from agpl_amd import _ffi

    blob = open(_ffi.QT_LIB_PATH, "rb").read()
    assert b"amdgcn-amd-amdhsa--gfx950" in blob and b"cdf_kernel" in blob and b"quantile_kernel" in blob
    assert b"predictive_kernel" not in blob and b"predictive_cat_kernel" not in blob  # the rules only, not the predictive's kernels


def test_the_other_libraries_keep_their_exports():
    from agpl_amd import _ffi

    assert len(S.exports(_ffi.LIB_PATH)) == 45 == len(_ffi.SYMBOLS)
    assert not set(NAMES) & set(S.exports(_ffi.LIB_PATH))
    assert len(S.arguments(os.path.join(INC, "agpl.h"))) == 45
    assert S.exports(_ffi.PR_LIB_PATH) == sorted(_ffi.PR_SYMBOLS) == ["agpl_predictive"]
    assert re.search(r"#define\s+AGPL_VERSION\s+121\b", open(os.path.join(INC, "agpl.h")).read())


def test_the_rules_and_their_constants_are_stated_once():
    pred = open(os.path.join(CSRC, "agpl_predictive.hip")).read()
    rules = open(os.path.join(CSRC, "agpl_predictive_rules.h")).read()
    src = open(os.path.join(CSRC, "agpl_quantile.hip")).read()
    for fn in ("sig_terms(double f)", "double peak_integral(", "void sigma_moments(", "double studentt_logp(", "double laplace_logp(",
               "bool bad_marginal("):
        assert rules.count(fn) == 1 and fn not in pred and fn not in src, fn
    assert '#include "agpl_predictive_rules.h"' in pred
    assert re.search(r'#define AGPL_PREDICTIVE_RULES_ONLY\n#include "agpl_predictive\.hip"', src)
    for name in ("kBlock", "kGrid", "kSpan", "kPoleCap", "kMaxHalf"):
        assert re.search(r"^constexpr\s+\w+\s+" + name + r"\s*=", pred, flags=re.M), name
        assert not re.search(r"constexpr\s+\w+\s+" + name + r"\b", rules + src), name
    assert seam_shapes.constant("kBlock") == 256  # the shapes of tests/test_gpu_quantile.py straddle it
    # one lane per point: no reductions, no allocation, the call stays asynchronous
    for word in ("atomic", "hipMalloc", "DeviceSynchronize", "agpl_ctx_synchronize", "__shfl"):
        assert word not in src, word
    assert "sigma_moments(" in src and "laplace_logp(" in src and "bad_marginal(" in src


def test_makefile_builds_and_links_the_library_as_the_other_extensions():
    assert S.links_exactly("../libagpl_quantile.so", "agpl_quantile.o")  # by default, in none of the other libraries, cleaned
    assert S.linked_like("../libagpl_quantile.so", "../libagpl_predictive.so")
    for h in ("agpl_predictive_rules.h", "../../include/agpl_quantile.h", "agpl_predictive.hip"):  # (the last: its constants, included)
        assert "agpl_quantile.o" in S.recompiled_by(h), h
    for obj in ("agpl_sampler.o", "agpl_predictive.o", "agpl_quantile.o"):  # no contraction, as the predictive
        assert S.contraction_off(obj), obj


def test_python_surface_exists():
    import agpl_amd

    assert callable(agpl_amd.predictive_cdf) and callable(agpl_amd.predictive_quantile)
    assert callable(agpl_amd.Plan.predict_cdf) and callable(agpl_amd.Plan.predict_quantiles)
    assert callable(agpl_amd.SparseCAVI.predict_cdf) and callable(agpl_amd.SparseCAVI.predict_quantiles)
    assert not hasattr(agpl_amd.SparseGibbs, "predict_cdf") and not hasattr(agpl_amd.SparseGibbs, "predict_quantiles")


def test_julia_shim_and_documents_name_the_entry_points():
    jl = open(os.path.join(ROOT, "julia", "AGPLDeviceExt.jl")).read()
    for name in NAMES:
        m = re.search(r"ccall\(\(:%s,\s*libagpl_quantile\),\s*\w+,\s*\(([^)]*)\)" % name, jl)
        assert m and len([t for t in m.group(1).split(",") if t.strip()]) == 8, name
        for doc in ("INTEGRATION.md", "DESIGN.md", "README.md"):
            assert name in open(os.path.join(ROOT, doc)).read(), (doc, name)
    assert "device_predictive_cdf" in jl and "device_predictive_quantile" in jl
    assert "### 4.25" in open(os.path.join(ROOT, "DESIGN.md")).read()


def test_header_compiles_alone(tmp_path):
    S.header_compiles_alone("agpl_quantile.h",
                            "return agpl_predictive_cdf(0, 0, 0, 0, 0, 0, 0, 0) == AGPL_ERR_INVALID_ARGUMENT &&\n"
                            "                        agpl_predictive_quantile(0, 0, 0, 0, 0, 0, 0, 0) == AGPL_ERR_INVALID_ARGUMENT ? 0 : 1;", tmp_path)
