"""The surface of libagpl_greedy.so (include/agpl_greedy.h), CPU-only: the header's five prototypes, the library's exports and the
binding's list agree; the binding's argument types follow the header; the library holds a gfx950 code object with the step kernel;
the other libraries keep their exports; the Makefile builds and links it as the other extensions; the Python,
Julia and document surfaces exist; the header compiles alone; the source holds no float atomic, includes the covariance rules
instead of restating them, and names its tile, unroll and partials cap."""
import ctypes as C
import os
import re

import abi_support as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "augmentedgplikelihoods.jl_amd", "csrc")
INC = os.path.join(ROOT, "include")
HEADER = os.path.join(INC, "agpl_greedy.h")
NAMES = ["agpl_greedy_begin", "agpl_greedy_bytes", "agpl_greedy_pivot", "agpl_greedy_step", "agpl_select_inducing_greedy"]
NARGS = {"agpl_greedy_bytes": 3, "agpl_greedy_begin": 11, "agpl_greedy_pivot": 12, "agpl_greedy_step": 18,
         "agpl_select_inducing_greedy": 15}


def constant(name):
    src = open(os.path.join(CSRC, "agpl_greedy.hip")).read()
    m = re.search(r"^\s*constexpr\s+int\s+" + name + r"\s*=\s*(\d+)\s*;", src, flags=re.M)
    assert m, name
    return int(m.group(1))


def test_header_exports_and_binding_agree():
    import agpl_amd  # noqa: F401
    from agpl_amd import _ffi

    protos = S.arguments(HEADER)
    assert sorted(protos) == NAMES
    assert {k: len(v) for k, v in protos.items()} == NARGS
    assert S.exports(_ffi.GV_LIB_PATH) == sorted(protos) == sorted(_ffi.GV_SYMBOLS)
    lib = _ffi.greedy_lib()  # loads, resolving against libagpl.so
    for name, args in protos.items():
        fn = getattr(lib, name)
        assert list(fn.argtypes) == [S.ctype(a) for a in args], name
        assert fn.restype is C.c_int32


def test_work_area_bytes_are_the_stated_layout():
    from agpl_amd import _ffi

    lib = _ffi.greedy_lib()
    b = C.c_int64()
    parts = constant("kGvPartials")
    for n, M in ((0, 1), (1, 1), (777, 40), (10_000_000, 512)):
        assert lib.agpl_greedy_bytes(n, M, C.byref(b)) == 0
        assert b.value == 8 * (M + 1) * n + 16 * parts
    assert 41.0e9 < b.value < 41.1e9  # the size of a plan at N = 1e7, M = 512
    E = _ffi.ERR_INVALID_ARGUMENT
    assert lib.agpl_greedy_bytes(-1, 4, C.byref(b)) == E and lib.agpl_greedy_bytes(5, 0, C.byref(b)) == E
    assert lib.agpl_greedy_bytes(5, 2049, C.byref(b)) == E and lib.agpl_greedy_bytes(5, 4, None) == E


def test_library_holds_a_gfx950_code_object_with_the_step_kernel():
    from agpl_amd import _ffi

    blob = open(_ffi.GV_LIB_PATH, "rb").read()
    assert b"amdgcn-amd-amdhsa--gfx950" in blob
    for k in (b"gv_step_kernel", b"gv_pick_kernel", b"gv_begin_kernel", b"gv_pivot_kernel"):
        assert k in blob, k
    assert b"km_step_kernel" not in blob


def test_the_other_libraries_keep_their_exports():
    from agpl_amd import _ffi

    assert len(S.exports(_ffi.LIB_PATH)) == 45 == len(_ffi.SYMBOLS)
    assert not set(NAMES) & set(S.exports(_ffi.LIB_PATH))
    assert len(S.arguments(os.path.join(INC, "agpl.h"))) == 45
    assert S.exports(_ffi.IN_LIB_PATH) == sorted(_ffi.IN_SYMBOLS) and len(_ffi.IN_SYMBOLS) == 6
    assert S.exports(_ffi.QT_LIB_PATH) == sorted(_ffi.QT_SYMBOLS)
    assert re.search(r"#define\s+AGPL_VERSION\s+121\b", open(os.path.join(INC, "agpl.h")).read())


def test_makefile_builds_and_links_the_library_as_the_other_extensions():
    assert S.links_exactly("../libagpl_greedy.so", "agpl_greedy.o")  # by default, in none of the other libraries, cleaned
    assert S.linked_like("../libagpl_greedy.so", "../libagpl_inducing.so")
    assert S.contraction_off("agpl_greedy.o")  # no contraction: every fused operation is an explicit fma
    assert "agpl_greedy.o" in S.recompiled_by("../../include/agpl_greedy.h")
    # what the other ABI tests pin is as it was
    assert S.contraction_off("agpl_sampler.o") and S.contraction_off("agpl_quantile.o")
    assert {S.CORE, "../libagpl_quantile.so"} <= set(S.build_commands()[1])


def test_source_has_no_float_atomic_and_includes_the_rules():
    src = open(os.path.join(CSRC, "agpl_greedy.hip")).read()
    code = re.sub(r"//.*", "", src)
    assert '#include "agpl_kernel_rules.h"' in src and "agpl::kernel_value<double>(" in code
    for word in (r"\bexp\(", r"\blog1p\(", r"\bexpf\(", r"\bpow\(", r"1\.7320508", r"2\.2360679", r"kernel_rule<"):
        assert not re.search(word, code), word  # no kappa restated
    calls = list(re.finditer(r"\batomic\w+\(\s*(\w+)", code))
    assert len(calls) == 2  # the status word's atomicMin, the trace's atomicAdd: 64-bit integers, never a double or a float
    for m in calls:
        assert re.search(r"unsigned long long \*(?:__restrict__ )?%s\b" % m.group(1), code), m.group(0)
    assert "__builtin_fma(" in code and "fmaf" not in code
    assert (constant("kGvTile"), constant("kGvUnroll"), constant("kGvPartials")) == (1024, 8, 1024)  # tests/test_gpu_greedy.py's shapes straddle them
    assert constant("kGvThreads") * constant("kGvPoints") == constant("kGvTile")


def test_python_surface_exists():
    import inspect

    import agpl_amd

    assert callable(agpl_amd.select_inducing_greedy) and "select_inducing_greedy" in agpl_amd.__all__
    sig = inspect.signature(agpl_amd.select_inducing_greedy)
    assert list(sig.parameters) == ["x", "M", "lengthscale", "variance", "kernel", "threshold", "ctx", "group", "return_info"]
    assert sig.parameters["threshold"].default == 1e-6 and sig.parameters["kernel"].default == "se"
    assert callable(agpl_amd.select_inducing)  # k-means stays


def test_julia_shim_and_documents_name_the_entry_points():
    jl = open(os.path.join(ROOT, "julia", "AGPLDeviceExt.jl")).read()
    m = re.search(r"ccall\(\(:agpl_select_inducing_greedy,\s*libagpl_greedy\),\s*\w+,\s*\(([^)]*)\)", jl)
    assert m and len([t for t in m.group(1).split(",") if t.strip()]) == NARGS["agpl_select_inducing_greedy"]
    assert re.search(r"^function device_select_inducing_greedy\(", jl, flags=re.M)
    assert re.search(r'^const libagpl_greedy = get\(ENV, "AGPL_GREEDY_LIB", "libagpl_greedy\.so"\)', jl, flags=re.M)
    for doc in ("INTEGRATION.md", "DESIGN.md", "README.md"):
        assert "agpl_select_inducing_greedy" in open(os.path.join(ROOT, doc)).read(), doc
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "### 4.26" in design
    for name in NAMES:
        assert name in design, name


def test_header_compiles_alone(tmp_path):
    S.header_compiles_alone("agpl_greedy.h",
                            "return agpl_greedy_bytes(0, 0, 0) == AGPL_ERR_INVALID_ARGUMENT &&\n"
                            "                        agpl_select_inducing_greedy(0, 0, 0, 0, AGPL_KERNEL_SE, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0) == AGPL_ERR_INVALID_ARGUMENT ? 0 : 1;", tmp_path)
