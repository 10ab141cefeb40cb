"""The surface of libagpl_loo.so (include/agpl_loo.h), CPU-only: the header's two prototypes, the library's exports and the binding's
list agree; the binding's argument types follow the header; the work area is the stated layout; the library holds a gfx950 code
object with the streaming kernel; the other libraries keep their exports; the Makefile builds and links it as the other extensions,
without contraction; the Python, Julia and document surfaces exist; the header compiles alone; the source holds no
float atomic and calls the plan's own marginal pass."""
import ctypes as C
import os
import re
import subprocess

import abi_support as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "augmentedgplikelihoods.jl_amd", "csrc")
INC = os.path.join(ROOT, "include")
HEADER = os.path.join(INC, "agpl_loo.h")
NAMES = ["agpl_plan_loo", "agpl_plan_loo_bytes"]
NARGS = {"agpl_plan_loo_bytes": 2, "agpl_plan_loo": 11}


def constant(name):
    src = open(os.path.join(CSRC, "agpl_loo.hip")).read()
    m = re.search(r"^\s*constexpr\s+int\s+" + name + r"\s*=\s*(\d+)\s*;", src, flags=re.M)
    assert m, name
    return int(m.group(1))


def test_header_exports_and_binding_agree():
    import agpl_amd  # noqa: F401
    from agpl_amd import _ffi

    protos = S.prototypes(HEADER)
    assert sorted(protos) == NAMES
    assert {k: len(v[1]) for k, v in protos.items()} == NARGS
    assert S.exports(_ffi.LO_LIB_PATH) == sorted(protos) == sorted(_ffi.LO_SYMBOLS)
    lib = _ffi.loo_lib()  # loads, resolving against libagpl.so
    for name, (ret, args) in protos.items():
        fn = getattr(lib, name)
        assert list(fn.argtypes) == [S.ctype(a) for a in args], name
        assert fn.restype is S.ctype(ret), name
    assert protos["agpl_plan_loo_bytes"][0] == "int64_t" and protos["agpl_plan_loo"][0] == "int32_t"


def test_work_area_bytes_are_the_stated_layout():
    from agpl_amd import _ffi

    lib = _ffi.loo_lib()
    al = lambda x: (x + 255) // 256 * 256
    parts = constant("kLooPartials")
    for N, L in ((1, 1), (257, 3), (775, 2), (10_000_000, 4), (5, 64)):
        assert lib.agpl_plan_loo_bytes(N, L) == 2 * al(4 * L * N) + 8 * L * parts
    for N, L in ((0, 1), (-3, 1), (5, 0), (5, 65)):  # sizes a plan does not take
        assert lib.agpl_plan_loo_bytes(N, L) == 0
        assert _ffi.lib().agpl_plan_bytes(C.c_int64(N), C.c_int32(256), C.c_int32(L), C.c_uint32(0)) == 0
    assert parts == 1024 and constant("kLooThreads") == 256 and constant("kLooMaxL") == 64


def test_library_holds_a_gfx950_code_object_with_the_kernels():
    from agpl_amd import _ffi

    blob = open(_ffi.LO_LIB_PATH, "rb").read()
    assert b"amdgcn-amd-amdhsa--gfx950" in blob
    for k in (b"loo_cavity_kernel", b"loo_sum_kernel"):
        assert k in blob, k
    assert b"marginal_factor_queue_kernel" not in blob  # the marginal pass stays libagpl.so's
    out = subprocess.check_output(["readelf", "-d", _ffi.LO_LIB_PATH]).decode()
    assert "libagpl.so" in out and "$ORIGIN" in out


def test_the_other_libraries_keep_their_exports():
    from agpl_amd import _ffi

    assert len(S.exports(_ffi.LIB_PATH)) == 45 == len(_ffi.SYMBOLS)
    assert not set(NAMES) & set(S.exports(_ffi.LIB_PATH))
    assert len(S.prototypes(os.path.join(INC, "agpl.h"))) == 45
    assert S.exports(_ffi.GV_LIB_PATH) == sorted(_ffi.GV_SYMBOLS) and len(_ffi.GV_SYMBOLS) == 5
    assert S.exports(_ffi.PR_LIB_PATH) == sorted(_ffi.PR_SYMBOLS)
    assert re.search(r"#define\s+AGPL_VERSION\s+121\b", open(os.path.join(INC, "agpl.h")).read())


def test_makefile_builds_and_links_the_library_as_the_other_extensions():
    assert S.links_exactly("../libagpl_loo.so", "agpl_loo.o")  # by default, in none of the other libraries, cleaned
    assert S.linked_like("../libagpl_loo.so", "../libagpl_greedy.so")
    assert S.contraction_off("agpl_loo.o")  # no contraction: a host reproduces the rule's bits
    assert "agpl_loo.o" in S.recompiled_by("../../include/agpl_loo.h")
    # what the other ABI tests pin is as it was
    assert S.contraction_off("agpl_sampler.o") and S.contraction_off("agpl_quantile.o")
    assert {S.CORE, "../libagpl_quantile.so", "../libagpl_greedy.so"} <= set(S.build_commands()[1])


def test_source_has_no_float_atomic_and_runs_the_plans_own_marginal_pass():
    src = open(os.path.join(CSRC, "agpl_loo.hip")).read()
    code = re.sub(r"//.*", "", src)
    assert "agpl_marginals_plan(" in code and "agpl_plan_state(" in code
    assert "hipMalloc" not in code and "agpl_ws_reserve" not in code and "agpl_pred_reserve" not in code  # the call allocates nothing
    calls = list(re.finditer(r"\batomic\w+\(\s*(\w+)", code))
    assert sorted(m.group(0).split("(")[0] for m in calls) == ["atomicAdd", "atomicMin"]  # info's two words: 64-bit integers
    for m in calls:
        assert re.search(r"unsigned long long \*(?:__restrict__ )?%s\b" % m.group(1), code), m.group(0)
    assert "fma(" not in code and "__fdividef" not in code and "__frcp" not in code and "rcp(" not in code


def test_python_surface_exists():
    import inspect

    import agpl_amd

    assert list(inspect.signature(agpl_amd.Plan.loo_cavity).parameters) == ["self", "gamma", "beta", "mu0"]
    sig = inspect.signature(agpl_amd.SparseCAVI.loo)
    assert list(sig.parameters) == ["self", "nsamples", "sweep"]
    assert sig.parameters["nsamples"].default == 0 and sig.parameters["sweep"].default is None
    assert callable(agpl_amd.SparseCAVI.loo_predict_y) and callable(agpl_amd.SparseCAVI.loo_cdf)
    assert "accumulate()" in agpl_amd.SparseCAVI.loo.__doc__  # the docstring says when a pass is run first
    for cls in (agpl_amd.SparseGibbs, agpl_amd.DenseGibbs):  # a chain has no sites
        assert not any(hasattr(cls, n) for n in ("loo", "loo_cdf", "loo_predict_y"))
    assert agpl_amd.LooResult.__slots__ == ("logp", "elpd", "leverage", "p_eff", "n_bad") and "LooResult" in agpl_amd.__all__


def test_julia_shim_and_documents_name_the_entry_points():
    jl = open(os.path.join(ROOT, "julia", "AGPLDeviceExt.jl")).read()
    m = re.search(r"ccall\(\(:agpl_plan_loo,\s*libagpl_loo\),\s*\w+,\s*\(([^)]*)\)", jl)
    assert m and len([t for t in m.group(1).split(",") if t.strip()]) == NARGS["agpl_plan_loo"]
    m = re.search(r"ccall\(\(:agpl_plan_loo_bytes,\s*libagpl_loo\),\s*(\w+),\s*\(([^)]*)\)", jl)
    assert m and m.group(1) == "Int64" and len([t for t in m.group(2).split(",") if t.strip()]) == NARGS["agpl_plan_loo_bytes"]
    assert re.search(r"^function device_loo_cavity\(", jl, flags=re.M)
    assert re.search(r'^const libagpl_loo = get\(ENV, "AGPL_LOO_LIB", "libagpl_loo\.so"\)', jl, flags=re.M)
    for doc in ("INTEGRATION.md", "DESIGN.md", "README.md"):
        text = open(os.path.join(ROOT, doc)).read()
        assert "agpl_plan_loo" in text and "agpl_plan_loo_bytes" in text, doc
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "### 4.27" in design and "### 4.26" in design


def test_header_states_the_rule_and_the_table():
    text = open(HEADER).read()
    for phrase in ("THE RULE", "q = var - d", "h = g * q", "t = 1 - h", "var_out = d + q / t", "u = b * q;  w = a - u;  mu_out = m0 + w / t",
                   "AGPL_PLAN_NO_MARGINALS", "lev_sum[l]", "The call allocates nothing"):
        assert phrase in text, phrase


def test_header_compiles_alone(tmp_path):
    S.header_compiles_alone("agpl_loo.h",
                            "return agpl_plan_loo_bytes(0, 0) == 0 &&\n"
                            "                        agpl_plan_loo(0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0) == AGPL_ERR_INVALID_ARGUMENT ? 0 : 1;", tmp_path)
