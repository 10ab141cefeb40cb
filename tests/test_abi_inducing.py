"""The surface of libagpl_inducing.so (include/agpl_inducing.h), CPU-only: the header's prototypes, the library's exports and the
binding's list agree; the binding's argument types follow the header; the library holds a gfx950 code object; the Makefile builds and
links it as the other extensions; libagpl.so keeps its 45 exports; the Julia shim calls the convenience entry with matching types."""
import ctypes as C
import os
import re
import subprocess

import abi_support as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "augmentedgplikelihoods.jl_amd", "csrc")
INC = os.path.join(ROOT, "include")
HEADER = os.path.join(INC, "agpl_inducing.h")
EXT = os.path.join(ROOT, "julia", "AGPLDeviceExt.jl")


def test_header_exports_and_binding_agree():
    import agpl_amd  # noqa: F401
    from agpl_amd import _ffi

    protos = S.arguments(HEADER)
    assert len(protos) == 6
    out = subprocess.check_output(["nm", "-D", "--defined-only", _ffi.IN_LIB_PATH]).decode()
    assert sorted(set(re.findall(r" T (agpl_\w+)", out))) == sorted(protos) == sorted(_ffi.IN_SYMBOLS)
    lib = _ffi.inducing_lib()  # loads, resolving against libagpl.so
    for name, args in protos.items():
        fn = getattr(lib, name)
        assert list(fn.argtypes) == [S.ctype(a) for a in args], name
        assert fn.restype is C.c_int32


def test_library_holds_a_gfx950_code_object():
    from agpl_amd import _ffi

    blob = open(_ffi.IN_LIB_PATH, "rb").read()
    assert b"amdgcn-amd-amdhsa--gfx950" in blob
    assert b"km_step_kernel" in blob and b"km_centres_kernel" in blob


def test_quanta_is_a_pure_host_function_and_matches_the_reference_rule():
    import agpl_amd as A
    import inducing_reference as R

    for bound, N, D in [(8.5, 5000, 1), (1.0, 4096, 16), (0.3, 10 ** 7, 16), (1e6, 300, 3), (37.2, 20000, 3), (2.0 ** -30, 9, 5)]:
        assert A.kmeans_quanta(bound, N, D) == R.quanta(bound, N, D)
    for bad in [(0.0, 10, 1), (float("inf"), 10, 1), (float("nan"), 10, 1), (1.0, 0, 1), (1.0, 10, 17), (-1.0, 10, 1)]:
        try:
            A.kmeans_quanta(*bad)
        except A.ArgumentError:
            continue
        raise AssertionError(bad)


def test_libagpl_keeps_its_exports():
    from agpl_amd import _ffi

    out = subprocess.check_output(["nm", "-D", "--defined-only", _ffi.LIB_PATH]).decode()
    assert len(set(re.findall(r" T (agpl_\w+)", out))) == 45 == len(_ffi.SYMBOLS)
    assert "kmeans" not in out
    assert re.search(r"#define\s+AGPL_VERSION\s+121\b", open(os.path.join(INC, "agpl.h")).read())


def test_julia_shim_calls_the_convenience_entry_with_the_header_types():
    args = S.arguments(HEADER)["agpl_select_inducing_kmeans"]
    src = open(EXT).read()
    m = re.search(r"ccall\(\(:agpl_select_inducing_kmeans,\s*libagpl_inducing\),\s*(\w+),\s*\(([^)]*)\)", src)
    assert m and m.group(1) == "Int32"
    julia = [t.strip() for t in m.group(2).split(",") if t.strip()]
    want = {C.c_void_p: "Ptr{Cvoid}", C.c_int64: "Int64", C.c_int32: "Int32", C.c_double: "Float64"}
    assert julia == [want[S.ctype(a)] for a in args]
    assert re.search(r"^function device_select_inducing\(", src, flags=re.M)
    assert re.search(r'^const libagpl_inducing\s*=.*"libagpl_inducing\.so"', src, flags=re.M)


def test_makefile_builds_and_links_the_library_as_the_other_extensions():
    assert S.links_exactly("../libagpl_inducing.so", "agpl_inducing.o")  # by default, in none of the other libraries, cleaned
    assert S.linked_like("../libagpl_inducing.so", "../libagpl_chain.so")
    assert "agpl_inducing.o" in S.recompiled_by("agpl_random.h") & S.recompiled_by("../../include/agpl_inducing.h")


def test_header_compiles_alone(tmp_path):
    S.header_compiles_alone("agpl_inducing.h",
                            "return agpl_kmeans_seed(0, 0, 0, 0, 0, 0, 0, 0, 0) == AGPL_ERR_INVALID_ARGUMENT ? 0 : 1;", tmp_path)
