"""The surface of libagpl_pathwise.so (include/agpl_pathwise.h), CPU-only: the header's one prototype, the library's exports and the
binding's list agree; the binding's argument types follow the header; the library holds a gfx950 code object with the pathwise
kernels; the Makefile builds and links it as the other extensions; libagpl.so keeps its 45 exports, libagpl_hyper.so and
libagpl_zgrad.so their one each; the Python surface exists; the header compiles alone."""
import ctypes as C
import os
import re
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "augmentedgplikelihoods.jl_amd", "csrc")
INC = os.path.join(ROOT, "include")
HEADER = os.path.join(INC, "agpl_pathwise.h")


def _prototypes(path):
    src = re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)
    return {m.group(1): [a.strip() for a in m.group(2).split(",") if a.strip()]
            for m in re.finditer(r"AGPL_API\s+[\w\s\*]+?\b(agpl_\w+)\s*\(([^;]*?)\)\s*;", src, flags=re.S)}


def _ctype(arg):
    if "*" in arg:
        return C.c_void_p
    return {"int64_t": C.c_int64, "int32_t": C.c_int32, "double": C.c_double}[arg.split()[0]]


def test_header_exports_and_binding_agree():
    import agpl_amd  # noqa: F401
    from agpl_amd import _ffi

    protos = _prototypes(HEADER)
    assert sorted(protos) == ["agpl_plan_sample_paths"]
    assert len(protos["agpl_plan_sample_paths"]) == 12
    out = subprocess.check_output(["nm", "-D", "--defined-only", _ffi.PW_LIB_PATH]).decode()
    assert sorted(set(re.findall(r" T (agpl_\w+)", out))) == sorted(protos) == sorted(_ffi.PW_SYMBOLS)
    lib = _ffi.pathwise_lib()  # loads, resolving against libagpl.so
    for name, args in protos.items():
        fn = getattr(lib, name)
        assert list(fn.argtypes) == [_ctype(a) for a in args], name
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
    assert len(_prototypes(os.path.join(INC, "agpl.h"))) == 45
    for path, syms in ((_ffi.HY_LIB_PATH, _ffi.HY_SYMBOLS), (_ffi.ZG_LIB_PATH, _ffi.ZG_SYMBOLS), (_ffi.CH_LIB_PATH, _ffi.CH_SYMBOLS)):
        out = subprocess.check_output(["nm", "-D", "--defined-only", path]).decode()
        assert sorted(set(re.findall(r" T (agpl_\w+)", out))) == sorted(syms)
    assert re.search(r"#define\s+AGPL_VERSION\s+121\b", open(os.path.join(INC, "agpl.h")).read())


def test_makefile_builds_and_links_the_library_as_the_other_extensions():
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert re.search(r"^PW_SRCS\s*:=\s*agpl_pathwise\.hip\s*$", mk, flags=re.M)
    assert re.search(r"^PW_OUT\s*\?=\s*\.\./libagpl_pathwise\.so\s*$", mk, flags=re.M)
    assert re.search(r"^all:.*\$\(PW_OUT\)", mk, flags=re.M)
    assert re.search(r"^clean:\n\t.*\$\(PW_OBJS\).*\$\(PW_OUT\)", mk, flags=re.M)
    rule = lambda v: re.search(r"^\$\(%s_OUT\):(.*)\n\t(.*)$" % v, mk, flags=re.M)
    new, ch = rule("PW"), rule("CH")
    assert new and ch and re.search(r"\$\(OUT\)", new.group(1))
    assert new.group(2).replace("PW_", "X_") == ch.group(2).replace("CH_", "X_")
    assert re.search(r"^%\.o:.*agpl_hyper_impl\.h.*agpl_pathwise\.h", mk, flags=re.M)
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
    done = 0
    for cc, std, ext in (("gcc", "-std=c11", "c"), ("g++", "-std=c++17", "cpp")):
        if shutil.which(cc) is None:
            continue
        f = tmp_path / f"t.{ext}"
        f.write_text('#include "agpl_pathwise.h"\n'
                     "int main(void) { return agpl_plan_sample_paths(0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0) == AGPL_ERR_INVALID_ARGUMENT ? 0 : 1; }\n")
        subprocess.check_call([cc, std, "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", INC, "-c", str(f), "-o",
                               str(tmp_path / f"t_{ext}.o")])
        done += 1
    assert done, "no host compiler"
