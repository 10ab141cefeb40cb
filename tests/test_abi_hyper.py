"""The surface of libagpl_hyper.so (include/agpl_hyper.h), CPU-only: the header's prototypes, the library's exports and the binding's
list agree; the binding's argument types follow the header; the library holds a gfx950 code object with the gradient's kernels; the
Makefile builds and links it as the other extensions; libagpl.so keeps its 45 exports; the header compiles alone."""
import ctypes as C
import os
import re
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "augmentedgplikelihoods.jl_amd", "csrc")
INC = os.path.join(ROOT, "include")
HEADER = os.path.join(INC, "agpl_hyper.h")


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
    assert sorted(protos) == ["agpl_plan_hyper_grad"]
    out = subprocess.check_output(["nm", "-D", "--defined-only", _ffi.HY_LIB_PATH]).decode()
    assert sorted(set(re.findall(r" T (agpl_\w+)", out))) == sorted(protos) == sorted(_ffi.HY_SYMBOLS)
    lib = _ffi.hyper_lib()  # loads, resolving against libagpl.so
    for name, args in protos.items():
        fn = getattr(lib, name)
        assert list(fn.argtypes) == [_ctype(a) for a in args], name
        assert fn.restype is C.c_int32


def test_library_holds_a_gfx950_code_object():
    from agpl_amd import _ffi

    blob = open(_ffi.HY_LIB_PATH, "rb").read()
    assert b"amdgcn-amd-amdhsa--gfx950" in blob
    assert b"hy_points_kernel" in blob and b"hy_kzz_grad_kernel" in blob


def test_libagpl_keeps_its_exports():
    from agpl_amd import _ffi

    out = subprocess.check_output(["nm", "-D", "--defined-only", _ffi.LIB_PATH]).decode()
    assert len(set(re.findall(r" T (agpl_\w+)", out))) == 45 == len(_ffi.SYMBOLS)
    assert "hyper" not in out
    assert re.search(r"#define\s+AGPL_VERSION\s+121\b", open(os.path.join(INC, "agpl.h")).read())


def test_makefile_builds_and_links_the_library_as_the_other_extensions():
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert re.search(r"^HY_SRCS\s*:=.*\bagpl_hyper\.hip\b", mk, flags=re.M)
    assert re.search(r"^HY_OUT\s*\?=\s*\.\./libagpl_hyper\.so\s*$", mk, flags=re.M)
    assert re.search(r"^all:.*\$\(HY_OUT\)", mk, flags=re.M)
    assert re.search(r"^clean:\n\t.*\$\(HY_OBJS\).*\$\(HY_OUT\)", mk, flags=re.M)
    assert not re.search(r"^(SE_|PR_|CH_|KN_|JT_|IN_)?SRCS\s*:=.*\bagpl_hyper\.hip\b", mk, flags=re.M)
    rule = lambda v: re.search(r"^\$\(%s_OUT\):(.*)\n\t(.*)$" % v, mk, flags=re.M)
    new, ch = rule("HY"), rule("CH")
    assert new and ch and re.search(r"\$\(OUT\)", new.group(1))
    assert new.group(2).replace("HY_", "X_") == ch.group(2).replace("CH_", "X_")
    assert re.search(r"^%\.o:.*agpl_kernel_rules\.h.*agpl_hyper\.h", mk, flags=re.M)
    assert re.search(r"^COMMON\s*:=\s*-O3 -std=c\+\+17 -fPIC --offload-arch=\$\(ARCH\) -fvisibility=hidden -Wall -Wno-unused-function "
                     r"-fno-slp-vectorize\s*$", mk, flags=re.M)


def test_header_compiles_alone(tmp_path):
    done = 0
    for cc, std, ext in (("gcc", "-std=c11", "c"), ("g++", "-std=c++17", "cpp")):
        if shutil.which(cc) is None:
            continue
        f = tmp_path / f"t.{ext}"
        f.write_text('#include "agpl_hyper.h"\n'
                     "int main(void) { return agpl_plan_hyper_grad(0, 0, 0, 0, 0, 0, 0, 0, 0) == AGPL_ERR_INVALID_ARGUMENT ? 0 : 1; }\n")
        subprocess.check_call([cc, std, "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", INC, "-c", str(f), "-o",
                               str(tmp_path / f"t_{ext}.o")])
        done += 1
    assert done, "no host compiler"
