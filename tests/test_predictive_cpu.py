"""CPU checks of the predictive-distribution surface (include/agpl_predictive.h, libagpl_predictive.so): the header, the library's
export list and the binding agree, the header stands alone, and the Makefile's default target builds the library."""
import os
import re
import shutil
import subprocess

from test_julia_artifacts import header_prototypes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "augmentedgplikelihoods.jl_amd", "csrc")
PR_HEADER = os.path.join(ROOT, "include", "agpl_predictive.h")
SE_HEADER = os.path.join(ROOT, "include", "agpl_se.h")
EXT = os.path.join(ROOT, "julia", "AGPLDeviceExt.jl")


def _prototypes(path):
    src = re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)
    return {m.group(1): len([a for a in m.group(2).split(",") if a.strip()])
            for m in re.finditer(r"AGPL_API\s+[\w\s\*]+?\b(agpl_\w+)\s*\(([^;]*?)\)\s*;", src, flags=re.S)}


def test_header_library_binding_and_julia_agree():
    import agpl_amd  # noqa: F401
    from agpl_amd import _ffi

    protos = _prototypes(PR_HEADER)
    assert protos == {"agpl_predictive": 12}
    out = subprocess.check_output(["nm", "-D", "--defined-only", _ffi.PR_LIB_PATH]).decode()
    assert sorted(set(re.findall(r" T (agpl_\w+)", out))) == sorted(protos)
    assert sorted(_ffi.PR_SYMBOLS) == sorted(protos)
    assert not set(protos) & set(header_prototypes())  # agpl.h keeps its 45 entry points
    assert not set(protos) & set(_prototypes(SE_HEADER))  # agpl_se.h its four
    m = re.search(r"ccall\(\(:agpl_predictive,\s*libagpl_predictive\),\s*\w+,\s*\(([^)]*)\)", open(EXT).read())
    assert m and len([t for t in m.group(1).split(",") if t.strip()]) == protos["agpl_predictive"]


def test_header_compiles_alone(tmp_path):
    done = 0
    for cc, std, ext in (("gcc", "-std=c11", "c"), ("g++", "-std=c++17", "cpp")):
        if shutil.which(cc) is None:
            continue
        f = tmp_path / f"t.{ext}"
        f.write_text('#include "agpl_predictive.h"\n'
                     "int main(void) { return agpl_predictive(0, 0, 0, 0, 0, 0, 0u, 0u, 0, 0, 0, 0) == AGPL_ERR_INVALID_ARGUMENT ? 0 : 1; }\n")
        subprocess.check_call([cc, std, "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), "-c",
                               str(f), "-o", str(tmp_path / f"t_{ext}.o")])
        done += 1
    assert done, "no host compiler"


def test_makefile_builds_the_library_by_default():
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert re.search(r"^PR_SRCS\s*:=.*\bagpl_predictive\.hip\b", mk, flags=re.M)
    assert re.search(r"^PR_OUT\s*\?=\s*\.\./libagpl_predictive\.so\s*$", mk, flags=re.M)
    assert re.search(r"^all:.*\$\(PR_OUT\)", mk, flags=re.M)
    assert re.search(r"^clean:\n\t.*\$\(PR_OBJS\).*\$\(PR_OUT\)", mk, flags=re.M)
    assert not re.search(r"^(SE_)?SRCS\s*:=.*\bagpl_predictive\.hip\b", mk, flags=re.M)  # in neither of the other libraries
    assert re.search(r"^\$\(PR_OUT\):.*\$\(OUT\)\n\t.*-lagpl\b.*ORIGIN", mk, flags=re.M)  # linked as libagpl_se.so is
    assert re.search(r"^[^\n#]*\bagpl_predictive\.o\b[^\n]*:\s*EXTRA\s*:=\s*\$\(NOFMA\)", mk, flags=re.M)
