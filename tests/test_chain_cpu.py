"""CPU checks of the chain-prediction surface (include/agpl_chain.h, libagpl_chain.so): the header, the library's export list, the
binding and the Julia shim agree, the header shares nothing with the other three and stands alone, and the Makefile builds and
links the library as it does the other two extensions."""
import os
import re
import shutil
import subprocess

from test_julia_artifacts import header_prototypes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "augmentedgplikelihoods.jl_amd", "csrc")
INC = os.path.join(ROOT, "include")
CH_HEADER = os.path.join(INC, "agpl_chain.h")
EXT = os.path.join(ROOT, "julia", "AGPLDeviceExt.jl")


def _prototypes(path):
    src = re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)
    return {m.group(1): len([a for a in m.group(2).split(",") if a.strip()])
            for m in re.finditer(r"AGPL_API\s+[\w\s\*]+?\b(agpl_\w+)\s*\(([^;]*?)\)\s*;", src, flags=re.S)}


def test_header_declares_exactly_the_exported_symbols():
    import agpl_amd  # noqa: F401
    from agpl_amd import _ffi

    protos = _prototypes(CH_HEADER)
    assert protos == {"agpl_plan_predict_chain": 10}
    out = subprocess.check_output(["nm", "-D", "--defined-only", _ffi.CH_LIB_PATH]).decode()
    assert sorted(set(re.findall(r" T (agpl_\w+)", out))) == sorted(protos)
    assert sorted(_ffi.CH_SYMBOLS) == sorted(protos)
    _ffi.chain_lib()  # loads, resolving against libagpl.so


def test_header_shares_no_symbol_with_the_other_three():
    protos = set(_prototypes(CH_HEADER))
    assert len(header_prototypes()) == 45 and not protos & set(header_prototypes())
    for other, count in (("agpl_se.h", 4), ("agpl_predictive.h", 1)):
        theirs = _prototypes(os.path.join(INC, other))
        assert len(theirs) == count and not protos & set(theirs), other


def test_header_compiles_alone(tmp_path):
    done = 0
    for cc, std, ext in (("gcc", "-std=c11", "c"), ("g++", "-std=c++17", "cpp")):
        if shutil.which(cc) is None:
            continue
        f = tmp_path / f"t.{ext}"
        f.write_text('#include "agpl_chain.h"\n'
                     "int main(void) { return agpl_plan_predict_chain(0, 0, 0, 0, 0, 0, 0, 0, 0, 0) == AGPL_ERR_INVALID_ARGUMENT ? 0 : 1; }\n")
        subprocess.check_call([cc, std, "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", INC, "-c", str(f), "-o",
                               str(tmp_path / f"t_{ext}.o")])
        done += 1
    assert done, "no host compiler"


def test_julia_ccall_has_the_prototypes_arity():
    src = open(EXT).read()
    m = re.search(r"ccall\(\(:agpl_plan_predict_chain,\s*libagpl_chain\),\s*\w+,\s*\(([^)]*)\)", src)
    assert m and len([t for t in m.group(1).split(",") if t.strip()]) == _prototypes(CH_HEADER)["agpl_plan_predict_chain"]
    assert re.search(r"^function device_predict_chain\(", src, flags=re.M)
    assert re.search(r'^const libagpl_chain\s*=.*"libagpl_chain\.so"', src, flags=re.M)


def test_makefile_builds_and_links_the_library_as_the_other_extensions():
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert re.search(r"^CH_SRCS\s*:=.*\bagpl_chain\.hip\b", mk, flags=re.M)
    assert re.search(r"^CH_OUT\s*\?=\s*\.\./libagpl_chain\.so\s*$", mk, flags=re.M)
    assert re.search(r"^all:.*\$\(CH_OUT\)", mk, flags=re.M)
    assert re.search(r"^clean:\n\t.*\$\(CH_OBJS\).*\$\(CH_OUT\)", mk, flags=re.M)
    assert not re.search(r"^(SE_|PR_)?SRCS\s*:=.*\bagpl_chain\.hip\b", mk, flags=re.M)  # in none of the other libraries
    rule = lambda v: re.search(r"^\$\(%s_OUT\):(.*)\n\t(.*)$" % v, mk, flags=re.M)
    ch, se, pr = rule("CH"), rule("SE"), rule("PR")
    assert ch and se and pr
    assert re.search(r"\$\(OUT\)", ch.group(1)) and re.search(r"-lagpl\b.*ORIGIN", ch.group(2))
    assert ch.group(2).replace("CH_", "X_") == se.group(2).replace("SE_", "X_") == pr.group(2).replace("PR_", "X_")
    # the generator both libraries build their images with is an internal header every object depends on
    assert re.search(r"^%\.o:.*\bagpl_se_build\.h\b.*agpl_chain\.h", mk, flags=re.M)
    for f in ("agpl_features.hip", "agpl_chain.hip"):
        assert '#include "agpl_se_build.h"' in open(os.path.join(CSRC, f)).read(), f
