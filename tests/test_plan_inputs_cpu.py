"""CPU checks of the plan-from-inputs surface (include/agpl_se.h, libagpl_se.so: agpl_plan_se_bytes, agpl_plan_create_se,
agpl_plan_predict, agpl_plan_features): the byte arithmetic, the header / library / binding / Julia agreement, and the generated
code of the fused build kernel (csrc/agpl_features.hip)."""
import ctypes as C
import os
import re
import subprocess

import pytest

import abi_support as S
from test_julia_artifacts import header_prototypes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "augmentedgplikelihoods.jl_amd", "csrc")
HIPCC = "/opt/rocm/bin/hipcc"
SE_HEADER = os.path.join(ROOT, "include", "agpl_se.h")
EXT = os.path.join(ROOT, "julia", "AGPLDeviceExt.jl")
NEW = ("agpl_plan_se_bytes", "agpl_plan_create_se", "agpl_plan_predict", "agpl_plan_features")


@pytest.fixture(scope="module")
def lib():
    import agpl_amd  # noqa: F401
    from agpl_amd import _ffi

    return _ffi.lib()


@pytest.fixture(scope="module")
def se(lib):
    from agpl_amd import _ffi

    return _ffi.se_lib()


def _al(x):
    return (x + 255) & ~255


def test_se_bytes_is_plan_bytes_plus_the_generator_state(lib, se):
    sel = se
    se = lambda N, M, L, D, fl=0: sel.agpl_plan_se_bytes(C.c_int64(N), C.c_int32(M), C.c_int32(L), C.c_int32(D), C.c_uint32(fl))
    pb = lambda N, M, L, fl=0: lib.agpl_plan_bytes(C.c_int64(N), C.c_int32(M), C.c_int32(L), C.c_uint32(fl))
    for N, M, L, D, fl in [(5003, 37, 1, 1, 0), (10_000, 64, 1, 3, 0), (7, 256, 4, 16, 1), (10**7, 1024, 1, 1, 0), (1, 1000, 2, 2, 1)]:
        Mp = (M + 255) // 256 * 256
        extra = _al(4 * Mp * Mp) + _al(8 * Mp * D) + _al(8 * 16)
        assert se(N, M, L, D, fl) == pb(N, M, L, fl) + extra
    for bad in [(0, 64, 1, 1), (10, 0, 1, 1), (10, 64, 0, 1), (10, 64, 65, 1), (10, 64, 1, 0), (10, 64, 1, 17), (-5, 64, 1, 1)]:
        assert se(*bad) == 0, bad
    assert se(10, 64, 1, 1, 2) == 0  # unknown flag


def test_extension_header_library_and_julia_agree(se):
    """include/agpl_se.h declares exactly the four entry points libagpl_se.so exports (and nothing of libagpl.so's), and the Julia
    extension calls each of them with the header's arity."""
    from agpl_amd import _ffi

    protos = S.arities(SE_HEADER)
    assert sorted(protos) == sorted(NEW) == sorted(_ffi.SE_SYMBOLS)
    assert protos == {"agpl_plan_se_bytes": 5, "agpl_plan_create_se": 13, "agpl_plan_predict": 6, "agpl_plan_features": 4}
    assert S.exports(_ffi.SE_LIB_PATH) == sorted(NEW)
    assert not set(NEW) & set(header_prototypes())  # agpl.h keeps its 45 entry points
    src = open(EXT).read()
    for name in NEW:
        m = re.search(r"ccall\(\(:" + name + r",\s*libagpl_se\),\s*\w+,\s*\(([^)]*)\)", src)
        assert m, name
        assert len([t for t in m.group(1).split(",") if t.strip()]) == protos[name], name


def test_extension_header_compiles_alone(tmp_path):
    """include/agpl_se.h is self-contained for a non-ctypes FFI (as agpl.h): a C11 and a C++17 unit that include only it compile."""
    S.header_compiles_alone("agpl_se.h", "return agpl_plan_se_bytes(0, 0, 0, 0, 0) == 0 ? 0 : 1;", tmp_path)


def test_makefile_builds_the_feature_source():
    assert S.links_exactly("../libagpl_se.so", "agpl_features.o")  # (and so not part of libagpl.so)


def test_fused_build_kernel_has_no_scratch_traffic(tmp_path):
    """The fused build kernel keeps its 64 accumulators, staging registers and the generator's float64 temporaries in VGPRs:
    no scratch (spill) instruction anywhere in it, in particular none in its tile loop, and a zero private segment."""
    if not os.path.exists(HIPCC):
        pytest.skip("no hipcc")
    flags = re.search(r"^COMMON\s*:=\s*(.*)$", open(os.path.join(CSRC, "Makefile")).read(), flags=re.M).group(1)
    flags = flags.replace("$(ARCH)", "gfx950").split()
    subprocess.check_call([HIPCC] + flags + ["--cuda-device-only", "-S", os.path.join(CSRC, "agpl_features.hip"), "-o", "f.s"],
                          cwd=tmp_path, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    asm = open(os.path.join(tmp_path, "f.s")).read()
    lines = asm.splitlines()
    start = next(i for i, ln in enumerate(lines) if re.match(r"^_Z\w*se_build_kernel\w*:", ln))
    end = next(i for i in range(start, len(lines)) if "s_endpgm" in lines[i])
    body = [ln.split(";")[0] for ln in lines[start:end + 1]]
    assert any("v_mfma_f32_32x32x2" in ln for ln in body), "the whitening does not run on the matrix cores"
    assert not [ln for ln in body if re.search(r"\bscratch_|buffer_\w+.*\boffen\b.*\bs\[0:3\]", ln)]
    blk = re.search(r"\.name:\s+_Z\w*se_build_kernel\w*.*?(?=\n  - |\Z)", asm, flags=re.S)
    assert blk is not None
    assert re.search(r"\.private_segment_fixed_size:\s+0\b", blk.group(0)), "private segment"
    assert re.search(r"\.vgpr_spill_count:\s+0\b", blk.group(0)), "VGPR spill"
