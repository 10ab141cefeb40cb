"""CPU tests of tests/joint_reference.py, the yardstick of the GPU tests of agpl_plan_predict_cov, and of the library's surface:

* on the data of every GPU case a numpy model of the documented arithmetic (split planes, dropped lo lo, float32 accumulation over
  Mp, the float32 kernel rule) stays inside the element-wise bars, and every wrong variant that the case's data can show leaves them:
  the bars can tell a wrong kernel from a right one before any GPU run;
* the header, the library's export list, the binding's argument types and the Julia shim agree; the Makefile builds and links the
  library as it does the other extensions; libagpl.so keeps its 45 exports.
"""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import abi_support as S
import joint_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "augmentedgplikelihoods.jl_amd", "csrc")
INC = os.path.join(ROOT, "include")
JT_HEADER = os.path.join(INC, "agpl_joint.h")
EXT = os.path.join(ROOT, "julia", "AGPLDeviceExt.jl")

CASES = [(c, False) for c in R.TIGHT + [R.SAMPLE]] + [(R.FRESH, True)]


@pytest.fixture(scope="module")
def worlds():
    """Per case: the reference with the images' exact features, its bars, and what the model needs -- computed once."""
    out = {}
    for c, fresh in CASES:
        d = R.case_data(c, fresh)
        e = R.plan_scale_exp(d.s2)
        img_a, Fa = R.feature_image(R.phi_f64(c.kind, d.xa, d.z, d.ell, d.s2), e)
        img_b, Fb = (img_a, Fa) if c.sym else R.feature_image(R.phi_f64(c.kind, d.xb, d.z, d.ell, d.s2), e)
        U = R.u_of_g(d.G)
        r2 = R.scaled_sqdist(d.xa, d.xb, d.ell)
        W = R.w_of_u(U)
        ref = R.reference(Fa, Fb, W, d.s2 * R.kappa(c.kind, r2))
        out[c.id, fresh] = (d, e, img_a, img_b, U, ref, R.bars(Fa, Fb, W, c.kind, r2, d.s2, R.plan_padded(c.M), e))
    return out


def _model(c, w, mutate=None):
    d, e, img_a, img_b, U, _, _ = w
    return R.model(img_a, img_b, U, c.kind, d.xa, d.xb, d.ell, d.s2, e, mutate=mutate).astype(np.float64)


@pytest.mark.parametrize("c,fresh", CASES, ids=[c.id + ("-fresh" if f else "") for c, f in CASES])
def test_the_model_stays_inside_the_bars(worlds, c, fresh):
    w = worlds[c.id, fresh]
    ref, bars = w[5], w[6]
    err = np.abs(_model(c, w) - ref)
    print(f"max err {err.max():.3e}, max err / bar {np.max(err / bars.total):.3f}, max bar / max |ref| {bars.total.max() / np.abs(ref).max():.2e}")
    assert (err <= bars.total).all(), np.max(err / bars.total)
    if fresh:  # U = I: W = 0 exactly, the result is the float32 kernel within the kernel term's own bar
        assert (err[0] <= bars.k).all()


@pytest.mark.parametrize("mutate", R.MUTATIONS)
@pytest.mark.parametrize("c,fresh", CASES, ids=[c.id + ("-fresh" if f else "") for c, f in CASES])
def test_every_wrong_variant_leaves_the_bars(worlds, c, fresh, mutate):
    w = worlds[c.id, fresh]
    ref, bars = w[5], w[6]
    err = np.abs(_model(c, w, mutate) - ref)
    if R.visible(mutate, c, fresh):
        assert (err > bars.total).any(), (mutate, np.max(err / bars.total))
    else:  # the data cannot show it: the variant computes the same thing
        assert (err <= bars.total).all()


def test_every_variant_is_visible_somewhere_and_every_value_of_the_issue_occurs():
    for m in R.MUTATIONS:
        assert any(R.visible(m, c, f) for c, f in CASES), m
    assert {c.M for c in R.TIGHT} == {5, 64, 256, 300} and {c.L for c in R.TIGHT} == {1, 3} and {c.D for c in R.TIGHT} == {1, 2, 16}
    assert {c.kind for c in R.TIGHT} == set(R.KINDS)
    assert {c.Na for c in R.TIGHT} == {c.Nb for c in R.TIGHT} == {1, 127, 128, 129, 257}
    assert {R.plan_padded(c.M) for c in R.TIGHT} == {256, 512}


def test_float32_rule_is_within_its_bar_of_the_float64_rule():
    r2 = np.concatenate([[0.0], np.logspace(-12, 3, 400)])
    for kind in R.KINDS:
        k64, k32 = R.kappa(kind, r2), R.kappa(kind, r2, np.float32(R.ALPHA), np.float32).astype(np.float64)
        bar = k64 * (8.0 * R.exponent(kind, r2) + 8.0) * 2.0 ** -24
        ok = k64 > 1e-30  # below, float32 is subnormal or zero
        assert (np.abs(k32 - k64)[ok] <= bar[ok]).all(), kind


# ---- the surface ------------------------------------------------------------------------------------------------------------------------

def test_header_declares_exactly_the_exported_symbol():
    import agpl_amd  # noqa: F401
    from agpl_amd import _ffi

    assert S.arities(JT_HEADER) == {"agpl_plan_predict_cov": 7}
    assert S.exports(_ffi.JT_LIB_PATH) == ["agpl_plan_predict_cov"]
    assert _ffi.JT_SYMBOLS == ["agpl_plan_predict_cov"]
    _ffi.joint_lib()  # loads, resolving against libagpl.so


def test_libagpl_keeps_its_exports():
    from agpl_amd import _ffi

    out = subprocess.check_output(["nm", "-D", "--defined-only", _ffi.LIB_PATH]).decode()
    assert len(S.exports(_ffi.LIB_PATH)) == 45 == len(_ffi.SYMBOLS)
    assert "agpl_plan_predict_cov" not in out
    assert re.search(r"#define\s+AGPL_VERSION\s+121\b", open(os.path.join(INC, "agpl.h")).read())


def test_header_binding_and_julia_agree_on_the_argument_types():
    from agpl_amd import _ffi

    args = S.prototypes(JT_HEADER)["agpl_plan_predict_cov"][1]
    want_c = [C.c_int64 if re.match(r"int64_t\s+\w+$", a) else C.c_void_p for a in args]
    assert [("*" in a) or bool(re.match(r"int64_t\s+\w+$", a)) for a in args] == [True] * 7
    fn = _ffi.joint_lib().agpl_plan_predict_cov
    assert list(fn.argtypes) == want_c and fn.restype is C.c_int32
    src = open(EXT).read()
    m = re.search(r"ccall\(\(:agpl_plan_predict_cov,\s*libagpl_joint\),\s*(\w+),\s*\(([^)]*)\)", src)
    assert m and m.group(1) == "Int32"
    julia = [t.strip() for t in m.group(2).split(",") if t.strip()]
    assert julia == ["Int64" if t is C.c_int64 else "Ptr{Cvoid}" for t in want_c]
    assert re.search(r"^function device_predict_cov\(", src, flags=re.M)
    assert re.search(r'^const libagpl_joint\s*=.*"libagpl_joint\.so"', src, flags=re.M)


def test_makefile_builds_and_links_the_library_as_the_other_extensions():
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert S.links_exactly("../libagpl_joint.so", "agpl_joint.o")  # by default, in none of the other libraries, cleaned
    assert S.linked_like("../libagpl_joint.so", "../libagpl_chain.so")
    assert "agpl_joint.o" in S.recompiled_by("agpl_se_build.h") & S.recompiled_by("../../include/agpl_joint.h")
    assert re.search(r"^COMMON\s*:=\s*-O3 -std=c\+\+17 -fPIC --offload-arch=\$\(ARCH\) -fvisibility=hidden -Wall -Wno-unused-function "
                     r"-fno-slp-vectorize\s*$", mk, flags=re.M)
    assert '#include "agpl_se_build.h"' in open(os.path.join(CSRC, "agpl_joint.hip")).read()


def test_header_compiles_alone(tmp_path):
    S.header_compiles_alone("agpl_joint.h", "return agpl_plan_predict_cov(0, 0, 0, 0, 0, 0, 0) == AGPL_ERR_INVALID_ARGUMENT ? 0 : 1;", tmp_path)
