"""The squared exponential x Matern kinds' rules (csrc/agpl_kernel_rules.h), compiled alone for the host with g++ as
tests/test_matern_product_rules_cpu.py compiles them: 70 and 72 are known beside the twelve older kinds and nothing else in -2 ... 79
is, the new predicate is theirs alone and every older predicate is false for them, the kinds carry no parameter, and the scale, p, t
and c0 are the closed forms.  Fails on the parent (no such enumerators)."""
import os
import subprocess

import numpy as np
import pytest

from test_additive_se_rules_cpu import CSRC, ROCM

SRC = r"""
#include <cmath>
#define _Float16 short
static inline double sinpi(double v) { return std::sin(M_PI * v); }
static inline double cospi(double v) { return std::cos(M_PI * v); }
#include "agpl_kernel_rules.h"
template <int K> void rules() {
    for (double a : {0.0, 0.5, 3.0, 40.0})
        printf("rule %d %.17g %.17g %.17g %.9g %.9g %.17g %.17g\n", K, a, agpl::kernel_se_matern_pterm<K, double>(a),
               agpl::kernel_se_matern_dpterm<K, double>(a), (double)agpl::kernel_se_matern_pterm<K, float>((float)a),
               (double)agpl::kernel_se_matern_dpterm<K, float>((float)a), agpl::kernel_se_matern_pterm_value(K, a),
               agpl::kernel_se_matern_dpterm_value(K, a));
    double s, P;
    agpl::kernel_se_matern_last(K, 3.0, -0.5, s, P);
    printf("const %d %.17g %.17g %.17g %.17g %.17g %d %d %.17g %.17g\n", K, agpl::kernel_se_matern_scale(K), agpl::kernel_se_matern_curvature(K, 2, 3),
           agpl::kernel_se_matern_curvature(K, 1, 3), s, P, (int)agpl::kernel_has_param(K),
           (int)(agpl::kernel_param_refused(K, -1.0, 1e300, false) != nullptr), (double)agpl::kernel_rule<K, float>(1.0, 0.0),
           agpl::kernel_drule<K, double>(1.0, 0.0));
}
int main() {
    for (int k = -2; k < 80; ++k)
        printf("kind %d %d %d %d %d %d %d %d %d\n", k, (int)agpl::kernel_kind_known(k), (int)agpl::kernel_kind_se_matern(k), (int)agpl::kernel_kind_product(k),
               (int)agpl::kernel_kind_sum(k), (int)agpl::kernel_kind_additive(k), (int)agpl::kernel_kind_additive2(k), (int)agpl::kernel_kind_warps(k),
               (int)agpl::kernel_kind_modulated(k));
    rules<AGPL_KERNEL_SE_MATERN32>();
    rules<AGPL_KERNEL_SE_MATERN52>();
}
"""
FORMS = {70: (np.sqrt(3.0), lambda a: 1 + a, lambda a: -3.0, 3.0), 72: (np.sqrt(5.0), lambda a: 1 + a + a * a / 3, lambda a: -5 / 3 * (1 + a), 5 / 3)}


@pytest.fixture(scope="module")
def rows(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("rules_se_matern")
    (tmp / "rules.cpp").write_text(SRC)
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-D__HIP_PLATFORM_AMD__", "-I", os.path.join(ROCM, "include"), "-I", CSRC,
                    str(tmp / "rules.cpp"), "-o", str(tmp / "rules")], check=True)
    return [ln.split() for ln in subprocess.run([str(tmp / "rules")], capture_output=True, text=True, check=True).stdout.splitlines()]


def test_kinds_70_and_72_and_their_predicates(rows):
    kinds = {int(r[1]): tuple(int(v) for v in r[2:]) for r in rows if r[0] == "kind"}
    assert len(kinds) == 82 and [k for k, v in kinds.items() if v[0]] == [0, 1, 2, 3, 4, 6, 8, 10, 14, 40, 64, 66, 70, 72]
    assert [k for k, v in kinds.items() if v[1]] == [70, 72] and kinds[70] == kinds[72] == (1, 1, 0, 0, 0, 0, 0, 0)


def test_polynomials_scale_and_curvature_are_the_closed_forms(rows):
    got = [r for r in rows if r[0] == "rule"]
    assert len(got) == 8
    for r in got:
        (_, p, t, _), a, v = FORMS[int(r[1])], float(r[2]), [float(s) for s in r[3:]]
        assert abs(v[0] - p(a)) <= 2 ** -51 * p(a) and abs(v[1] - t(a)) <= 2 ** -51 * abs(t(a)) and v[4:] == v[:2]
        assert abs(v[2] - p(a)) <= 2 ** -22 * p(a) and abs(v[3] - t(a)) <= 2 ** -22 * abs(t(a))
    consts = [r for r in rows if r[0] == "const"]
    assert len(consts) == 2
    for r in consts:  # scale; c0 in the last dimension, 1 in a leading one; s and P of r_lead^2 = 3, u = -0.5; no parameter, none refused
        (c, p, _, c0), v = FORMS[int(r[1])], [float(s) for s in r[2:]]
        assert v[0] == c and abs(v[1] - c0) <= 2 ** -52 and v[2] == 1.0 and abs(v[3] - (1.5 + 0.5 * c)) <= 2 ** -51 * 3
        assert abs(v[4] - p(0.5 * c)) <= 2 ** -51 * p(0.5 * c) and v[5:] == [0, 0, 0, 0]  # (kernel_rule and kernel_drule give 0)


def test_python_names_and_refusals():
    from agpl_amd import _ffi, sparse

    assert sparse.kernel_kind("se_matern32") == (70, 0.0) and sparse.kernel_kind("se_matern52") == (72, 0.0)
    with pytest.raises(_ffi.ArgumentError, match="kernel must be"):  # (a parameter where the kind has none: tests/test_kernels_cpu.py's case)
        sparse.kernel_kind(("se_matern52", 1.0))
    with pytest.raises(_ffi.AGPLError, match="select_inducing_greedy") as e:
        sparse.select_inducing(None, 4, kernel="se_matern32")
    assert e.value.code == _ffi.ERR_UNSUPPORTED
