"""The product Matern kinds' rules (csrc/agpl_kernel_rules.h), compiled alone for the host with g++ as
tests/test_additive2_se_rules_cpu.py compiles them: 64 and 66 are known and 65, 67 are not, the product predicate is theirs alone, the
sum / warp / modulation predicates are false for them, p, t and c0 are the closed forms and the kinds carry no parameter.
Fails on the parent (no such enumerators)."""
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
        printf("rule %d %.17g %.17g %.17g %.9g %.9g %.17g %.17g\n", K, a, agpl::kernel_pterm<K, double>(a), agpl::kernel_dpterm<K, double>(a),
               (double)agpl::kernel_pterm<K, float>((float)a), (double)agpl::kernel_dpterm<K, float>((float)a), agpl::kernel_pterm_value(K, a),
               agpl::kernel_dpterm_value(K, a));
    printf("const %d %.17g %.17g %d %d %.17g %.17g\n", K, agpl::kernel_product_scale(K), agpl::kernel_product_curvature(K),
           (int)agpl::kernel_has_param(K), (int)(agpl::kernel_param_refused(K, -1.0, 1e300, false) != nullptr),
           (double)agpl::kernel_rule<K, float>(1.0, 0.0), agpl::kernel_drule<K, double>(1.0, 0.0));
}
int main() {
    for (int k = -2; k < 70; ++k)
        printf("kind %d %d %d %d %d %d %d %d\n", k, (int)agpl::kernel_kind_known(k), (int)agpl::kernel_kind_product(k), (int)agpl::kernel_kind_sum(k),
               (int)agpl::kernel_kind_additive(k), (int)agpl::kernel_kind_additive2(k), (int)agpl::kernel_kind_warps(k), (int)agpl::kernel_kind_modulated(k));
    rules<AGPL_KERNEL_MATERN32_PRODUCT>();
    rules<AGPL_KERNEL_MATERN52_PRODUCT>();
    printf("value %.17g %.9g %.17g %.9g\n", agpl::kernel_product_value(2.0, 3.0), (double)agpl::kernel_product_value(2.f, 3.f),
           agpl::kernel_product_value(800.0, (double)INFINITY), (double)agpl::kernel_product_value(90.f, INFINITY));
}
"""


@pytest.fixture(scope="module")
def rows(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("rules_product")
    (tmp / "rules.cpp").write_text(SRC)
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-D__HIP_PLATFORM_AMD__", "-I", os.path.join(ROCM, "include"), "-I", CSRC,
                    str(tmp / "rules.cpp"), "-o", str(tmp / "rules")], check=True)
    return [ln.split() for ln in subprocess.run([str(tmp / "rules")], capture_output=True, text=True, check=True).stdout.splitlines()]


def test_kinds_64_and_66_and_their_predicates(rows):
    kinds = {int(r[1]): tuple(int(v) for v in r[2:]) for r in rows if r[0] == "kind"}
    assert [k for k, v in kinds.items() if v[0]] == [0, 1, 2, 3, 4, 6, 8, 10, 14, 40, 64, 66] and not kinds[65][0] and not kinds[67][0]
    assert [k for k, v in kinds.items() if v[1]] == [64, 66] and kinds[64] == kinds[66] == (1, 1, 0, 0, 0, 0, 0)


def test_polynomials_scale_and_curvature_are_the_closed_forms(rows):
    forms = {64: (np.sqrt(3.0), lambda a: 1 + a, lambda a: -3.0, 3.0), 66: (np.sqrt(5.0), lambda a: 1 + a + a * a / 3, lambda a: -5 / 3 * (1 + a), 5 / 3)}
    got = [r for r in rows if r[0] == "rule"]
    assert len(got) == 8
    for r in got:
        (_, p, t, _), a, v = forms[int(r[1])], float(r[2]), [float(s) for s in r[3:]]
        assert abs(v[0] - p(a)) <= 2 ** -51 * p(a) and abs(v[1] - t(a)) <= 2 ** -51 * abs(t(a)) and v[4:] == v[:2]
        assert abs(v[2] - p(a)) <= 2 ** -22 * p(a) and abs(v[3] - t(a)) <= 2 ** -22 * abs(t(a))
    for r in (r for r in rows if r[0] == "const"):
        c, _, _, c0 = forms[int(r[1])]  # scale, c0 = -t(0); no parameter, none refused; kernel_rule and kernel_drule give 0
        assert float(r[2]) == c and abs(float(r[3]) - c0) <= 2 ** -52 and [float(s) for s in r[4:]] == [0, 0, 0, 0]
    v = [float(s) for s in next(r for r in rows if r[0] == "value")[1:]]
    assert abs(v[0] - 3 * np.exp(-2.0)) <= 1e-15 and abs(v[1] - 3 * np.exp(-2.0)) <= 1e-7 and v[2:] == [0, 0]  # (past the cut: 0, never inf 0)
