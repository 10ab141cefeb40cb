"""The all-orders additive (ANOVA) squared exponential kind's rules (csrc/agpl_kernel_rules.h), compiled alone for the host with g++ as
tests/test_se_matern_rules_cpu.py compiles them: 80 is known beside the fourteen older kinds and nothing else in -2 ... 95 is, the new
predicate is its alone and every older predicate is false for it, it carries a parameter in (0, 1], and the factor, its derivative
and the curvature are the closed forms.  Fails on the parent (no such enumerator)."""
import os
import subprocess

import numpy as np
import pytest

from test_additive_se_rules_cpu import CSRC, ROCM

ETA, US = 0.3, (0.0, 0.5, 3.0, 40.0)
SRC = r"""
#include <cmath>
#define _Float16 short
static inline double sinpi(double v) { return std::sin(M_PI * v); }
static inline double cospi(double v) { return std::cos(M_PI * v); }
#include "agpl_kernel_rules.h"
int main() {
    const int K = AGPL_KERNEL_ANOVA_SE;
    for (int k = -2; k < 96; ++k)
        printf("kind %d %d %d %d %d %d %d %d %d %d\n", k, (int)agpl::kernel_kind_known(k), (int)agpl::kernel_kind_anova(k), (int)agpl::kernel_kind_se_matern(k),
               (int)agpl::kernel_kind_product(k), (int)agpl::kernel_kind_sum(k), (int)agpl::kernel_kind_additive(k), (int)agpl::kernel_kind_additive2(k),
               (int)agpl::kernel_kind_warps(k), (int)agpl::kernel_kind_modulated(k));
    for (double eta : {0.3, 1.0})
        for (double u : {0.0, 0.5, 3.0, 40.0})
            printf("rule %.17g %.17g %.17g %.17g %.9g %.9g %.17g %.9g\n", eta, u, agpl::kernel_anova_factor<double>(eta, u), agpl::kernel_anova_dfactor<double>(eta, u),
                   (double)agpl::kernel_anova_factor<float>((float)eta, u), (double)agpl::kernel_anova_dfactor<float>((float)eta, u),
                   agpl::kernel_anova_factor<double>(eta, -u), (double)agpl::kernel_anova_factor<float>((float)eta, -u));
    printf("const %d %.17g %.17g %.9g %.17g", (int)agpl::kernel_has_param(K), agpl::kernel_anova_curvature(K, 0.3), agpl::kernel_anova_curvature(AGPL_KERNEL_SE, 0.3),
           (double)agpl::kernel_rule<K, float>(1.0, 0.3), agpl::kernel_drule<K, double>(1.0, 0.3));
    for (double eta : {0.0, -1.0, 1.5, (double)NAN, 1e-3, 1.0}) printf(" %d", (int)(agpl::kernel_param_refused(K, eta, 1e300, false) != nullptr));
    printf(" %s\n", agpl::kernel_param_range(K));
}
"""


@pytest.fixture(scope="module")
def rows(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("rules_anova_se")
    (tmp / "rules.cpp").write_text(SRC)
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-D__HIP_PLATFORM_AMD__", "-I", os.path.join(ROCM, "include"), "-I", CSRC,
                    str(tmp / "rules.cpp"), "-o", str(tmp / "rules")], check=True)
    return [ln.split() for ln in subprocess.run([str(tmp / "rules")], capture_output=True, text=True, check=True).stdout.splitlines()]


def test_kind_80_and_its_predicates(rows):
    kinds = {int(r[1]): tuple(int(v) for v in r[2:]) for r in rows if r[0] == "kind"}
    assert len(kinds) == 98 and [k for k, v in kinds.items() if v[0]] == [0, 1, 2, 3, 4, 6, 8, 10, 14, 40, 64, 66, 70, 72, 80]
    assert [k for k, v in kinds.items() if v[1]] == [80] and kinds[80] == (1, 1, 0, 0, 0, 0, 0, 0, 0)
    c = [r for r in rows if r[0] == "const"][0]  # a parameter; curvature eta (1 for another kind); kernel_rule and kernel_drule give 0
    assert [float(v) for v in c[1:6]] == [1, 0.3, 1.0, 0, 0]
    assert [int(v) for v in c[6:12]] == [1, 1, 1, 1, 0, 0] and " ".join(c[12:]) == "positive and at most 1"  # eta = 0, -1, 1.5, NaN; 1e-3, 1


def test_factor_and_derivative_are_the_closed_forms(rows):
    got = [[float(s) for s in r[1:]] for r in rows if r[0] == "rule"]
    assert [(v[0], v[1]) for v in got] == [(eta, u) for eta in (ETA, 1.0) for u in US]
    for eta, u, g, dg, g32, dg32, gm, gm32 in got:  # g in [1 - eta, 1] and |dg| <= eta / sqrt(e): absolute bars
        e = np.exp(-0.5 * u * u)
        assert abs(g - (1 - eta * (1 - e))) <= 2 ** -51 and abs(dg + eta * u * e) <= 2 ** -51 and gm == g
        assert abs(g32 - (1 - eta * (1 - e))) <= 2 ** -22 and abs(dg32 + eta * u * e) <= 2 ** -22 and gm32 == g32
        assert u != 0.0 or (g == 1.0 and g32 == 1.0 and dg == 0.0 and dg32 == 0.0)  # k(x, x) = variance to the bit


def test_python_names_and_refusals():
    from agpl_amd import _ffi, sparse

    assert sparse.kernel_kind(("anova_se", 0.3)) == (80, 0.3) and _ffi.KERNEL_ANOVA_SE == 80
    assert sparse.kernel_kind_anova(80) and not any(sparse.kernel_kind_anova(k) for k in (0, 14, 40, 64, 72, 79, 81))
    with pytest.raises(_ffi.ArgumentError, match="kernel must be"):
        sparse.kernel_kind("anova_se")
    for bad in (1.5, 0.0, float("nan")):
        with pytest.raises(_ffi.ArgumentError, match="eta of the all-orders"):
            sparse.kernel_kind(("anova_se", bad))
    with pytest.raises(_ffi.ArgumentError, match="positive and at most 1"):
        sparse.kernel_kind(("anova_se", 1.5))
    with pytest.raises(_ffi.AGPLError, match="select_inducing_greedy") as e:
        sparse.select_inducing(None, 4, kernel=("anova_se", 0.3))
    assert e.value.code == _ffi.ERR_UNSUPPORTED
