"""The squared exponential x categorical kind's rules (csrc/agpl_kernel_rules.h), compiled alone for the host with g++ as
tests/test_anova_se_rules_cpu.py compiles them: 96 is known beside the fifteen older kinds and nothing else in -2 ... 127 is, the new
predicate is its alone and every older predicate is false for it, the last C dimensions and no other are categorical, and C is an
integer in 1 ... 16.  Fails on the parent (no such enumerator)."""
import math
import os
import subprocess

import pytest

from test_additive_se_rules_cpu import CSRC, ROCM

SRC = r"""
#include <cmath>
#define _Float16 short
static inline double sinpi(double v) { return std::sin(M_PI * v); }
static inline double cospi(double v) { return std::cos(M_PI * v); }
#include "agpl_kernel_rules.h"
int main() {
    const int K = AGPL_KERNEL_SE_CATEGORICAL;
    for (int k = -2; k < 128; ++k)
        printf("kind %d %d %d %d %d %d %d %d %d %d %d\n", k, (int)agpl::kernel_kind_known(k), (int)agpl::kernel_kind_categorical(k), (int)agpl::kernel_kind_anova(k),
               (int)agpl::kernel_kind_se_matern(k), (int)agpl::kernel_kind_product(k), (int)agpl::kernel_kind_sum(k), (int)agpl::kernel_kind_additive(k),
               (int)agpl::kernel_kind_additive2(k), (int)agpl::kernel_kind_warps(k), (int)agpl::kernel_kind_modulated(k));
    const int dc[3][2] = {{1, 1}, {4, 2}, {16, 16}};
    for (auto &c : dc)
        for (int d = 0; d < c[0]; ++d)
            printf("dim %d %d %d %d %d\n", c[0], c[1], d, (int)agpl::kernel_dim_categorical(K, d, c[0], c[1]), (int)agpl::kernel_dim_categorical(AGPL_KERNEL_SE, d, c[0], c[1]));
    printf("const %d %.17g %.17g %.17g %.17g %.17g %d %d", (int)agpl::kernel_has_param(K), agpl::kernel_rule<K, double>(1.0, 2.0), agpl::kernel_drule<K, double>(1.0, 2.0),
           agpl::kernel_categorical_warp(0.0, 4.0), agpl::kernel_categorical_warp(-3.0, 4.0), agpl::kernel_categorical_half(0.5),
           (int)agpl::kernel_categorical_exceeds(K, 3.0, 2), (int)agpl::kernel_categorical_exceeds(K, 2.0, 2));
    for (double C : {0.0, -1.0, 1.5, 17.0, (double)NAN, 1.0, 16.0}) printf(" %d", (int)(agpl::kernel_param_refused(K, C, 1e300, false) != nullptr));
    printf("\n");
}
"""


@pytest.fixture(scope="module")
def rows(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("rules_se_categorical")
    (tmp / "rules.cpp").write_text(SRC)
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-D__HIP_PLATFORM_AMD__", "-I", os.path.join(ROCM, "include"), "-I", CSRC,
                    str(tmp / "rules.cpp"), "-o", str(tmp / "rules")], check=True)
    return [ln.split() for ln in subprocess.run([str(tmp / "rules")], capture_output=True, text=True, check=True).stdout.splitlines()]


def test_kind_96_its_predicates_and_its_parameter(rows):
    kinds = {int(r[1]): tuple(int(v) for v in r[2:]) for r in rows if r[0] == "kind"}
    assert len(kinds) == 130 and [k for k, v in kinds.items() if v[0]] == [0, 1, 2, 3, 4, 6, 8, 10, 14, 40, 64, 66, 70, 72, 80, 96]
    assert [k for k, v in kinds.items() if v[1]] == [96] and kinds[96] == (1, 1, 0, 0, 0, 0, 0, 0, 0, 0)
    dims = [[int(v) for v in r[1:]] for r in rows if r[0] == "dim"]
    assert len(dims) == 21 and all(cat == (d >= D - C) and other == 0 for D, C, d, cat, other in dims)
    c = [r for r in rows if r[0] == "const"][0]  # a parameter; the squared exponential's rule on r^2; [us != 0] / ell; 1 / (2 ell^2); C > D
    assert abs(float(c[2]) - math.exp(-0.5)) <= 2 ** -53 and float(c[3]) == -float(c[2]) and [float(v) for v in c[1:2] + c[4:9]] == [1, 0, 4, 2, 1, 0]
    assert [int(v) for v in c[9:]] == [1, 1, 1, 1, 1, 0, 0]  # C = 0, -1, 1.5, 17, NaN are refused; 1 and 16 are not


def test_python_names_and_refusals():
    from agpl_amd import _ffi, sparse

    assert sparse.kernel_kind(("se_categorical", 2)) == (96, 2.0) and _ffi.KERNEL_SE_CATEGORICAL == 96
    assert sparse.kernel_kind_categorical(96) and not any(sparse.kernel_kind_categorical(k) for k in (0, 8, 72, 80, 95, 97))
    assert [sparse.kernel_dim_categorical(96, d, 4, 2.0) for d in range(4)] == [False, False, True, True]
    with pytest.raises(_ffi.ArgumentError, match="kernel must be"):
        sparse.kernel_kind("se_categorical")
    for bad in (2.5, 0, 17, float("nan")):
        with pytest.raises(_ffi.ArgumentError, match="the number C of trailing categorical inputs"):
            sparse.kernel_kind(("se_categorical", bad))
    with pytest.raises(_ffi.AGPLError, match="select_inducing_greedy") as e:
        sparse.select_inducing(None, 4, kernel=("se_categorical", 1))
    assert e.value.code == _ffi.ERR_UNSUPPORTED
