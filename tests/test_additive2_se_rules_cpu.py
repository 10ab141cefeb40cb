"""The second-order additive squared exponential kind's rules (csrc/agpl_kernel_rules.h), compiled alone for the host with g++ as
tests/test_additive_se_rules_cpu.py compiles them: the kind (40: that test holds that nothing between 15 and 39 is a kind) is known,
its predicate holds for it alone over -2 ... 63, the two mixing weights w / D and (1 - w) / P and the prior-variance factor (2 - w) / D
are the closed forms (at D = 1 there is no pair and w is ignored: 1, 0 and 1), and the parameter check refuses what is not in (0, 1].
Fails on the parent (no such enumerator)."""
import os
import subprocess

import pytest

from test_additive_se_rules_cpu import CSRC, ROCM

SRC = r"""
#include <cmath>
#include <limits>
#define _Float16 short
static inline double sinpi(double v) { return std::sin(M_PI * v); }
static inline double cospi(double v) { return std::cos(M_PI * v); }
#include "agpl_kernel_rules.h"
int main() {
    const int K = AGPL_KERNEL_ADDITIVE2_SE;
    for (int k = -2; k < 64; ++k)
        printf("kind %d %d %d %d %d\n", k, (int)agpl::kernel_kind_known(k), (int)agpl::kernel_kind_additive2(k), (int)agpl::kernel_kind_additive(k), (int)agpl::kernel_kind_sum(k));
    for (int D : {1, 2, 4})
        for (double w : {0.25, 1.0})
            printf("weights %d %.17g %.17g %.17g %.17g\n", D, w, agpl::kernel_sum_weight1(K, D, w), agpl::kernel_sum_weight2(K, D, w), agpl::kernel_sum_curvature(K, D, w));
    const double inf = std::numeric_limits<double>::infinity();
    for (double w : {0.0, -1.0, 1.5, std::nan(""), inf, 1.0, 0.25})
        printf("param %.17g %d\n", w, (int)(agpl::kernel_param_refused(K, w, 1e300, false) != nullptr));
    float S1 = 0.f, E2 = 0.f;  // the recurrence on e = 1, 2, 3: S1 = 6, E2 = 1 2 + 1 3 + 2 3 = 11
    for (float e : {1.f, 2.f, 3.f}) agpl::kernel_sum_step(e, S1, E2);
    printf("step %.9g %.9g %d %d\n", S1, E2, (int)agpl::kernel_has_param(K), K);
}
"""


@pytest.fixture(scope="module")
def rows(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("rules2")
    (tmp / "rules.cpp").write_text(SRC)
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-D__HIP_PLATFORM_AMD__", "-I", os.path.join(ROCM, "include"), "-I", CSRC,
                    str(tmp / "rules.cpp"), "-o", str(tmp / "rules")], check=True)
    return [ln.split() for ln in subprocess.run([str(tmp / "rules")], capture_output=True, text=True, check=True).stdout.splitlines()]


def test_the_kind_is_40_and_the_predicate_is_its_alone(rows):
    kinds = {int(r[1]): tuple(int(v) for v in r[2:]) for r in rows if r[0] == "kind"}
    assert sorted(kinds) == list(range(-2, 64)) and kinds[40] == (1, 1, 0, 1) and kinds[14] == (1, 0, 1, 1)
    assert [k for k, v in kinds.items() if v[1]] == [40] and [k for k, v in kinds.items() if v[3]] == [14, 40]
    assert [k for k, v in kinds.items() if v[0]] == [0, 1, 2, 3, 4, 6, 8, 10, 14, 40]
    assert [r for r in rows if r[0] == "step"] == [["step", "6", "11", "1", "40"]]


def test_weights_curvature_and_parameter_check(rows):
    got = {(int(r[1]), float(r[2])): tuple(float(v) for v in r[3:]) for r in rows if r[0] == "weights"}
    for (D, w), (w1, w2, c) in got.items():
        we = w if D > 1 else 1.0  # (no pair at D = 1: the squared exponential)
        want = (we / D, (1 - we) / (D * (D - 1) / 2) if D > 1 else 0.0, (2 - we) / D)
        assert max(abs(a - b) for a, b in zip((w1, w2, c), want)) <= 2.0 ** -52, (D, w, w1, w2, c)
        assert abs(D * w1 + (D * (D - 1) / 2) * w2 - 1) <= 2.0 ** -51  # k(x, x) = variance
    assert len(got) == 6 and got[(4, 1.0)] == (0.25, 0.0, 0.25)  # w = 1: the additive kind's 1 / D
    assert [(r[1], int(r[2])) for r in rows if r[0] == "param"] == [("0", 1), ("-1", 1), ("1.5", 1), ("nan", 1), ("inf", 1), ("1", 0), ("0.25", 0)]
