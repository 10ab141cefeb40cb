"""The additive squared exponential kind's rules (csrc/agpl_kernel_rules.h), compiled alone for the host with g++ as
tests/test_lik_desc_cpu.py compiles its header: the kind (14; 12 is refused by an existing test) is known, the predicate holds for it
alone, and the per-dimension term and its derivative agree with the float64 closed forms on a grid.  Fails on the parent (no such
enumerator)."""
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "augmentedgplikelihoods.jl_amd", "csrc")
ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")
# the header's device-only neighbours need three names the host compiler lacks; nothing under test uses them
SRC = r"""
#include <cmath>
#define _Float16 short
static inline double sinpi(double v) { return std::sin(M_PI * v); }
static inline double cospi(double v) { return std::cos(M_PI * v); }
#include "agpl_kernel_rules.h"
int main() {
    for (int k = -2; k < 40; ++k) printf("kind %d %d %d %.17g\n", k, (int)agpl::kernel_kind_known(k), (int)agpl::kernel_kind_additive(k), agpl::kernel_term_weight(k, 4));
    for (int i = -60; i <= 60; ++i) {
        const double u = 0.1 * i;
        printf("term %.17g %.17g %.17g %.9g %.9g\n", u, agpl::kernel_term<double>(u), agpl::kernel_dterm<double>(u),
               (double)agpl::kernel_term<float>(u), (double)agpl::kernel_dterm<float>(u));
    }
}
"""


def test_the_kind_is_known_and_its_term_is_the_closed_form(tmp_path):
    (tmp_path / "rules.cpp").write_text(SRC)
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-D__HIP_PLATFORM_AMD__", "-I", os.path.join(ROCM, "include"), "-I", CSRC,
                    str(tmp_path / "rules.cpp"), "-o", str(tmp_path / "rules")], check=True)
    rows = [ln.split() for ln in subprocess.run([str(tmp_path / "rules")], capture_output=True, text=True, check=True).stdout.splitlines()]
    kinds = {int(r[1]): (int(r[2]), int(r[3]), float(r[4])) for r in rows if r[0] == "kind"}
    assert kinds[14] == (1, 1, 0.25) and [k for k, v in kinds.items() if v[1] or v[2] != 1.0] == [14]
    assert [k for k, v in kinds.items() if v[0]] == [0, 1, 2, 3, 4, 6, 8, 10, 14]
    t = np.array([[float(v) for v in r[1:]] for r in rows if r[0] == "term"])
    u, e = t[:, 0], np.exp(-0.5 * t[:, 0] ** 2)
    assert len(u) == 121 and np.abs(t[:, 1] - e).max() <= 4e-16 and np.abs(t[:, 2] + u * e).max() <= 4e-16  # float64: two roundings
    assert np.abs(t[:, 3] - e).max() <= 3 * 2.0 ** -24 and np.abs(t[:, 4] + u * e).max() <= 3 * 2.0 ** -24  # float32: |u e| <= 0.61
