"""The reference of the expected log-likelihood tests (tests/likgrad_reference.py) checked on its own, CPU-only: its analytic
derivatives against central differences of its values, quad's error estimates over the whole case box, the two closed forms the
device uses against quad, and the device's digamma (csrc/agpl_digamma.h, its host instantiation in a stand-alone C++ program)
against scipy.special.digamma."""
import math
import os
import shutil
import subprocess

import numpy as np
import pytest
from scipy import special

import likgrad_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "augmentedgplikelihoods.jl_amd", "csrc")


@pytest.mark.parametrize("kind", [k for k in R.KINDS if R.NPARAMS[k]])
def test_analytic_derivatives_equal_central_differences(kind):
    """h = 1e-4 in each log-parameter.  The bar has three parts: the truncation term h^2 |f'''| / 6 of the central difference --
    the third derivatives of these log densities in a log-parameter are sums of the terms of ell and dell themselves times small
    integers (e.g. Laplace: f''' = E|y - f| / beta), bounded here by 10 max(1, |ell|, |dell|), so 10 h^2 / 6 of that scale --, quad's
    own error estimates of the two values divided by 2 h, and of the derivative; and the rounding of the two values, 4 ulp of |ell|
    each, divided by 2 h."""
    h = 1e-4
    worst = 0.0
    for p, y, mu, var in R.cases(kind, R.SEED + R.KINDS.index(kind)):
        for i in range(0, len(y), 8):  # every eighth case of every group: 64 per kind
            ell, _ = R.ref_ell(kind, p, y[i], mu[i], var[i])
            dell, derr = R.ref_dell(kind, p, y[i], mu[i], var[i])
            for k in range(R.NPARAMS[kind]):
                pp, pm = list(p), list(p)
                pp[k], pm[k] = p[k] * math.exp(h), p[k] * math.exp(-h)
                (fp, ep), (fm, em) = R.ref_ell(kind, pp, y[i], mu[i], var[i]), R.ref_ell(kind, pm, y[i], mu[i], var[i])
                fd = (fp - fm) / (2.0 * h)
                scale = max(1.0, abs(ell), abs(dell[k]))
                bar = 10.0 * h * h / 6.0 * scale + (ep + em) / (2.0 * h) + derr[k] + 8.0 * np.finfo(float).eps * abs(ell) / (2.0 * h)
                worst = max(worst, abs(fd - dell[k]) / bar)
                assert abs(fd - dell[k]) <= bar, (kind, p, i, k, fd, dell[k], bar)
    print(f"{kind}: worst |central difference - analytic| in units of its bar {worst:.3e}")


@pytest.mark.parametrize("kind", R.KINDS)
def test_every_case_of_the_box_meets_quads_error_estimate(kind):
    n = 0
    for p, y, mu, var, ell, dell, eerr, derr in R.box(kind):
        assert np.isfinite(ell).all() and np.isfinite(dell).all()
        assert (eerr <= 1e-10 * np.maximum(1.0, np.abs(ell))).all(), (kind, p, eerr.max())
        assert (derr <= 1e-10 * np.maximum(1.0, np.abs(dell))).all(), (kind, p, derr.max())
        s = np.sqrt(var)
        assert (np.abs(mu) <= 8.0).all() and (s >= 1e-3 * (1 - 1e-12)).all() and (s <= 6.0 * (1 + 1e-12)).all()
        if kind == "studentt":
            assert (s / (p[1] * math.sqrt(p[0])) <= 50.0 * (1 + 1e-12)).all()
        n += len(y)
    assert n == R.NCASES == 512 and len(R.box(kind)) == R.NGROUPS


def test_closed_forms_against_quad():
    rng = np.random.default_rng(7)
    for _ in range(32):
        mu, s, beta = rng.uniform(-8, 8), float(np.exp(rng.uniform(np.log(1e-3), np.log(6.0)))), float(np.exp(rng.uniform(-3, 1.6)))
        y = mu + 3.0 * rng.standard_normal() * math.sqrt(s * s + 2 * beta * beta)
        ea, err = R.gauss_expect(lambda f: abs(y - f), mu, s * s, split=(y,))
        assert abs(R.laplace_closed(beta, y, mu, s * s) - ea) <= err + 1e-13 * max(1.0, ea)
        e2, err = R.gauss_expect(lambda f: (y - f) ** 2, mu, s * s, split=(y,))
        assert abs((y - mu) ** 2 + s * s - e2) <= err + 1e-13 * max(1.0, e2)
        # and through the reference itself: ell of the Laplace likelihood from the closed form
        ell, err = R.ref_ell("laplace", (beta,), y, mu, s * s)
        assert abs(-R.laplace_closed(beta, y, mu, s * s) / beta - math.log(2 * beta) - ell) <= err + 1e-13 * max(1.0, abs(ell))


@pytest.mark.parametrize("kind,p", [("studentt", (4.0, 1.0)), ("laplace", (0.7,)), ("negbinomial", (5.0,)), ("poisson", (3.0,)),
                                    ("bernoulli", (0.0,))])
def test_the_many_point_sums_equal_the_per_point_functions(kind, p):
    """ref_sums (quad_vec on all points at once; the Laplace closed form) against the sum of ref_ell / ref_dell, on marginals like
    a fit's (s in [0.05, 1]): 1e-11 of max(1, |sum|) plus both error estimates."""
    rng = np.random.default_rng(11)
    n = 48
    mu, s = rng.uniform(-3, 3, n), np.exp(rng.uniform(np.log(0.05), 0.0, n))
    y = mu + rng.standard_normal(n) if kind in ("studentt", "laplace") else rng.integers(0, 2 if kind == "bernoulli" else 9, n)
    ell, dell, eerr, derr = R.reference(kind, p, y, mu, s * s)
    tot, grad, err = R.ref_sums(kind, p, y, mu, s * s)
    assert abs(tot - ell.sum()) <= 1e-11 * max(1.0, abs(ell.sum())) + eerr.sum() + err
    for k in range(R.NPARAMS[kind]):
        assert abs(grad[k] - dell[:, k].sum()) <= 1e-11 * max(1.0, abs(dell[:, k].sum())) + derr[:, k].sum() + err


DIGAMMA_TU = r"""
#include <stdio.h>
#include <stdlib.h>
#include "agpl_digamma.h"
int main(int argc, char **argv) {
    for (int i = 1; i < argc; ++i) printf("%.17g\n", agpl::digamma(strtod(argv[i], 0)));
    return 0;
}
"""


def test_header_digamma_against_scipy(tmp_path):
    cxx = next((c for c in ("g++", "c++", "clang++") if shutil.which(c)), None)
    assert cxx, "no host C++ compiler"
    src = tmp_path / "digamma.cpp"
    src.write_text(DIGAMMA_TU)
    exe = tmp_path / "digamma"
    subprocess.check_call([cxx, "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-Wextra", "-Werror", "-I", CSRC, str(src), "-o", str(exe)])
    xs = [1e-3, 0.5, 1.0, 5.999, 6.0, 6.001, 1e3, 1e8]
    out = subprocess.check_output([str(exe)] + [repr(x) for x in xs]).decode().split()
    got, ref = np.array([float(v) for v in out]), special.digamma(np.array(xs))
    rel = np.abs(got - ref) / np.abs(ref)
    print("digamma: relative errors", rel)
    assert (rel <= 1e-14).all(), (got, ref)
    # outside the domain
    assert math.isnan(float(subprocess.check_output([str(exe), "0", "-1.5"]).decode().split()[0]))
