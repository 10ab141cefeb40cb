"""The supported domain of agpl_expected_loglik (include/agpl_likgrad.h) as a grid of named points per
likelihood: plain numbers, no GPU, no package import.  Every point of predictive_domain.GRID (GRID, not points(): the two Laplace
points removed there were removed for a reason of that reference) with the same (name, p, y, mu, var) tuples, plus what this kernel
in particular can get wrong: the Student-t rule above s / a = 64 (a = sigma sqrt(nu)) and at that seam, the variance edges of every
kind, and the Poisson derivative where it is a difference of two numbers of 5e5.  tests/test_likgrad_domain_cpu.py proves the
reference and the numpy twin on every point, tests/test_gpu_likgrad_domain.py runs the device on every point.  Accuracy outside this
grid's ranges is not promised.  REMOVED names the points the reference cannot vouch for; nothing is excluded at run time."""
import math

import predictive_domain as PD

KINDS = ("bernoulli", "negbinomial", "studentt", "poisson", "laplace", "heterogauss")


def _n(x):
    return f"{x:g}"


# E sigma(f) under N(1, 0.05^2), from the reference (likgrad_domain_reference.logistic_expectations(1.0, 0.0025)[2]; the CPU test holds
# the number to it): the Poisson point with y within 1 of lambda E sigma(f) at lambda = 1e6 is stated as a plain number
E_SIGMA_MU1_S005 = 0.7309451028429497


def st_point(tag, nu, sg, k, mu, s):
    """A Student-t point at a residual of k predictive standard deviations (the scale stands in where the variance is infinite),
    named as predictive_domain names its own."""
    sd = math.sqrt(s * s + sg * sg * (nu / (nu - 2.0) if nu > 2.0 else 1.0))
    return (f"{tag}nu{_n(nu)}_sg{_n(sg)}_k{k}_mu{_n(mu)}_s{_n(s)}", (nu, sg), mu + k * sd, mu, s * s)


_st = st_point


def _studentt_extra():
    out = []
    for nu in (0.01, 1.0, 100.0):  # s / a from 0.5 (the kept rule) to 2e5
        for s in (0.05, 2.0, 20.0):
            for k in (0, 1, 3, 50):
                out.append(_st("wide_", nu, 1e-3, k, 10.0 if s == 20.0 else 0.0, s))
    for nu in (0.01, 0.1):
        for k in (0, 1, 3, 50):
            out.append(_st("wide_", nu, 0.5, k, 0.0, 50.0))
    a = 0.05 * math.sqrt(3.0)
    for ratio in (63.9, 64.0, 64.1):  # the seam between the trapezoid rule in f and the sinh rule
        for k in (0, 1):
            name, p, y, mu, var = _st("seam_", 3.0, 0.05, k, 0.0, ratio * a)
            out.append((f"seam{_n(ratio)}_k{k}", p, y, mu, var))
    for var in (0.0, 1e-320, 1e-30):
        out.append((f"edge_var{_n(var)}", (3.0, 0.5), 0.7, 0.2, var))
    return out


def _edges(kind):
    out = []
    for var in (0.0, 1e-320, 1e-30):
        if kind == "bernoulli":
            out.append((f"edge_var{_n(var)}", (0.0,), 1, 0.3, var))
        elif kind == "negbinomial":
            out.append((f"edge_var{_n(var)}", (15.0,), 7, 0.3, var))
        elif kind == "poisson":
            out.append((f"edge_var{_n(var)}", (3.0,), 2, 0.3, var))
        elif kind == "laplace":
            out.append((f"edge_var{_n(var)}", (0.5,), 0.7, 0.2, var))
        elif kind == "heterogauss":  # in either latent alone
            out.append((f"edge_varf{_n(var)}", (2.0,), 0.7, (0.2, -1.0), (var, 0.3)))
            out.append((f"edge_varg{_n(var)}", (2.0,), 0.7, (0.2, -1.0), (0.3, var)))
    return out


def _poisson_extra():
    y = int(round(1e6 * E_SIGMA_MU1_S005))
    return [("lam1e+06_ynear_mu1_s0.05", (1e6,), y, 1.0, 0.0025)]


GRID = {k: list(PD.GRID[k]) for k in KINDS}
GRID["studentt"] += _studentt_extra()
GRID["poisson"] += _poisson_extra()
for _k in KINDS:
    if _k != "studentt":
        GRID[_k] += _edges(_k)

# points the reference cannot vouch for (kind -> names), at most 2 % per kind
REMOVED = {k: () for k in KINDS}


def points(kind):
    return [pt for pt in GRID[kind] if pt[0] not in REMOVED[kind]]


def groups(kind):
    """The kind's points by parameter set: [(p, [points])], one device launch each."""
    out = {}
    for pt in points(kind):
        out.setdefault(pt[1], []).append(pt)
    return list(out.items())
