"""The supported domain of agpl_predictive (include/agpl_predictive.h) as a grid of named points per likelihood:
plain numbers, no GPU, no package import.  tests/test_predictive_domain_cpu.py proves the float64 reference and the numpy twin on
every point, tests/test_gpu_predictive_domain.py runs the device on every point.  Accuracy outside this grid's ranges is not promised.

GRID[kind] = list of (name, p, y, mu, var); heteroscedastic: mu = (mu_f, mu_g), var = (var_f, var_g).  The corners of the old test box
(tests/predictive_reference.box_cases: mu = +-4, s in {0.05, 2} at its parameter settings) are on it.  REMOVED names the points that
the reference cannot vouch for (DESIGN.md 4.23 lists them with the reason); nothing is excluded at run time."""
import math

S = (1e-8, 1e-3, 0.05, 2.0, 5.0, 10.0, 20.0, 50.0)
MU = (0.0, 4.0, -4.0, 10.0, -10.0, 40.0, -40.0)
IMAX = 2 ** 31 - 1


def _n(x):
    return f"{x:g}"


def _bernoulli():
    out = []
    for mu in MU + (-300.0,):
        for s in S:
            out.append((f"y1_mu{_n(mu)}_s{_n(s)}", (0.0,), 1, mu, s * s))
    for mu in (0.0, 4.0, -4.0, -40.0):  # (mu = +-4 at s = 0.05, 2: the old box's corners with either label)
        for s in S:
            out.append((f"y0_mu{_n(mu)}_s{_n(s)}", (0.0,), 0, mu, s * s))
    return out


def _negbinomial():
    out = []
    for r in (1.0, 15.0):  # the old box's corners
        for y in (0, 60):
            for mu in (4.0, -4.0):
                for s in (0.05, 2.0):
                    out.append((f"box_r{_n(r)}_y{y}_mu{_n(mu)}_s{_n(s)}", (r,), y, mu, s * s))
    for r in (1e-3, 1.0, 15.0, 1e4):
        for s in S:
            out.append((f"r{_n(r)}_y1_mu0_s{_n(s)}", (r,), 1, 0.0, s * s))
        for mu in (10.0, -10.0, 40.0, -40.0, -300.0):
            out.append((f"r{_n(r)}_y60_mu{_n(mu)}_s2", (r,), 60, mu, 4.0))
        for mu in (40.0, -300.0):
            out.append((f"r{_n(r)}_y60_mu{_n(mu)}_s50", (r,), 60, mu, 2500.0))
        for y in (1000, 100000):
            out.append((f"r{_n(r)}_y{y}_mu-4_s0.05", (r,), y, -4.0, 0.0025))
            out.append((f"r{_n(r)}_y{y}_mu4_s5", (r,), y, 4.0, 25.0))
        out.append((f"r{_n(r)}_ymax_mu10_s5", (r,), IMAX, 10.0, 25.0))
        out.append((f"r{_n(r)}_ymax_mu40_s0.05", (r,), IMAX, 40.0, 0.0025))
    out.append(("r15_y3_mu-1_s50", (15.0,), 3, -1.0, 2500.0))  # the mean overflows: Var y = +inf, not NaN
    return out


def _poisson():
    out = []
    for y in (0, 12):  # the old box's corners (lambda = 3, y <= 12)
        for mu in (4.0, -4.0):
            for s in (0.05, 2.0):
                out.append((f"box_y{y}_mu{_n(mu)}_s{_n(s)}", (3.0,), y, mu, s * s))
    for lam, ys in ((1e-6, (0, 1)), (3.0, (0, 1, 60)), (1e6, (0, 1000, 500000))):
        for y in ys:
            for s in S:
                out.append((f"lam{_n(lam)}_y{y}_mu1_s{_n(s)}", (lam,), y, 1.0, s * s))
        for mu in MU[1:]:
            out.append((f"lam{_n(lam)}_y{ys[-1]}_mu{_n(mu)}_s2", (lam,), ys[-1], mu, 4.0))
            out.append((f"lam{_n(lam)}_y{ys[1]}_mu{_n(mu)}_s20", (lam,), ys[1], mu, 400.0))
    out.append(("lam3_y100000_mu4_s5", (3.0,), 100000, 4.0, 25.0))
    out.append(("lam1e+06_y100000_mu-4_s0.05", (1e6,), 100000, -4.0, 0.0025))
    out.append(("lam1e+06_ymax_mu10_s5", (1e6,), IMAX, 10.0, 25.0))
    return out


def _st_point(tag, nu, sg, k, mu, s):
    # residual of k predictive standard deviations; the Student-t part's scale stands in where its variance is infinite (nu <= 2)
    sd = math.sqrt(s * s + sg * sg * (nu / (nu - 2.0) if nu > 2.0 else 1.0))
    return (f"{tag}nu{_n(nu)}_sg{_n(sg)}_k{k}_mu{_n(mu)}_s{_n(s)}", (nu, sg), mu + k * sd, mu, s * s)


def _studentt():
    out = []
    for nu in (1.5, 3.0, 10.0):  # the old box's corners
        for sg in (0.1, 0.5, 2.0):
            for mu, s, k in ((-4.0, 0.05, 3), (4.0, 2.0, -3), (-4.0, 2.0, 3), (4.0, 0.05, -3)):
                out.append(_st_point("box_", nu, sg, k, mu, s))
    for i, nu in enumerate((0.01, 0.1, 0.5, 1.0, 2.0, 2.5, 10.0, 30.0, 100.0, 300.0, 1e3, 1e4, 1e6)):
        mu = MU[i % len(MU)]
        for k in (0, 3, 50):
            out.append(_st_point("", nu, 0.5, k, mu, 2.0))
        out.append(_st_point("", nu, 0.5, 3, mu, 50.0))
    for sg in (1e-3, 2.0, 1e3):
        for nu in (0.01, 100.0, 1e6):
            out.append(_st_point("", nu, sg, 0, 0.0, 0.05))
            out.append(_st_point("", nu, sg, 50, 10.0, 20.0))
            out.append(_st_point("", nu, sg, 3, -40.0, 1e-8))
    out.append(("issue_nu300", (300.0, 0.5), 0.7, 0.2, 0.3))  # the row the parent's range lost
    return out


def _hetero_point(tag, lam, k, mf, mg, vf, vg):
    sd = math.sqrt(vf + (1.0 + math.exp(-mg)) / lam)  # predictive standard deviation at the mean of g
    return (f"{tag}lam{_n(lam)}_k{k}_mf{_n(mf)}_mg{_n(mg)}_vf{_n(vf)}_vg{_n(vg)}", (lam,), mf + k * sd, (mf, mg), (vf, vg))


def _heterogauss():
    out = []
    for mf in (4.0, -4.0):  # the old box's corners
        for mg in (4.0, -4.0):
            for sf in (0.05, 2.0):
                for sg in (0.05, 2.0):
                    out.append(_hetero_point("box_", 2.0, 3 if mf > 0 else -3, mf, mg, sf * sf, sg * sg))
    for lam, vfs in ((2.0, (0.3,)), (1e-6, (0.0, 0.3)), (1e6, (1e-6, 0.3))):
        for i, vg in enumerate((0.0, 0.01, 4.0, 25.0, 100.0)):
            for j, mg in enumerate((-30.0, -1.0, 5.0, 30.0)):
                out.append(_hetero_point("", lam, (0, 3, -3)[(i + j) % 3], 0.2, mg, vfs[(i + j) % len(vfs)], vg))
    for vf in (0.0, 1e-6):
        for vg in (0.0, 100.0):
            for mg in (-1.0, 30.0):
                out.append(_hetero_point("", 2.0, 3, -10.0, mg, vf, vg))
    for vg in (25.0, 100.0):
        out.append((f"issue_vg{_n(vg)}", (2.0,), 1.0, (0.2, -1.0), (0.3, vg)))
    out.append(("y30_mg-30", (2.0,), 30.0, (0.0, -30.0), (0.3, 4.0)))
    return out


def _laplace():
    out = []
    for beta in (0.1, 1.0):  # the old box's corners
        for mu, s, k in ((-4.0, 0.05, 3), (4.0, 2.0, -3), (-4.0, 2.0, 3), (4.0, 0.05, -3)):
            out.append((f"box_b{_n(beta)}_mu{_n(mu)}_s{_n(s)}", (beta,), mu + k * math.sqrt(s * s + 2.0 * beta * beta), mu, s * s))
    for beta in (1e-3, 0.1, 1.0, 10.0):
        for var in (1e-10, 0.0025, 4.0, 400.0):
            d0 = var / beta  # z1 = 0 at d = d0, z2 = 0 at d = -d0
            for tag, d in (("d0", 0.0), ("z1+", 0.99 * d0), ("z1-", 1.01 * d0), ("z2+", -0.99 * d0), ("z2-", -1.01 * d0),
                           ("far+", 3000.0 * beta), ("far-", -3000.0 * beta)):
                out.append((f"b{_n(beta)}_v{_n(var)}_{tag}", (beta,), 1.0 + d, 1.0, var))
    return out


GRID = {"bernoulli": _bernoulli(), "negbinomial": _negbinomial(), "studentt": _studentt(), "poisson": _poisson(),
        "laplace": _laplace(), "heterogauss": _heterogauss()}

# points the float64 reference cannot vouch for (kind -> names), at most 2 % per kind
REMOVED = {k: () for k in GRID}
REMOVED["laplace"] = ("b0.001_v400_z1+", "b0.001_v400_z2+")  # quad's error estimate is 6.2e-9 at both (|log p| = 2e8)


def points(kind):
    return [pt for pt in GRID[kind] if pt[0] not in REMOVED[kind]]


def groups(kind):
    """The kind's points by parameter set: [(p, [points])], one device launch each."""
    out = {}
    for pt in points(kind):
        out.setdefault(pt[1], []).append(pt)
    return list(out.items())
