"""GPU tests of how the sparse drivers are constructed and how they prepare new inputs (agpl_amd/sparse.py):

* the two routes into a ``Plan``, a ``SparseCAVI`` and a ``SparseGibbs`` (features; raw inputs) give objects with the same
  attributes, and no public method reaches for one that a route lacks;
* each route, taken twice, gives the same numbers bit for bit (the two routes differ from each other in the last bits: features
  decoded from a plan's image are rounded again when another plan splits them);
* objects built from features refuse every method that needs new inputs, by that method's name;
* every method that takes new inputs refuses a wrong D and a wrong-sized prior mean, and takes 1-D inputs on a D = 1 plan.

No kernel depends on the size here: N = 300 (three 128-point tiles, the last partly filled), M = 40 (padded to 256), D = 2; a
Bernoulli likelihood and, for L > 1, a 3-class categorical one (CAVI and plans; the Gibbs cases are Bernoulli).
"""
import re

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

N, M, D, NS, JITTER = 300, 40, 2, 5, 1e-6
ELL = (1.0, 1.4)
KINDS = ("bernoulli", "categorical")
# The project's bar for natural parameters on the split-float16 path (NAT_TOL of tests/test_gpu_plan_inputs.py).  The
# routes differ by one more rounding of the features: decoded from hi + lo float16 (22 bits) to float32 and split again, an
# error of at most 2^-22 of the largest feature per entry, about 2.4e-7 -- forty times below the bar.
NAT_TOL = 1e-5


@pytest.fixture(scope="module")
def A():
    import agpl_amd

    return agpl_amd


@pytest.fixture(scope="module")
def world(A):
    """The inputs, and per likelihood kind ``(lik, y, cavi)``: a ``from_inputs`` SparseCAVI after three sweeps, made once."""
    rng = np.random.default_rng(11)
    x = torch.from_numpy(rng.uniform(-3, 3, size=(N, D))).cuda()
    z = torch.from_numpy(rng.uniform(-3, 3, size=(M, D))).cuda()
    x_s = torch.from_numpy(rng.uniform(-3, 3, size=(NS, D))).cuda()
    f = torch.sin(x[:, 0]) + 0.5 * torch.cos(x[:, 1])
    noise = torch.from_numpy(rng.normal(size=(3, N))).cuda()
    cls = torch.argmax(torch.stack([f, -f, torch.cos(x[:, 0])]) + 0.5 * noise, dim=0)
    ctx = A.Context(0, seed=5)
    made = {}
    for kind in KINDS:
        if kind == "bernoulli":
            lik, y = A.BernoulliLikelihood(), (f + 0.5 * noise[0] > 0).to(torch.uint8)
        else:
            lik, y = A.CategoricalLikelihood(3), torch.nn.functional.one_hot(cls, 3).to(torch.uint8).contiguous()
        cavi = A.SparseCAVI.from_inputs(lik, x, y, z, ELL, jitter=JITTER, ctx=ctx)
        cavi.run(3)
        made[kind] = (lik, y, cavi)
    return ctx, x, z, x_s, made


def from_features(A, cls, lik, plan, y, ctx, **kw):
    """The object of class ``cls`` through ``__init__``, on the features and the residual that ``plan`` holds."""
    return cls(lik, plan.features(), plan.resid.clone(), y, ctx=ctx, **kw)


def state_differences(a, b):
    """The fields of ``Plan.state()`` in which two plans differ in any bit, each with the number of differing elements and the first
    one's flat index; [] if none.  Every field is compared whole, at the padded size -- v, the float16 images U_hi / U_lo, v32,
    logdet -- but for ``U_colmajor``, of which the factor's triangle (padding included) is compared: column-major lower, the upper
    triangle of the row-major view.  Its other triangle is not part of the state: a plan made from inputs never writes it
    (agpl_gaussian_factor, which whitens K_ZZ in that array, and agpl_plan_update both leave "the other triangle of A" untouched,
    csrc/agpl_factor.hip; only agpl_plan_create's identity fills it), so it holds what the memory block held before, and no
    pass reads it (pack_factor_split_kernel, joint_w_kernel and plan_kl_part_kernel stop at the diagonal).  Two builds of one
    model differed there, and nowhere else."""
    sa, sb = a.state(), b.state()
    assert sa.keys() == sb.keys() == set(a._STATE)
    sa["U_colmajor"], sb["U_colmajor"] = torch.triu(sa["U_colmajor"]), torch.triu(sb["U_colmajor"])
    bits = {2: torch.int16, 4: torch.int32, 8: torch.int64}
    out = []
    for k in sa:
        ne = (sa[k].view(bits[sa[k].element_size()]) != sb[k].view(bits[sb[k].element_size()])).reshape(-1)
        if bool(ne.any()):
            out.append(f"{k} {tuple(sa[k].shape)}: {int(ne.sum())} differ, first at {int(ne.nonzero()[0])}")
    return out


@pytest.mark.parametrize("kind", KINDS)
def test_constructors_agree_on_attributes(A, world, kind):
    ctx, x, z, _, made = world
    lik, y, cavi = made[kind]
    p_in = cavi.plan
    p_f = A.Plan(p_in.features(), p_in.resid.clone(), p_in.L, ctx)
    assert vars(p_f).keys() == vars(p_in).keys()
    assert not p_f.se and (p_f.D, p_f.variance, p_f.kernel, p_f.kernel_param) == (None,) * 4
    assert p_in.se and (p_in.D, p_in.variance, p_in.kernel, p_in.kernel_param) == (D, 1.0, "se", 0.0)
    for kw in ({}, {"keep_points": True, "track_elbo": True}):
        a = from_features(A, A.SparseCAVI, lik, p_in, y, ctx, **kw)
        b = A.SparseCAVI.from_inputs(lik, x, y, z, ELL, jitter=JITTER, ctx=ctx, **kw)
        assert vars(a).keys() == vars(b).keys()
        assert a.x is None and b.x is None and a._sites_of is None and b._sites_of is None
    if kind == "bernoulli":
        for kw in ({}, {"keep_points": True}):
            a = from_features(A, A.SparseGibbs, lik, p_in, y, ctx, **kw)
            b = A.SparseGibbs.from_inputs(lik, x, y, z, ELL, jitter=JITTER, ctx=ctx, **kw)
            assert vars(a).keys() == vars(b).keys()


@pytest.mark.parametrize("kind", KINDS)
def test_no_method_needs_an_attribute_a_route_lacks(A, world, kind):
    ctx, x, z, _, made = world
    lik, y, cavi = made[kind]
    fresh = A.SparseCAVI.from_inputs(lik, x, y, z, ELL, jitter=JITTER, ctx=ctx, keep_points=True)
    res = fresh.loo()  # before any sweep: the sites come from a pass of loo's own
    assert tuple(res.logp.shape) == (N,) and bool(torch.isfinite(res.logp).all()) and res.n_bad == 0
    with pytest.raises(A.ArgumentError, match="keep_inputs=True"):
        fresh.hyper_grad()
    with pytest.raises(A.ArgumentError, match="keep_inputs=True"):
        from_features(A, A.SparseCAVI, lik, cavi.plan, y, ctx).hyper_grad()


@pytest.mark.parametrize("kind", KINDS)
def test_cavi_constructions_agree_on_results(A, world, kind):
    """Each route, taken twice, runs the same three sweeps bit for bit.  (The two routes do not agree with EACH OTHER to the bit:
    the float32 features decoded from a plan's image are rounded once more when a second plan splits them again.)"""
    ctx, x, z, _, made = world
    lik, y, b = made[kind]  # from_inputs, three sweeps
    b2 = A.SparseCAVI.from_inputs(lik, x, y, z, ELL, jitter=JITTER, ctx=ctx)
    b2.run(3)
    assert torch.equal(b2.G, b.G) and torch.equal(b2.g, b.g)
    assert state_differences(b2.plan, b.plan) == []
    a, a2 = (from_features(A, A.SparseCAVI, lik, b.plan, y, ctx) for _ in range(2))
    a.run(3), a2.run(3)
    assert torch.equal(a2.G, a.G) and torch.equal(a2.g, a.g)
    assert state_differences(a2.plan, a.plan) == []
    # across the routes: the same model -- sizes and residual equal, the natural parameters within the project's bar for them
    assert (a.N, a.M, a.L) == (b.N, b.M, b.L) and torch.equal(a.plan.resid, b.plan.resid) and torch.equal(a.resid, b.resid)
    for s, t in ((a.G, b.G), (a.g, b.g)):
        assert float((s - t).abs().max() / t.abs().max()) <= NAT_TOL


def test_gibbs_constructions_agree_on_results(A, world):
    """As above for the sampler: the same seed and the same route give the same prior draw and the same three draws."""
    _, x, z, _, made = world
    lik, y, cavi = made["bernoulli"]
    b, b2 = (A.SparseGibbs.from_inputs(lik, x, y, z, ELL, jitter=JITTER, ctx=A.Context(0, seed=77)) for _ in range(2))
    a, a2 = (from_features(A, A.SparseGibbs, lik, cavi.plan, y, A.Context(0, seed=77)) for _ in range(2))
    assert (a.N, a.M, a.L) == (b.N, b.M, b.L) and torch.equal(a.plan.resid, b.plan.resid) and torch.equal(a.kdiag, b.kdiag)
    for one, two in ((b, b2), (a, a2)):
        assert torch.equal(one.v, two.v)  # the prior draw
        for _ in range(3):
            assert torch.equal(one.sweep(), two.sweep())


CAVI_NEW_INPUT = {"predict": ("x",), "predict_cov": ("x",), "predict_grad": ("x",), "sample_f": ("x",), "sample_paths": (2,),
                  "sample_y": ("x", 2), "predict_y": ("x",), "predict_cdf": ("x", "y"), "predict_quantiles": ("x",),
                  "heldout_logp": ("x", "y")}
GIBBS_NEW_INPUT = {"predict": ("x", "V"), "sample_paths": ("V",), "sample_y": ("x", "V"), "predict_y": ("x", "V"),
                   "heldout_logp": ("x", "y", "V")}


@pytest.fixture(scope="module")
def feature_built(A, world):
    ctx, _, _, x_s, made = world
    lik, y, cavi = made["bernoulli"]
    given = {"x": x_s, "y": y[:NS], "V": torch.zeros((2, 1, M), dtype=torch.float64, device="cuda")}
    return (from_features(A, A.SparseCAVI, lik, cavi.plan, y, ctx), from_features(A, A.SparseGibbs, lik, cavi.plan, y, ctx),
            lambda args: [given.get(a, a) if isinstance(a, str) else a for a in args])


@pytest.mark.parametrize("name", sorted(CAVI_NEW_INPUT))
def test_feature_built_cavi_refuses_new_inputs(A, feature_built, name):
    cavi, _, args = feature_built
    with pytest.raises(A.ArgumentError) as e:
        getattr(cavi, name)(*args(CAVI_NEW_INPUT[name]))
    assert re.search(rf"\b{name} needs", str(e.value)) and "from_inputs" in str(e.value)


@pytest.mark.parametrize("name", sorted(GIBBS_NEW_INPUT))
def test_feature_built_gibbs_refuses_new_inputs(A, feature_built, name):
    _, gibbs, args = feature_built
    with pytest.raises(A.ArgumentError) as e:
        getattr(gibbs, name)(*args(GIBBS_NEW_INPUT[name]))
    assert re.search(rf"\b{name} needs", str(e.value)) and "from_inputs" in str(e.value)


# the methods of a plan that take new inputs: name -> (the call, whether it takes mu0_s, the shape of its first result for Ns inputs)
def _chain(plan):
    return torch.zeros((2, plan.L, plan.M), dtype=torch.float64, device="cuda")


NEW_INPUT = {
    "predict": (lambda p, lik, x, mu0: p.predict(x, mu0)[0], True, lambda L, d, n: (L, n)),
    "predict_chain": (lambda p, lik, x, mu0: p.predict_chain(_chain(p), x, mu0)[0], True, lambda L, d, n: (L, n)),
    "predict_cov": (lambda p, lik, x, mu0: p.predict_cov(x), False, lambda L, d, n: (L, n, n)),
    "predict_grad": (lambda p, lik, x, mu0: p.predict_grad(x)[0], False, lambda L, d, n: (L, d, n)),
    "sample_f": (lambda p, lik, x, mu0: p.sample_f(x, 2, mu0), True, lambda L, d, n: (2, L, n)),
    "Paths.__call__": (lambda p, lik, x, mu0: p.sample_paths(2, nfeatures=32)(x, mu0), True, lambda L, d, n: (2, L, n)),
    "predict_y_chain": (lambda p, lik, x, mu0: p.predict_y_chain(lik, _chain(p), x, None, mu0)[0], True, lambda L, d, n: (n,)),
}


@pytest.fixture(scope="module")
def plan_1d(A, world):
    ctx, x, _, _, _ = world
    z = torch.linspace(-3, 3, 12, dtype=torch.float64, device="cuda")  # a grid, lengthscale = 1.5 spacings: a well-conditioned K_ZZ
    return A.Plan.from_inputs(x[:, 0].contiguous(), z, 1.5 * 6 / 11, jitter=JITTER, ctx=ctx)


@pytest.mark.parametrize("name", sorted(NEW_INPUT))
def test_input_preparation(A, world, plan_1d, name):
    ctx, _, _, x_s, made = world
    lik, _, cavi = made["bernoulli"]
    call, takes_mu0, shape = NEW_INPUT[name]
    plan = cavi.plan
    assert tuple(call(plan, lik, x_s, None).shape) == shape(1, D, NS)
    with pytest.raises(A.ArgumentError, match=re.escape("must be [Ns, 2]")):
        call(plan, lik, torch.zeros((NS, 3), dtype=torch.float64, device="cuda"), None)
    assert tuple(call(plan_1d, lik, x_s[:, 0].contiguous(), None).shape) == shape(1, 1, NS)  # 1-D inputs on a D = 1 plan
    if takes_mu0:
        good = torch.zeros((1, NS), dtype=torch.float32, device="cuda")
        assert tuple(call(plan, lik, x_s, good).shape) == shape(1, D, NS)
        with pytest.raises(A.ArgumentError, match="mu0_s must be"):
            call(plan, lik, x_s, torch.zeros(NS + 1, dtype=torch.float32, device="cuda"))
    ctx.synchronize()
