"""GPU tests of the shared descriptor check (csrc/agpl_lik_desc.h) as libagpl.so's own entry points see it (run with
-m gpu on an MI355X).  agpl_lik_to_device used to carry a copy of the check that had drifted from the extension libraries': it took a
non-finite r, nu or sigma and any lambda or beta.  Each of those descriptors is now refused as ArgumentError with the extensions'
message by an array-fed operator, the Gibbs auxiliary draw and the synthetic workload; a valid descriptor of each kind goes through the
same three calls as before.  n = 64 points: nothing here depends on the size."""
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

N = 64
SYNTH_KINDS = (0, 1, 2, 3, 4)  # the kinds agpl_synth_xy has a workload for


@pytest.fixture(scope="module")
def A():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import __graft_entry__ as g

    g.build()
    import agpl_amd

    return agpl_amd


@pytest.fixture(scope="module")
def ctx(A):
    return A.Context(0, seed=20261021)


def inputs(A, lik):
    """(y, f, var) of N points in the layout and element type of the kind: f in -2 .. 2, y away from f."""
    from agpl_amd import operators as ops

    L, cols = lik._nlatent, ops._ycols(lik)
    f = torch.linspace(-2.0, 2.0, N * L, dtype=torch.float64, device="cuda").reshape((N,) if L == 1 else (N, L))
    if lik.ykind == "i32x2":
        y = A.binomial_obs(torch.full((N,), 2, device="cuda"), torch.full((N,), 5, device="cuda"))
    elif lik.ykind == "u8":
        y = torch.zeros((N,) if cols == 1 else (N, cols), dtype=torch.uint8, device="cuda")
        if cols == 1:
            y[::2] = 1
        else:  # one-hot rows, the classes in turn
            y[torch.arange(N), torch.arange(N) % cols] = 1
    elif lik.ykind == "i32":
        y = torch.full((N,), 2, dtype=torch.int32, device="cuda")
    else:
        y = torch.full((N,), 3.5, dtype=torch.float64, device="cuda")
    return y, f, torch.full_like(f, 0.3)


def three_calls(A, ctx, lik):
    y, f, var = inputs(A, lik)
    return [lambda: A.aux_posterior(lik, y, (f, var), ctx=ctx), lambda: A.aux_sample(lik, y, f, ctx=ctx, sweep=1),
            lambda: A.synth_xy(lik, 7, 0, N, ctx=ctx)]


REFUSED = [
    ("NegativeBinomialLikelihood", (math.inf,), "NegBinomial failures r must be > 0"),
    ("StudentTLikelihood", (math.inf, 1.0), "StudentT needs nu > 0 and sigma > 0"),
    ("StudentTLikelihood", (3.0, math.inf), "StudentT needs nu > 0 and sigma > 0"),
    ("PoissonLikelihood", (-1.0,), "the link's scale lambda must be > 0"),
    ("PoissonLikelihood", (0.0,), "the link's scale lambda must be > 0"),
    ("PoissonLikelihood", (math.nan,), "the link's scale lambda must be > 0"),
    ("PoissonLikelihood", (math.inf,), "the link's scale lambda must be > 0"),
    ("HeteroscedasticGaussianLikelihood", (-1.0,), "the link's scale lambda must be > 0"),
    ("HeteroscedasticGaussianLikelihood", (math.inf,), "the link's scale lambda must be > 0"),
    ("LaplaceLikelihood", (-1.0,), "Laplace needs beta > 0"),
    ("LaplaceLikelihood", (0.0,), "Laplace needs beta > 0"),
    ("LaplaceLikelihood", (math.nan,), "Laplace needs beta > 0"),
    ("LaplaceLikelihood", (math.inf,), "Laplace needs beta > 0"),
]


@pytest.mark.parametrize("name,params,message", REFUSED, ids=["%s%r" % (n[:-10], p) for n, p, _ in REFUSED])
def test_the_core_refuses_what_the_extensions_refuse(A, ctx, name, params, message):
    lik = getattr(A, name)(*params)
    for call in three_calls(A, ctx, lik):
        with pytest.raises(A.ArgumentError) as info:
            call()
        assert info.value.code == -1 and str(info.value).endswith(": " + message), str(info.value)


VALID = [
    ("BernoulliLikelihood", ()), ("NegativeBinomialLikelihood", (2.5,)), ("StudentTLikelihood", (3.0, 1.5)), ("CategoricalLikelihood", (3,)),
    ("CategoricalLikelihood", (3, True)), ("PoissonLikelihood", (4.0,)), ("LaplaceLikelihood", (0.7,)),
    ("HeteroscedasticGaussianLikelihood", (2.0,)), ("BinomialLikelihood", (5,)), ("AsymmetricLaplaceLikelihood", (0.25, 0.5)),
    ("LogisticNoiseLikelihood", (0.7,)), ("BinomialTrialsLikelihood", ()),
]


@pytest.mark.parametrize("name,params", VALID, ids=["%s%r" % (n[:-10], p) for n, p in VALID])
def test_a_valid_descriptor_of_each_kind_still_runs(A, ctx, name, params):
    lik = getattr(A, name)(*params)
    posterior, draw, synth = three_calls(A, ctx, lik)
    q = posterior().inds[0]
    for key in q.keys():
        if key != "y":
            assert np.isfinite(q[key].cpu().numpy()).all(), key
    om = draw().ω.cpu().numpy()
    assert om.shape[0] == N and np.isfinite(om).all() and (om >= 0).all()  # (PG(0, c) of a class without counts is 0)
    if lik.kind in SYNTH_KINDS:
        x, y = synth()
        assert x.shape == (N,) and y.shape[0] == N and bool(((x >= -10) & (x <= 10)).all())
    elif lik.ykind == "i32x2":  # refused by the host before any device call, as before
        with pytest.raises(A.ArgumentError, match="trials"):
            synth()
    else:  # a valid descriptor without a synthetic workload: past the descriptor check, refused by agpl_synth_xy itself
        with pytest.raises(A.AGPLError, match="no synthetic workload is defined for likelihood kind %d" % lik.kind) as info:
            synth()
        assert info.value.code == -3
