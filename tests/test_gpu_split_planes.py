"""The low-order float16 plane of both sweep contractions, element by element (tests/split_reference.py: data whose checked sums are
short and same-signed, placed at the seams of a long launch; float64 references; bars from the arithmetic; the CPU proof that named
wrong variants leave them is tests/test_split_reference_cpu.py).

  * accumulation (syrk_strip_kernel behind agpl_cavi_pass_plan): point-banded features; exact zeros between the bands, exact symmetry,
    bitwise repeat, |G - ref| <= bar_ab and |g - ref| <= bar_a with the gamma, beta the pass exports;
  * marginal pass (marginal_factor_queue_kernel behind agpl_marginals_plan and agpl_cavi_pass_plan): stage-banded positive features
    against a dense positive U with same-signed lo parts, written through G, g and one update and READ BACK from the plan.

Every test first asserts from the data alone that each cross term, at every seam position / stage, is worth >= 4 bars on some
checked element.  SPLIT_ERR lines: the largest |device - float64| / bar."""
import numpy as np
import pytest

import split_reference as SR

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")


@pytest.fixture(scope="module")
def A():
    import agpl_amd as A

    return A


@pytest.fixture(scope="module")
def ctx(A):
    return A.Context(0, seed=13)


def _lik(A, L):
    return A.BernoulliLikelihood() if L == 1 else A.CategoricalLikelihood(np.zeros(L))


@pytest.mark.parametrize("case", SR.ACC_CASES, ids=lambda c: c.id)
def test_accumulation_sees_both_cross_terms_at_every_seam(A, ctx, case):
    N, M, L = case
    d = SR.acc_data(case)
    cavi = A.SparseCAVI(_lik(A, L), torch.from_numpy(SR.acc_dense(d)).cuda(), torch.from_numpy(d.resid).cuda(),
                        torch.from_numpy(d.y).cuda(), ctx=ctx, keep_points=True)
    assert cavi.plan is not None and cavi.plan.scale_exp == d.e
    cavi.accumulate()
    G, g = cavi.G.cpu().numpy().copy(), cavi.g.cpu().numpy().copy()
    cavi.accumulate()
    cavi.check()
    gamma, beta = cavi.gamma.cpu().numpy(), cavi.beta.cpu().numpy()
    assert gamma.shape == (L, N) and np.all(gamma > 0)
    Gr, gr = SR.acc_reference(d, gamma, beta)
    bG, bg = SR.acc_bars(d, gamma, beta)
    vis = SR.acc_visibility(d, gamma, bG)  # from the data alone
    assert vis >= 4.0, vis
    assert np.array_equal(cavi.G.cpu().numpy(), G) and np.array_equal(cavi.g.cpu().numpy(), g), "not bitwise reproducible"
    T = len(d.positions)
    off = (np.arange(M)[:, None] - np.arange(M)[None, :]) % T != 0
    assert np.all(G[:, off] == 0.0), "cross-talk between steps, slots or slices"
    assert np.array_equal(G, G.transpose(0, 2, 1))
    rG, rg = SR.ratio(G, Gr, bG), SR.ratio(g, gr, bg)
    print(f"SPLIT_ERR acc {case.id} G {rG:.3f} g {rg:.3f} (smallest cross term {vis:.1f} bars, {T} seam positions)")
    assert rG <= 1.0 and rg <= 1.0, (rG, rg)


@pytest.mark.parametrize("case", SR.MARG_CASES, ids=lambda c: c.id)
def test_marginal_pass_sees_both_cross_terms_in_every_stage(A, ctx, case):
    N, M, L, kind = case
    d = SR.marg_data(case)
    cavi = A.SparseCAVI(_lik(A, L), torch.from_numpy(d.Phi).cuda(), torch.from_numpy(d.resid).cuda(), torch.from_numpy(d.y).cuda(),
                        ctx=ctx, keep_points=True)
    assert cavi.plan is not None and cavi.plan.scale_exp == d.e
    cavi.G.copy_(torch.from_numpy(d.G))
    cavi.g.copy_(torch.from_numpy(d.g))
    cavi.update()
    cavi.check()
    Uv = np.stack([np.tril(cavi.plan.U_lead[l].cpu().numpy().T) for l in range(L)])  # U[a][b] is stored column-major
    v32 = cavi.plan.v32[:, :M].cpu().numpy().copy()
    assert np.abs(Uv - d.U_int).max() <= 1e-9 * np.abs(d.U_int).max()  # the update gave back the factor the data were made for
    assert np.abs(v32 - d.v_int).max() <= 1e-6
    ref = SR.marg_reference(d, Uv, v32)
    bars = SR.marg_bars(d, Uv, v32, ref)
    vis = SR.marg_visibility(d, Uv, bars, whole=kind == "dense")  # from the data alone
    assert vis >= 4.0, vis
    mu, var = (x.cpu().numpy() for x in cavi.marginals())
    rmu, rvar = SR.ratio(mu, ref.mu, bars.mu), SR.ratio(var, ref.var, bars.var)
    line = f"SPLIT_ERR marg {case.id} mu {rmu:.3f} var {rvar:.3f}"
    rc = 0.0
    if L == 1:  # the marginals inside a pass: Bernoulli, mu0 = 0, c = sqrt(mu^2 + var)
        cavi.accumulate()
        cavi.check()
        rc = SR.ratio(cavi.c.cpu().numpy()[None, :], ref.c, bars.c)
        line += f" c {rc:.3f}"
    print(line + f" (smallest cross term {vis:.1f} bars)")
    assert rmu <= 1.0 and rvar <= 1.0 and rc <= 1.0, (rmu, rvar, rc)
