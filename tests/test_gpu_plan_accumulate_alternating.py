"""The plan's split-float16 accumulation (agpl_syrk.hip syrk_strip_kernel) with TWO different gamma | beta sets run alternately
through the SAME plan, each compared with its own float64 reference: G = Phi Diag(gamma) Phi', g = Phi beta.  A repeat test that
feeds one input cannot see a slab entry (or a g row) that a pass fails to write: the stale value of the previous pass is the
right one.  Here the previous pass had another gamma at every point (asserted: the two sets come from different posteriors), so a
stale entry of G is wrong by O(1); g is covered where beta depends on the posterior (L = 3).  Shapes: M = 256 (diagonal tiles only), 512 and 768, ragged N (last stage and last slice partly
filled), L = 3.  Bar: 5e-6 of max|ref| per array, that of tests/test_gpu_plan_accumulate.py; bitwise equality between the two
visits of the same set."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")


@pytest.fixture(scope="module")
def A():
    import agpl_amd as A

    return A


@pytest.fixture(scope="module")
def ctx(A):
    return A.Context(0, seed=13)


def relmax(a, b):
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))


def _float64_sums(Phi, gamma, beta):
    P = Phi.astype(np.float64)
    G = np.stack([(P * gamma[l].astype(np.float64)[:, None]).T @ P for l in range(gamma.shape[0])])
    g = np.stack([P.T @ beta[l].astype(np.float64) for l in range(beta.shape[0])])
    return G, g


@pytest.mark.parametrize("N,M,L", [(20011, 256, 3), (9013, 512, 3), (13007, 768, 3), (70001, 256, 1), (33, 512, 1)])
def test_two_inputs_alternate_through_one_plan(A, ctx, N, M, L):
    rng = np.random.default_rng(3 * N + M + L)
    Phi = (rng.standard_normal((N, M)) * 0.3).astype(np.float32)
    if L == 1:
        lik = A.BernoulliLikelihood()
        y = (rng.uniform(size=N) < 0.5).astype(np.uint8)
    else:
        lik = A.CategoricalLikelihood(np.zeros(L))
        lab = rng.integers(0, L + 1, size=N)
        y = (lab[:, None] == np.arange(L)[None, :]).astype(np.uint8)
    cavi = A.SparseCAVI(lik, torch.from_numpy(Phi).cuda(), torch.ones(N, device="cuda"), torch.from_numpy(y).cuda(), ctx=ctx,
                        keep_points=True)
    assert cavi.plan is not None
    # two posteriors q(v): the prior N(0, I) (the update of G = 0, g = 0) and the one the first pass's (G, g) gives -- gamma and
    # (for most likelihoods) beta are functions of q(v)
    cavi.accumulate()
    cavi.check()
    sets = [(torch.zeros_like(cavi.G), torch.zeros_like(cavi.g)), (cavi.G.clone(), cavi.g.clone())]
    seen = {}
    for visit in range(4):  # sets 0, 1, 0, 1
        k = visit & 1
        cavi.G.copy_(sets[k][0])
        cavi.g.copy_(sets[k][1])
        cavi.update()
        cavi.accumulate()
        cavi.check()
        G, g = cavi.G.cpu().numpy().copy(), cavi.g.cpu().numpy().copy()
        gamma, beta = cavi.gamma.cpu().numpy(), cavi.beta.cpu().numpy()
        assert gamma.shape == (L, N) and np.all(gamma > 0)
        Gr, gr = _float64_sums(Phi, gamma, beta)
        eG, eg = relmax(G, Gr), relmax(g, gr)
        print(f"N={N} M={M} L={L} visit {visit} set {k}: relmax G {eG:.3e} g {eg:.3e}")
        assert eG < 5e-6, eG
        assert eg < 5e-6, eg
        assert np.array_equal(G, G.transpose(0, 2, 1))
        if k in seen:
            assert np.array_equal(G, seen[k][0]) and np.array_equal(g, seen[k][1]), "a set's second visit differs from its first"
        seen[k] = (G, g, gamma.copy(), beta.copy())
    # the two sets really differ everywhere (else the alternation shows nothing)
    assert np.all(seen[0][2] != seen[1][2])  # gamma: a function of q(f_i), different at every point
    # (beta need not differ -- Bernoulli's is y - 1/2 whatever q is, and where it is equal a stale g entry is the right one)
    bdiff = float(np.mean(seen[0][3] != seen[1][3]))
    print(f"N={N} M={M} L={L}: beta differs at {bdiff:.3f} of the points")
    if L > 1:  # the logistic-softmax beta carries the expected auxiliary counts, which depend on q: here the g rows are covered too
        assert bdiff > 0.5
    assert relmax(seen[0][0], seen[1][0]) > 1e-3
