"""learn_hyperparameters on the GPU against the float64 reference loop of tests/hyper_learn_reference.py (the same schedule on the
oracle and the autograd gradient): 1-D Bernoulli data from synth_xy, N = 4096, M = 32, the lengthscale started at three times the
generating one, 8 outer steps of 3 sweeps.  And the step the loop rests on: a plan rebuilt into the same storage, with q(v) carried
over through Plan.state / load_state, gives the marginals it gave before."""
import numpy as np
import pytest

import hyper_learn_reference as LR

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

# |final log ell (device) - final log ell (reference loop)|: 4 x the worst value measured on an MI355X over the three seeds below
# (the margin covers another draw of the data).  Measured: 1.03e-5 (seed 5), 1.11e-5 (seed 6), 6.7e-6 (seed 7); the ELBO gains were
# 24.767 / 25.077 / 26.529 against the reference loop's 24.765 / 25.076 / 26.526.
LOG_ELL_MARGIN = 4 * 1.113e-05
SEEDS = [5, 6, 7]


@pytest.fixture(scope="module")
def A():
    import agpl_amd

    return agpl_amd


@pytest.mark.parametrize("seed", SEEDS)
def test_the_device_loop_follows_the_reference_loop(A, oracle, seed):
    ctx = A.Context(0, seed=23)
    lik = A.BernoulliLikelihood()
    x, y = A.synth_xy(lik, seed, 0, LR.N, ctx=ctx)
    z = torch.from_numpy(LR.Z).cuda()
    cavi, tr = A.learn_hyperparameters(lik, x, y, z, LR.ELL0, LR.VAR0, kernel=LR.KERNEL, nouter=LR.NOUTER, nsweeps=LR.NSWEEPS, lr=LR.LR,
                                       jitter=LR.JITTER, ctx=ctx)
    ref = LR.reference_loop(oracle, x.cpu().numpy(), y.cpu().numpy())
    gain, gain_ref = tr["elbo"][-1] - tr["elbo"][0], ref["elbo"][-1] - ref["elbo"][0]
    d_ell = abs(float(tr["log_lengthscale"][-1, 0]) - ref["log_lengthscale"][-1])
    d_var = abs(tr["log_variance"][-1] - ref["log_variance"][-1])
    print(f"HYPER_LEARN seed={seed} gain={gain:.4f} gain_ref={gain_ref:.4f} elbo0={tr['elbo'][0]:.4f} ref_elbo0={ref['elbo'][0]:.4f} "
          f"log_ell={float(tr['log_lengthscale'][-1, 0]):.8f} ref={ref['log_lengthscale'][-1]:.8f} d_ell={d_ell:.3e} d_var={d_var:.3e}")
    assert tr["log_lengthscale"].shape == (LR.NOUTER + 1, 1) and len(tr["elbo"]) == LR.NOUTER == cavi.nsweeps // LR.NSWEEPS
    assert gain_ref > 0 and gain >= 0.5 * gain_ref
    assert d_ell <= LOG_ELL_MARGIN


def test_q_survives_a_rebuild_into_the_same_storage(A):
    ctx = A.Context(0, seed=29)
    lik = A.BernoulliLikelihood()
    x, y = A.synth_xy(lik, 5, 0, 1000, ctx=ctx)
    z = torch.from_numpy(LR.Z).cuda()
    make = lambda mem: A.SparseCAVI.from_inputs(lik, x, y, z, 1.5, 2.0, LR.JITTER, ctx=ctx, keep_inputs=True, storage=mem, kernel=LR.KERNEL)
    a = make(None)
    a.run(3)
    mu, var = (t.clone() for t in a.marginals())
    st, mem = a.plan.state(), a.plan.mem
    a.plan.close()
    assert a.plan.U_colmajor is None and a.plan.resid is None  # (the closed plan no longer views the storage)
    a.plan.close()  # (idempotent)
    b = make(mem)
    assert b.plan.mem.data_ptr() == mem.data_ptr()
    assert not torch.equal(b.marginals()[0], mu)  # q(v) = N(0, I) again
    b.plan.load_state(st)
    mu_b, var_b = b.marginals()
    assert torch.equal(mu_b, mu) and torch.equal(var_b, var)
    with pytest.raises(A.ArgumentError):
        make(torch.empty(16, dtype=torch.uint8, device="cuda"))
