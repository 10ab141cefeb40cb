"""The float64 reference loop of tests/hyper_learn_reference.py on the CPU: with the settings tests/test_gpu_hyper_learn.py uses
(N = 4096, M = 32, the lengthscale started at three times the generating one, 8 outer steps of 3 sweeps) following the reference
gradient raises the ELBO by at least 1 % of its magnitude and moves the lengthscale towards the generating one."""
import numpy as np

import hyper_learn_reference as LR


def test_the_reference_loop_raises_the_elbo_by_one_percent(oracle):
    x, y = oracle.synth_x(LR.SEED, 0, LR.N), oracle.synth_y(oracle.bernoulli(), LR.SEED, 0, LR.N)
    tr = LR.reference_loop(oracle, x, y)
    gain = tr["elbo"][-1] - tr["elbo"][0]
    print("elbo", tr["elbo"], "log ell", tr["log_lengthscale"], "log var", tr["log_variance"])
    assert np.all(np.isfinite(tr["elbo"]))
    assert gain >= 0.01 * abs(tr["elbo"][0]), (gain, tr["elbo"][0])
    assert tr["log_lengthscale"][-1] < tr["log_lengthscale"][0]
