"""The float64 reference loop of tests/zgrad_learn_reference.py on the CPU, with the settings tests/test_gpu_zgrad_learn.py uses
(N = 4096, M = 16 inducing inputs started bunched in the first third of the inputs' range, 8 outer steps of 3 sweeps): learning
the inducing inputs with the kernel raises the ELBO by more than learning the kernel alone, and spreads them out."""
import numpy as np

import hyper_learn_reference as LR
import zgrad_learn_reference as ZL


def test_learning_the_inducing_inputs_gains_more_than_the_kernel_alone(oracle):
    x, y = oracle.synth_x(LR.SEED, 0, ZL.N), oracle.synth_y(oracle.bernoulli(), LR.SEED, 0, ZL.N)
    with_z, without = ZL.reference_loop(oracle, x, y, True), ZL.reference_loop(oracle, x, y, False)
    gain, gain0 = with_z["elbo"][-1] - with_z["elbo"][0], without["elbo"][-1] - without["elbo"][0]
    print("gain with z", gain, "without", gain0, "z", with_z["z"][-1, :, 0])
    assert np.all(np.isfinite(with_z["elbo"])) and with_z["z"].shape == (ZL.NOUTER + 1, ZL.M, 1)
    assert with_z["elbo"][0] == without["elbo"][0]  # (the same first step: z has not moved yet)
    assert gain0 > 0 and gain > gain0, (gain, gain0)
    assert np.array_equal(without["z"][-1], without["z"][0])
    assert np.ptp(with_z["z"][-1]) > np.ptp(with_z["z"][0])
