"""CPU tests of tests/chain_reference.py, the yardstick of the GPU tests of agpl_plan_predict_chain:

* on the data of every case of tests/test_gpu_chain_predict_shapes.py (and the tight chain of tests/test_gpu_chain_predict.py) a numpy
  model of the documented arithmetic stays within the element-wise bars, no element exempted -- the bars are not too tight for a
  correct implementation;
* six wrong variants of the epilogue and the packing each leave the bars in the GPU case named beside them -- the bars are tight
  enough to fail a subtly wrong kernel;
* the model itself has the exact properties the GPU tests ask of the kernel (power-of-two scales, constant and zero chains).

The features are random float64 rows of norm <= 1 passed through the image's split, as the plan's own features are.
"""
import numpy as np
import pytest

import chain_reference as R
from chain_reference import Case


def features(M, seed=7):
    rng = np.random.default_rng([seed, M])
    G = rng.standard_normal((R.N, M))
    Phi = G / np.linalg.norm(G, axis=1, keepdims=True) * rng.uniform(0.2, 1.0, size=(R.N, 1))
    return R.model_features(Phi)


_FEATS = {}


def feats(M):
    if M not in _FEATS:
        _FEATS[M] = features(M)
    return _FEATS[M]


def errors(c, mutate=None):
    """max over the elements of err / bar for (F, mean, spread) -- inf where err > 0 = bar -- and the outputs."""
    image, Phi = feats(c.M)
    V, mu0 = R.case_data(c)
    ref = R.reference(Phi, V, mu0)
    bar = R.bars(Phi, ref, R.plan_padded(c.M))
    out = R.model(image, V, mu0, mutate)
    worst = []
    for got, want, b in zip(out, (ref.F, ref.mean, ref.spread), (bar.F, bar.mean, bar.spread)):
        assert np.isfinite(got).all()
        err = np.abs(got.astype(np.float64) - want)
        with np.errstate(divide="ignore", invalid="ignore"):
            ratio = np.where(b > 0, err / b, np.where(err > 0, np.inf, 0.0))
        worst.append(float(np.max(ratio)))
    return worst, out


@pytest.mark.parametrize("c", R.CASES, ids=lambda c: c.id)
def test_the_model_is_within_the_bars(c):
    worst, _ = errors(c)
    print(f"{c.id}: max err / bar  F {worst[0]:.3f}  mean {worst[1]:.3f}  spread {worst[2]:.3f}")
    assert max(worst) <= 1.0, worst


# the GPU cases that must see each wrong variant: (mutation, case, the output that leaves its bar)
CAUGHT = [
    ("second_half_latent_from_0", Case(64, 3, 43, "separated", None), 0),   # T L = 129: rows 64 .. start at latent 64 % 3 = 1
    ("second_half_latent_from_0", Case(64, 5, 26, "separated", None), 2),
    ("second_half_latent_from_0", Case(64, 10, 13, "separated", None), 0),
    ("second_half_latent_from_0", Case(64, 33, 2, "separated", None), 0),
    ("base_of_next_latent", Case(64, 3, 11, "separated", None), 0),
    ("base_of_next_latent", Case(512, 2, 65, "separated", None), 0),
    ("no_lo_plane_of_V", Case(64, 1, 32, "separated", None), 0),
    ("no_lo_plane_of_V", Case(64, 1, 32, "separated", None), 2),
    ("no_lo_plane_of_V", Case(64, 2, 37, "small_latent", -20), 0),
    ("rows_32_up_of_last_group_skipped", Case(64, 1, 33, "separated", None), 0),
    ("rows_32_up_of_last_group_skipped", Case(64, 1, 129, "separated", None), 2),
    ("rows_32_up_of_last_group_skipped", Case(64, 33, 2, "separated", None), 1),  # vbar's block: latent 32
    ("rows_32_up_of_last_group_skipped", Case(64, 64, 3, "separated", None), 1),
    ("spread_as_difference_of_sums", Case(64, 1, 37, "tight", None), 2),
    ("spread_as_difference_of_sums", Case(200, 2, 37, "tight", None), 2),
    ("ssq_into_latent_0", Case(64, 3, 22, "separated", None), 2),
    ("ssq_into_latent_0", Case(64, 64, 2, "separated", None), 2),
]


@pytest.mark.parametrize("mutate,c,which", CAUGHT, ids=lambda v: v.id if isinstance(v, Case) else str(v))
def test_each_wrong_variant_leaves_the_bars(mutate, c, which):
    assert c in R.CASES
    worst, _ = errors(c, mutate)
    print(f"{mutate} at {c.id}: max err / bar  F {worst[0]:.3g}  mean {worst[1]:.3g}  spread {worst[2]:.3g}")
    assert worst[which] > 1.0, worst


def test_every_wrong_variant_is_listed():
    assert {m for m, _, _ in CAUGHT} == set(R.MUTATIONS)


def test_cases_are_the_issue_s():
    tl = sorted({c.T * c.L for c in R.SEAMS})
    for seam in (32, 33, 64, 65, 66, 128, 129, 130, 192, 256, 257, 384):
        assert seam in tl
    assert {c.L for c in R.SEAMS} == {1, 3, 5, 10, 33, 64}
    assert R.NS_EDGES in R.SEAMS
    assert len({c.id for c in R.CASES}) == len(R.CASES)


def test_power_of_two_scales_give_the_same_bits_in_the_model():
    image, _ = feats(64)
    outs = {c.arg: R.model(image, *R.case_data(c)) for c in R.POW2}
    for k in (20, -20):
        s = np.float32(2.0 ** k)
        assert np.array_equal(outs[k][0], outs[0][0] * s) and np.array_equal(outs[k][1], outs[0][1] * s)
        assert np.array_equal(outs[k][2], outs[0][2] * s * s)


def test_degenerate_chains_in_the_model():
    image, _ = feats(64)
    four, three, zero_mu0, zero = R.DEGENERATE
    V, mu0 = R.case_data(four)
    assert np.array_equal(R.chain_mean(V), V[0])  # four equal terms sum without rounding that survives
    F, mean, spread = R.model(image, V, mu0)
    assert not spread.any() and all(np.array_equal(F[t], mean) for t in range(four.T))
    V, mu0 = R.case_data(zero_mu0)
    F, mean, spread = R.model(image, V, mu0)
    assert np.array_equal(mean, mu0) and all(np.array_equal(F[t], mu0) for t in range(zero_mu0.T)) and not spread.any()
    F, mean, spread = R.model(image, *R.case_data(zero))
    assert not F.any() and not mean.any() and not spread.any()


def test_scale_rule():
    for mx in (1.0, 1.5, 2.0 ** -30, 3.7e5, 2.0 ** 13, np.nextafter(2.0 ** 14, 0)):
        assert 2.0 ** 13 <= mx * 2.0 ** R.scale_exp(mx) < 2.0 ** 14
    assert R.scale_exp(0.0) == 0 and R.scale_exp(2.0 ** -120) == 90 and R.scale_exp(2.0 ** 120) == -90


def test_reference_is_the_textbook_one():
    rng = np.random.default_rng(1)
    Phi, (V, mu0) = rng.standard_normal((R.N, 64)) / 8, R.separated(rng, 9, 3, 64)
    ref = R.reference(Phi, V, mu0)
    F = mu0.astype(np.float64) + np.einsum("na,tla->tln", Phi, V)
    assert np.allclose(ref.F, F, rtol=1e-13, atol=0) and np.allclose(ref.mean, F.mean(0), rtol=1e-13, atol=0)
    assert np.allclose(ref.spread, F.var(0), rtol=1e-9, atol=0)
