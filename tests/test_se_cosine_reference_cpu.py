"""CPU checks of tests/se_cosine_reference.py (the float64 reference of the squared exponential x cosine kernel), of the cases
tests/test_gpu_se_cosine.py uses, and of the host-side surface of the kind: the binding's constant, ``kernel_kind``, the refusals,
the spectral measure and the code-object metadata of the kind's kernels."""
import os
import re
import subprocess

import numpy as np
import pytest

import kernels_reference as K
import periodic_reference as P
import se_cosine_reference as SC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_kind_on_the_host():
    """Fails without the feature: ``("se_cosine", p)`` is no kernel."""
    import agpl_amd as A
    from agpl_amd import _ffi
    from agpl_amd.sparse import kernel_dim_modulated, kernel_dim_warped, kernel_kind

    assert kernel_kind(("se_cosine", 2.5)) == (10, 2.5)
    hdr = open(os.path.join(ROOT, "include", "agpl_kernels.h")).read()
    assert "AGPL_KERNEL_SE_COSINE = AGPL_KERNEL_RQ + 6" in hdr and _ffi.KERNEL_SE_COSINE == SC.KIND == K.RQ + 6
    assert kernel_kind(("se_periodic", 2.5)) == (8, 2.5) and kernel_kind(("periodic", 2.5)) == (6, 2.5) and kernel_kind(("rq", 2)) == (4, 2.0)
    for bad in (("se_cosine", 0.0), ("se_cosine", -1.0), ("se_cosine", float("nan")), ("se_cosine", float("inf")), ("se_cosine",),
                "se_cosine"):
        with pytest.raises(A.ArgumentError):
            A.Plan.from_inputs(None, None, 1.0, kernel=bad)
    with pytest.raises(A.ArgumentError, match="the period p of the squared exponential x cosine kernel"):
        kernel_kind(("se_cosine", 0.0))
    with pytest.raises(A.ArgumentError, match="se_cosine"):  # the error text lists the new form
        kernel_kind("no such kernel")
    with pytest.raises(A.ArgumentError, match="lengthscale"):
        A.spectral_frequencies(("se_cosine", 1.0), 8, 2, device="cpu")
    with pytest.raises(A.AGPLError, match="select_inducing_greedy") as e:
        A.select_inducing(None, 4, kernel=("se_cosine", 1.0))
    assert e.value.code == _ffi.ERR_UNSUPPORTED
    # the host's copy of the predicate: the last dimension of kind 10 and nothing else; the kind warps nothing
    for D in (1, 2, 16):
        assert [kernel_dim_modulated(10, d, D) for d in range(D)] == [False] * (D - 1) + [True]
        assert not any(kernel_dim_warped(10, d, D) for d in range(D))
        assert not any(kernel_dim_modulated(k, d, D) for k in (0, 1, 2, 3, 4, 6, 8) for d in range(D))


def test_kinds_5_7_and_9_stay_refused_by_the_host_table():
    from agpl_amd.sparse import _KERNEL_NAMES

    assert sorted(_KERNEL_NAMES) == [0, 1, 2, 3, 4, 6, 8, 10]
    rules = open(os.path.join(ROOT, "augmentedgplikelihoods.jl_amd", "csrc", "agpl_kernel_rules.h")).read()
    known = re.search(r"bool kernel_kind_known\(int kind\) \{(.*?)\}", rules, flags=re.S).group(1)
    assert re.findall(r"AGPL_KERNEL_\w+", known) == ["AGPL_KERNEL_SE", "AGPL_KERNEL_RQ", "AGPL_KERNEL_PERIODIC", "AGPL_KERNEL_SE_PERIODIC",
                                                     "AGPL_KERNEL_SE_COSINE"]  # 0 .. 4, 6, 8, 10


@pytest.mark.parametrize("ratio", SC.RATIOS)
def test_kernel_is_the_squared_exponential_times_a_cosine(ratio):
    for D, M in SC.CASES:
        x, z, ell, p = SC.workload(50, M, D, ratio)
        k = SC.kernel(x, z, ell, 1.7, p)
        se = K.kernel(K.SE, x, z, ell, 1.7)
        cos = np.cos(2 * np.pi * (x[:, None, -1] - z[None, :, -1]) / p)
        exact = SC.cospi(2 * (x[:, None, -1] - z[None, :, -1]) / p)
        assert np.array_equal(k, se * exact)  # exactly the squared exponential reference times the factor
        assert np.abs(k - se * cos).max() <= 1e-14
        assert (k < 0).any() and (k > 0).any()
        assert np.array_equal(SC.kernel(x, x, ell, 1.7, p), SC.kernel(x, x, ell, 1.7, p).T)  # symmetric to the bit
        assert np.array_equal(np.diag(SC.kernel(x, x, ell, 1.7, p)), np.full(50, 1.7))
        # the placed pairs: half a period (k = -s2 E, E = 1 here) and a quarter period (k = 0)
        assert abs(k[0, 1] + 1.7 * np.exp(-0.5 * (0.5 * p / ell[-1]) ** 2)) <= 1e-14 and abs(k[0, 2]) <= 1e-14
    # at exact lags: 0 a quarter period away, -E half a period away, +E a whole period away
    o, ell = np.zeros((1, 2)), SC.lengthscales(2)
    for p in (1.0, 2.5, 0.25):
        at = lambda t: SC.kernel(np.array([[0.1, t]]), np.array([[0.1, 0.0]]), ell, 1.0, p)[0, 0]
        assert at(p / 4) == 0.0 and at(-p / 4) == 0.0 and at(3 * p / 4) == 0.0
        assert at(p / 2) == -np.exp(-0.5 * (p / 2 / ell[1]) ** 2) < 0 and at(p) == np.exp(-0.5 * (p / ell[1]) ** 2)
    # a very long period: the squared exponential, to 1e-12 of scale
    x, z, ell, _ = SC.workload(50, 64, 3, 0.3)
    assert np.abs(SC.kernel(x, z, ell, 1.7, 1e12) - K.kernel(K.SE, x, z, ell, 1.7)).max() <= 1e-12 * 1.7


@pytest.mark.parametrize("ratio", SC.RATIOS)
def test_analytic_gradients_match_central_differences(ratio):
    D = 3
    x, z, ell, p = SC.workload(7, 16, D, ratio)
    z = z[:5].copy()  # (keeps the placed pairs: z[1] half a period and z[2] a quarter period from x[0])
    h = 1e-6 * min(p, ell.min())
    scale = 2.0 * max(1 / ell.min(), 2 * np.pi / p)  # the size of d k / d x
    for d in range(D):
        e = np.zeros(D)
        e[d] = h
        num = (SC.kernel(x + e, z, ell, 2.0, p) - SC.kernel(x - e, z, ell, 2.0, p)) / (2 * h)
        assert np.abs(SC.dkernel_da(x, z, ell, 2.0, p)[d] - num).max() < 1e-7 * scale
        num = (SC.kernel(x, z + e, ell, 2.0, p) - SC.kernel(x, z - e, ell, 2.0, p)) / (2 * h)
        assert np.abs(-SC.dkernel_da(x, z, ell, 2.0, p)[d] - num).max() < 1e-7 * scale  # d / d z_d is the negative
        up, dn = ell * np.exp(1e-6 * (e > 0)), ell * np.exp(-1e-6 * (e > 0))
        num = (SC.kernel(x, z, up, 2.0, p) - SC.kernel(x, z, dn, 2.0, p)) / 2e-6
        assert np.abs(SC.dkernel_dlogell(x, z, ell, 2.0, p)[d] - num).max() < 1e-7 * 2.0 * 25
        num = (SC.phi_f64(x + e, z, ell, 2.0, p)[0] - SC.phi_f64(x - e, z, ell, 2.0, p)[0]) / (2 * h)
        assert np.abs(SC.dphi_dx(x, z, ell, 2.0, p)[d] - num).max() < 1e-6 * np.abs(num).max()
        # -d^2 k / d tau_d^2 at 0 by a second difference: the prior variance of d f / d x_d, and the stated normalisation
        o, hh = np.zeros((1, D)), 1e2 * e
        num = (2 * SC.kernel(o, o, ell, 2.0, p)[0, 0] - SC.kernel(o + hh, o, ell, 2.0, p)[0, 0] - SC.kernel(o - hh, o, ell, 2.0, p)[0, 0]) / hh[d] ** 2
        assert abs(SC.prior_grad_variance(ell, 2.0, p)[d] - num) < 1e-4 * num
    want = 1.0 / ell ** 2
    want[-1] += (2 * np.pi / p) ** 2
    assert np.allclose(SC.prior_grad_variance(ell, 2.0, p), 2.0 * want, rtol=1e-15)
    c = SC.grad_normalisation(ell, p)
    assert (c[:-1] == 1).all() and c[-1] == 1 + (2 * np.pi * ell[-1] / p) ** 2
    assert np.allclose(c * 2.0 / ell ** 2, SC.prior_grad_variance(ell, 2.0, p), rtol=1e-14)
    # the placed pairs: at half a period the factor's own derivative vanishes and d k / d x_L is the envelope's, with the sign flipped
    dk = SC.dkernel_da(x[:1], z[1:3], ell, 2.0, p)[-1, 0]
    u = (x[0, -1] - z[1, -1]) / ell[-1]
    assert abs(dk[0] - 2.0 * np.exp(-0.5 * u * u) * u / ell[-1]) <= 1e-12 * scale
    u = (x[0, -1] - z[2, -1]) / ell[-1]  # a quarter period: k = 0 and d k / d x_L is all the factor's, -+(2 pi / p) E
    assert abs(abs(dk[1]) - 2.0 * np.exp(-0.5 * u * u) * 2 * np.pi / p) <= 1e-12 * scale


def test_bound_gradients_analytic_against_autograd():
    """The analytic gradients of the sweep's bound (the product rule in closed form) against autograd through the whole bound, with
    inducing inputs half and a quarter period from a point, in both regimes."""
    import hyper_reference as HR

    for ratio in SC.RATIOS:
        M, N, D = 16, 60, 3
        x, z, ells, p = SC.workload(N, M, D, ratio)
        m, S, beta, gamma = HR.synthetic_q(M, 1, N, 3)[:4]
        g = SC.bound_gradients(x, z, ells, 1.3, p, 1e-6, m, S, beta, gamma)
        assert np.abs(g["theta"] - g["auto_theta"]).max() <= 1e-10 * g["scale_theta"].max()
        assert np.abs(g["z"] - g["auto_z"]).max() <= 1e-10 * g["scale_z"].max()
        assert np.abs(g["auto_z"]).max() > 0 and np.abs(g["auto_theta"]).max() > 0


def test_spectral_measure_reproduces_kappa():
    """With 2e5 frequencies the mean of cos(omega . delta_u) is E c at delta within 5 standard errors of that mean (computed here), for
    the package's draw and for the reference's; the last column's |omega| sits near 2 pi ell_L / p."""
    import torch

    import agpl_amd as A

    D, nb = 3, 25
    F = nb * A.sparse.MAX_PATH_FEATURES  # 204800, in calls of the largest number of features a call draws
    ell = SC.lengthscales(D)
    for ratio in SC.RATIOS:
        p = SC.period_of(ell, ratio)
        shift = 2 * np.pi * ell[-1] / p
        gen = torch.Generator(device="cpu").manual_seed(11)
        draws = [A.spectral_frequencies(("se_cosine", p), F // nb, D, generator=gen, device="cpu", lengthscale=ell) for _ in range(nb)]
        om, ph = torch.cat([d[0] for d in draws]).numpy(), torch.cat([d[1] for d in draws])
        assert om.shape == (F, D) and ph.shape == (F,) and 0 <= float(ph.min()) and float(ph.max()) < 2 * np.pi
        for name, w in (("package", om), ("reference", SC.spectral_draw(np.random.default_rng(3), F, D, ell, p))):
            for d in range(D - 1):  # N(0, 1)
                assert abs(w[:, d].mean()) < 5 / np.sqrt(F) and abs(w[:, d].std() - 1) < 5 / np.sqrt(2 * F)
            last = w[:, -1]
            # n +- shift with a fair sign: mean 0 +- 5 se, variance 1 + shift^2, and E |omega| that of the folded normal at shift
            assert abs(last.mean()) < 5 * np.sqrt((1 + shift ** 2) / F)
            assert abs((np.abs(last) - shift >= 0).mean() - 0.5) < 0.5 * np.exp(-0.5 * shift ** 2) + 5 / np.sqrt(F)
            from math import erf
            folded = np.sqrt(2 / np.pi) * np.exp(-0.5 * shift ** 2) + shift * erf(shift / np.sqrt(2))
            assert abs(np.abs(last).mean() - folded) < 5 * np.sqrt((1 + shift ** 2) / F), (name, np.abs(last).mean(), folded)
            assert abs(np.abs(last).mean() - shift) < 0.2 * shift + np.sqrt(2 / np.pi)  # near 2 pi ell_L / p
            for delta in ([0.1, -0.2, 0.3 * p], [0.0, 0.0, 0.25 * p], [0.3, 0.1, 0.5 * p], [0.05, 0.0, p], [0.0, 0.4, 0.0],
                          [0.0, 0.0, 0.6 * ell[-1]]):
                delta = np.array(delta)
                c = np.cos(w @ (delta / ell))
                se = c.std(ddof=1) / np.sqrt(F)
                kappa = SC.kernel(delta[None], np.zeros((1, D)), ell, 1.0, p)[0, 0]
                print(f"{name} ratio {ratio} delta {delta}: mean {c.mean():.5f} E c {kappa:.5f} se {se:.2e}")
                assert abs(c.mean() - kappa) <= 5 * se, (name, delta, c.mean(), kappa, se)


def _gpu_inputs():
    """(label, z, ells, p) of every case of tests/test_gpu_se_cosine.py."""
    for D, M in SC.CASES:
        for ratio in SC.RATIOS:
            _, z, ells, p = SC.workload(8, M, D, ratio)
            yield f"D={D} M={M} ell/p={ratio}", z, ells, p


def test_gpu_cases_are_no_worse_conditioned_than_the_existing_kinds():
    """cond(K_ZZ + jitter I) of every case of tests/test_gpu_se_cosine.py against the worst case of tests/kernels_reference.py's
    own (a condition on the inputs): the float64 reference alone carries them."""
    worst = 0.0
    for kind in K.KINDS:
        for M, D, s2 in K.SHAPES:
            _, z, ell = K.workload(K.N, M, D)
            worst = max(worst, np.linalg.cond(K.kernel(kind, z, z, ell, s2, K.param_of(kind)) + K.JITTER * np.eye(M)))
    for label, z, ells, p in _gpu_inputs():
        cond = np.linalg.cond(SC.kernel(z, z, ells, 1.0, p) + SC.JITTER * np.eye(len(z)))
        print(f"{label}: cond {cond:.4g} (worst existing {worst:.4g})")
        assert cond <= worst, (label, cond, worst)
    for D, M in SC.CASES:
        for ratio in SC.RATIOS:
            for N in SC.NS:
                xN, zN, _, _ = SC.workload(N, M, D, ratio)
                assert np.array_equal(zN, SC.workload(8, M, D, ratio)[1])  # z does not depend on N
            x, z, ells, p = SC.workload(777, M, D, ratio)
            assert x[:, :-1].min(initial=0) >= 0 and x[:, :-1].max(initial=1) <= 1 and np.ptp(x[:, -1]) >= 3 * p  # the last coordinate spans a few periods
            Phi, res, _ = SC.phi_f64(x, z, ells, 1.0, p)
            k = SC.kernel(x, z, ells, 1.0, p)
            print(f"D={D} M={M} ell/p={ratio}: median residual {np.median(res):.3g} s2, min k {k.min():.3f}, max |phi| {np.abs(Phi).max():.3f}")
            # the features neither all zero nor beyond the Nystrom bound, and k well on both sides of zero
            assert 1e-2 <= np.abs(Phi).max() <= 1.0 and k.min() <= -0.1 and k.max() >= 0.1
            # the placed pairs, to the rounding of the coordinates themselves
            assert abs(k[0, 1] + np.exp(-0.5 * (0.5 * p / ells[-1]) ** 2)) <= 1e-14 and abs(k[0, 2]) <= 1e-14


def test_variance_cases_keep_max_var_above_the_float32_floor():
    """The cases tests/test_gpu_se_cosine.py compares variances on keep max var >= 0.025 s2 (tests/test_gpu_periodic.py found that
    the float32 variance bar has no margin below that).  var = s2 - |phi|^2 + |U phi|^2 >= s2 - |phi|^2 whatever q(v) is, and the new
    inputs reach two lengthscales beyond the inducing inputs' stretch, so the residual alone carries the condition in every case."""
    for D, M, ratio in SC.FIT:
        _, z, ells, p = SC.workload(8, M, D, ratio)
        low = SC.max_var_lower_bound(SC.predict_inputs(z, ells, p, ratio), z, ells, 1.0, p)
        print(f"D={D} M={M} ell/p={ratio}: max var >= {low:.3g} s2")
        assert low >= 0.025, (D, M, ratio, low)


@pytest.mark.parametrize("D,ratio,periods", SC.GREEDY_CASES)
def test_greedy_inputs_have_clear_pivot_margins(D, ratio, periods):
    """The inputs of tests/test_gpu_se_cosine.py's greedy test: every pick after the first (a tie by construction, resolved to the
    lowest index) beats the runner-up by more than the periodic test's GREEDY_MARGIN s2."""
    x, ells, p = SC.greedy_inputs(D, ratio, periods)
    piv, margins = SC.greedy_pivots(x, SC.GREEDY_M, ells, 1.0, p)
    print(f"D={D} ell/p={ratio}: pivots {piv.tolist()} margins {np.array2string(margins, precision=2)}")
    assert piv[0] == 0 and len(set(piv.tolist())) == SC.GREEDY_M and (margins > P.GREEDY_MARGIN).all()
    assert (SC.kernel(x[piv], x[piv], ells, 1.0, p) < -1e-3).any()  # the picks meet k below zero


@pytest.mark.parametrize("source,names", [("agpl_kernels.hip", ["se_build_se_cosine_kernelILb0E"]),
                                          ("agpl_grad.hip", ["se_build_se_cosine_kernelILb1E"]),
                                          ("agpl_joint.hip", ["joint_cov_se_cosine_kernel"]),
                                          ("agpl_hyper.hip", ["hy_points_kernelILi10ELi%dELb0E" % dt for dt in (1, 4, 16)]),
                                          ("agpl_zgrad.hip", ["hy_points_kernelILi10ELi%dELb1E" % dt for dt in (1, 4, 16)])])
def test_se_cosine_kernels_have_no_scratch(tmp_path, source, names):
    """The code-object metadata of the kind's kernels (names of their own), as tests/test_se_periodic_reference_cpu.py reads it: one
    instantiation each, no private segment, no spilled VGPR; the two generator kernels and the joint kernel at most 256 VGPRs (two
    256-thread workgroups per CU) with the product on the matrix cores."""
    hipcc = "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc")
    csrc = os.path.join(ROOT, "augmentedgplikelihoods.jl_amd", "csrc")
    flags = re.search(r"^COMMON\s*:=\s*(.*)$", open(os.path.join(csrc, "Makefile")).read(), flags=re.M).group(1)
    flags = flags.replace("$(ARCH)", "gfx950").split()
    subprocess.check_call([hipcc] + flags + ["--cuda-device-only", "-S", os.path.join(csrc, source), "-o", "k.s"], cwd=tmp_path,
                          stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    asm = open(os.path.join(tmp_path, "k.s")).read()
    for want in names:
        blocks = re.findall(r"\.name:\s+(_Z\w*" + want + r"\w*)(.*?)(?=\n  - |\Z)", asm, flags=re.S)
        assert len(blocks) == 1, (want, [b[0] for b in blocks])
        name, meta = blocks[0]
        assert re.search(r"\.private_segment_fixed_size:\s+0\b", meta) and re.search(r"\.vgpr_spill_count:\s+0\b", meta), name
        vgprs = int(re.search(r"\.vgpr_count:\s+(\d+)", meta).group(1))
        print(source, want, "vgpr_count", vgprs)
        body = asm[asm.index("\n" + name + ":"):]
        assert "v_mfma_f32_" in body[:body.index("s_endpgm")], name
        if "hy_points" not in want:
            assert 0 < vgprs <= 256, (name, vgprs)
