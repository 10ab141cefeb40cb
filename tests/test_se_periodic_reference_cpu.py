"""CPU checks of tests/se_periodic_reference.py (the float64 reference of the squared exponential x periodic kernel), of the cases
tests/test_gpu_se_periodic.py uses, and of the host-side surface of the kind: the binding's constant, ``kernel_kind``, the refusals
and the spectral measure."""
import os
import re
import subprocess

import numpy as np
import pytest

import kernels_reference as K
import periodic_reference as P
import se_periodic_reference as SP

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_kind_on_the_host():
    """Fails without the feature: ``("se_periodic", p)`` is no kernel."""
    import agpl_amd as A
    from agpl_amd import _ffi
    from agpl_amd.sparse import kernel_kind

    assert kernel_kind(("se_periodic", 2.5)) == (8, 2.5)
    hdr = open(os.path.join(ROOT, "include", "agpl_kernels.h")).read()
    assert "AGPL_KERNEL_SE_PERIODIC = AGPL_KERNEL_RQ + 4" in hdr and _ffi.KERNEL_SE_PERIODIC == SP.KIND == K.RQ + 4
    assert kernel_kind(("periodic", 2.5)) == (6, 2.5) and kernel_kind(("rq", 2)) == (4, 2.0)
    for bad in (("se_periodic", 0.0), ("se_periodic", -1.0), ("se_periodic", float("nan")), ("se_periodic", float("inf")),
                ("se_periodic",), "se_periodic"):
        with pytest.raises(A.ArgumentError):
            A.Plan.from_inputs(None, None, 1.0, kernel=bad)
    with pytest.raises(A.ArgumentError, match="period"):
        kernel_kind(("se_periodic", 0.0))
    with pytest.raises(A.ArgumentError, match="se_periodic"):  # the error text lists the new form
        kernel_kind("no such kernel")
    with pytest.raises(A.ArgumentError, match="lengthscale"):
        A.spectral_frequencies(("se_periodic", 1.0), 8, 2, device="cpu")
    with pytest.raises(A.AGPLError, match="select_inducing_greedy") as e:
        A.select_inducing(None, 4, kernel=("se_periodic", 1.0))
    assert e.value.code == _ffi.ERR_UNSUPPORTED


@pytest.mark.parametrize("p", SP.PERIODS)
def test_kernel_is_se_in_the_leading_dimensions_times_periodic_in_the_last(p):
    for D in (2, 3, 4):
        x, z, ell = SP.workload(50, 64, D, p)
        k = SP.kernel(x, z, ell, 1.7, p)
        se = K.kernel(K.SE, x[:, :-1], z[:, :-1], ell[:-1], 1.7)
        per = P.kernel(x[:, -1:], z[:, -1:], ell[-1:], 1.0, p)
        assert np.abs(k - se * per).max() <= 1e-14
        shift = np.zeros(D)
        shift[-1] = p
        assert np.abs(SP.kernel(x, z + shift, ell, 1.7, p) - k).max() <= 1e-14  # repeats in the last dimension
        shift = np.zeros(D)
        shift[0] = p
        assert np.abs(SP.kernel(x, z + shift, ell, 1.7, p) - k).max() > 1e-2  # and in no other
    x, z, ell = SP.workload(50, 16, 1, p)  # D = 1: the periodic kernel
    assert np.array_equal(SP.kernel(x, z, ell, 1.7, p), P.kernel(x, z, ell, 1.7, p))
    assert np.array_equal(SP.dkernel_da(x, z, ell, 1.7, p), P.dkernel_da(x, z, ell, 1.7, p))
    # x = (t, t): the locally periodic kernel SE(t) Per(t)
    x, z, ell = SP.locally_periodic(50, 16, p)
    want = K.kernel(K.SE, x[:, :1], z[:, :1], ell[:1], 1.0) * P.kernel(x[:, :1], z[:, :1], ell[1:], 1.0, p)
    assert np.abs(SP.kernel(x, z, ell, 1.0, p) - want).max() <= 1e-14


@pytest.mark.parametrize("p", SP.PERIODS)
def test_analytic_gradients_match_central_differences(p):
    D = 3
    x, z, ell = SP.workload(7, 16, D, p)
    z = z[:5].copy()
    z[1] = x[0]
    z[1, -1] += p / 2  # delta_last = p / 2 from a point: u at its maximum, u' = 0
    h = 1e-6
    for d in range(D):
        e = np.zeros(D)
        e[d] = h
        num = (SP.kernel(x + e, z, ell, 2.0, p) - SP.kernel(x - e, z, ell, 2.0, p)) / (2 * h)
        assert np.abs(SP.dkernel_da(x, z, ell, 2.0, p)[d] - num).max() < 1e-7
        up, dn = ell * np.exp(e), ell * np.exp(-e)
        num = (SP.kernel(x, z, up, 2.0, p) - SP.kernel(x, z, dn, 2.0, p)) / (2 * h)
        assert np.abs(SP.dkernel_dlogell(x, z, ell, 2.0, p)[d] - num).max() < 1e-7
        num = (SP.phi_f64(x + e, z, ell, 2.0, p)[0] - SP.phi_f64(x - e, z, ell, 2.0, p)[0]) / (2 * h)
        assert np.abs(SP.dphi_dx(x, z, ell, 2.0, p)[d] - num).max() < 1e-6
        # the prior variance of d f / d x_d: d^2 k / dx_d dx'_d at x = x' by a second difference
        o = np.zeros((1, D))
        num = (2 * SP.kernel(o, o, ell, 2.0, p)[0, 0] - SP.kernel(o + e * 1e2, o, ell, 2.0, p)[0, 0]
               - SP.kernel(o - e * 1e2, o, ell, 2.0, p)[0, 0]) / (h * 1e2) ** 2
        assert abs(SP.prior_grad_variance(ell, 2.0, p)[d] - num) < 1e-4 * num
    u, du = SP.warp(x[:1], z[1:2], ell, p)
    assert abs(abs(u[0, 0, -1]) - 1 / ell[-1]) < 1e-14 and abs(du[0, 0, -1]) < 1e-14 and (du[0, 0, :-1] == 1 / ell[:-1]).all()


def test_bound_gradients_analytic_against_autograd():
    """The analytic gradients of the sweep's bound (the rule's u and u' in closed form) against autograd through the whole bound, with
    an inducing input at delta_last = p / 2 from a point."""
    import hyper_reference as HR

    p, M, N, D = 2.5, 16, 60, 3
    x, z, ells = SP.workload(N, M, D, p)
    z[1] = x[0]
    z[1, -1] += p / 2
    m, S, beta, gamma = HR.synthetic_q(M, 1, N, 3)[:4]
    g = SP.bound_gradients(x, z, ells, 1.3, p, 1e-6, m, S, beta, gamma)
    assert np.abs(g["theta"] - g["auto_theta"]).max() <= 1e-10 * g["scale_theta"].max()
    assert np.abs(g["z"] - g["auto_z"]).max() <= 1e-10 * g["scale_z"].max()
    assert np.abs(g["auto_z"]).max() > 0 and np.abs(g["auto_theta"]).max() > 0


def test_spectral_measure_reproduces_kappa():
    """With 2e5 frequencies the mean of cos(omega . delta_u) is kappa(delta) within 5 standard errors of that mean (computed here);
    the last column lies on the lattice 2 pi k ell / p and the leading ones do not."""
    import torch

    import agpl_amd as A

    p, D, nb = 2.5, 3, 25
    F = nb * A.sparse.MAX_PATH_FEATURES  # 204800, in calls of the largest number of features a call draws
    ell = SP.lengthscales(D)
    gen = torch.Generator(device="cpu").manual_seed(11)
    draws = [A.spectral_frequencies(("se_periodic", p), F // nb, D, generator=gen, device="cpu", lengthscale=ell) for _ in range(nb)]
    om, ph = torch.cat([d[0] for d in draws]).numpy(), torch.cat([d[1] for d in draws])
    assert om.shape == (F, D) and ph.shape == (F,) and 0 <= float(ph.min()) and float(ph.max()) < 2 * np.pi
    k = om[:, -1] * p / (2 * np.pi * ell[-1])
    assert np.abs(k - np.round(k)).max() < 1e-9 and np.abs(k).max() >= 1
    for d in range(D - 1):
        kd = om[:, d] * p / (2 * np.pi * ell[d])
        assert np.abs(kd - np.round(kd)).max() > 0.4  # a continuous draw: N(0, 1)
        assert abs(om[:, d].mean()) < 5 / np.sqrt(F) and abs(om[:, d].std() - 1) < 5 / np.sqrt(2 * F)
    for delta in ([0.1, -0.2, 0.3], [0.0, 0.0, 1.1], [0.3, 0.1, p + 0.2], [0.05, 0.0, p / 2], [0.0, 0.4, 0.0]):
        delta = np.array(delta)
        c = np.cos(om @ (delta / ell))
        se = c.std(ddof=1) / np.sqrt(F)
        kappa = SP.kernel(delta[None], np.zeros((1, D)), ell, 1.0, p)[0, 0]
        print(f"delta {delta}: mean {c.mean():.5f} kappa {kappa:.5f} se {se:.2e}")
        assert abs(c.mean() - kappa) <= 5 * se, (delta, c.mean(), kappa, se)
    # D = 1 is the periodic kind's measure, draw for draw
    g1, g2 = torch.Generator(device="cpu").manual_seed(3), torch.Generator(device="cpu").manual_seed(3)
    a = A.spectral_frequencies(("se_periodic", p), 64, 1, generator=g1, device="cpu", lengthscale=0.3)
    b = A.spectral_frequencies(("periodic", p), 64, 1, generator=g2, device="cpu", lengthscale=0.3)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def _gpu_inputs():
    """(label, z, ells, p, M) of every case of tests/test_gpu_se_periodic.py."""
    for D, M in SP.CASES:
        for p in SP.PERIODS:
            _, z, ells = SP.workload(8, M, D, p)
            yield f"D={D} M={M} p={p}", z, ells, p
    for p in SP.PERIODS:
        _, z, ells = SP.locally_periodic(8, 16, p)
        yield f"locally periodic p={p}", z, ells, p


def test_gpu_cases_are_no_worse_conditioned_than_the_existing_kinds():
    """cond(K_ZZ + jitter I) of every case of tests/test_gpu_se_periodic.py against the worst case of tests/kernels_reference.py's
    own (a condition on the inputs): the float64 reference alone carries them."""
    worst = 0.0
    for kind in K.KINDS:
        for M, D, s2 in K.SHAPES:
            _, z, ell = K.workload(K.N, M, D)
            worst = max(worst, np.linalg.cond(K.kernel(kind, z, z, ell, s2, K.param_of(kind)) + K.JITTER * np.eye(M)))
    for label, z, ells, p in _gpu_inputs():
        assert len(np.unique(np.floor(z[:, -1] / p))) == 1 or label.startswith("locally")  # the last coordinate within one period
        cond = np.linalg.cond(SP.kernel(z, z, ells, 1.0, p) + SP.JITTER * np.eye(len(z)))
        print(f"{label}: cond {cond:.4g} (worst existing {worst:.4g})")
        assert cond <= worst, (label, cond, worst)
    for D, M in SP.CASES:
        for p in SP.PERIODS:
            x, z, ells = SP.workload(777, M, D, p)
            Phi, res, _ = SP.phi_f64(x, z, ells, 1.0, p)
            med = np.median(res)
            print(f"D={D} M={M} p={p}: median residual {med:.3g} s2")
            # the features neither all zero (half the points keep more than half of s2 explained) nor all saturated
            assert np.abs(Phi).max() <= 1.0 and 1e-5 <= med <= 0.5


def test_variance_cases_keep_max_var_above_the_float32_floor():
    """The cases tests/test_gpu_se_periodic.py compares variances on keep max var >= 0.025 s2 (tests/test_gpu_periodic.py found
    that the float32 variance bar has no margin below that).  var = s2 - |phi|^2 + |U phi|^2 >= s2 - |phi|^2 whatever q(v) is, so
    the residual at the new inputs carries the condition without a device for D >= 2 and for the locally periodic case.  At D = 1
    the 16 inducing inputs explain all but 1.7e-4 s2 of the prior variance: max var there is what q(v) leaves (0.05 - 0.07 s2
    measured), it cannot be formed without the fit, and the GPU test asserts it itself, as the periodic kind's does."""
    for D, M, p in SP.FIT:
        _, z, ells = SP.workload(8, M, D, p)
        low = SP.max_var_lower_bound(SP.predict_inputs(z, p), z, ells, 1.0, p)
        print(f"D={D} M={M} p={p}: max var >= {low:.3g} s2")
        assert low >= 0.025 or D == 1, (D, M, p, low)
        assert D > 1 or low < 0.025  # (the reason D = 1 is left to the GPU test: should this change, assert it here too)
    for p in SP.PERIODS:
        _, z, ells = SP.locally_periodic(8, 16, p)
        low = SP.max_var_lower_bound(SP.locally_periodic_predict_inputs(p), z, ells, 1.0, p)
        print(f"locally periodic p={p}: max var >= {low:.3g} s2")
        assert low >= 0.025


@pytest.mark.parametrize("D,p", [(1, 1.0), (2, 1.0), (3, 2.5)])
def test_greedy_inputs_have_clear_pivot_margins(D, p):
    """The inputs of tests/test_gpu_se_periodic.py's greedy test: every pick after the first (a tie by construction, resolved to the
    lowest index) beats the runner-up by more than the periodic test's GREEDY_MARGIN s2."""
    x, ells = SP.greedy_inputs(D, p)
    piv, margins = SP.greedy_pivots(x, SP.GREEDY_M, ells, 1.0, p)
    print(f"D={D} p={p}: pivots {piv.tolist()} margins {np.array2string(margins, precision=2)}")
    assert piv[0] == 0 and len(set(piv.tolist())) == SP.GREEDY_M and (margins > P.GREEDY_MARGIN).all()


@pytest.mark.parametrize("source,names", [("agpl_kernels.hip", ["se_build_se_periodic_kernelILb0E"]),
                                          ("agpl_grad.hip", ["se_build_se_periodic_kernelILb1E"]),
                                          ("agpl_joint.hip", ["joint_cov_se_periodic_kernel"])])
def test_se_periodic_instantiations_keep_two_workgroups_per_cu(tmp_path, source, names):
    """What tests/test_periodic_reference_cpu.py asserts of the periodic kernels, for this kind's (their own names): one
    instantiation each, no private segment, no spilled VGPR, at most 256 VGPRs (two 256-thread workgroups per CU), the product on the
    matrix cores."""
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
        assert 0 < vgprs <= 256, (name, vgprs)
        body = asm[asm.index("\n" + name + ":"):]
        assert "v_mfma_f32_" in body[:body.index("s_endpgm")], name
