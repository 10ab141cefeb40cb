"""CPU checks of tests/periodic_reference.py (the float64 reference of the periodic kernel), of the cases tests/test_gpu_periodic.py
uses, and of the host-side surface of the kind: the binding's constant, ``kernel_kind`` and the spectral weights."""
import os
import re
import subprocess

import numpy as np
import pytest

import kernels_reference as K
import periodic_reference as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("p", P.PERIODS)
def test_kernel_repeats_with_the_period(p):
    x, z, ell = P.workload(50, 64, 3, 0.3, p)
    k0 = P.kernel(x, z, ell, 1.0, p)
    for d in range(3):
        shift = np.zeros(3)
        shift[d] = p
        assert np.abs(P.kernel(x, z + shift, ell, 1.0, p) - k0).max() <= 1e-14


def test_kernel_tends_to_the_squared_exponential():
    """sin(pi delta / p) / ell -> delta / (ell p / pi) as p grows: SE with lengthscale ell p / pi, the difference O((delta / p)^2)."""
    rng = np.random.default_rng(1)
    a, b = rng.uniform(-1, 1, (20, 2)), rng.uniform(-1, 1, (30, 2))
    p, ell = 1e5, np.array([2e-5, 3e-5])
    se = K.kernel(K.SE, a, b, ell * p / np.pi, 1.7)
    assert np.abs(P.kernel(a, b, ell, 1.7, p) - se).max() < 1e-8


@pytest.mark.parametrize("p", P.PERIODS)
def test_analytic_gradients_match_central_differences(p):
    x, z, ell = P.workload(7, 16, 3, 0.3, p)
    z = z[:5]
    h = 1e-6
    for d in range(3):
        e = np.zeros(3)
        e[d] = h
        num = (P.kernel(x + e, z, ell, 2.0, p) - P.kernel(x - e, z, ell, 2.0, p)) / (2 * h)
        assert np.abs(P.dkernel_da(x, z, ell, 2.0, p)[d] - num).max() < 1e-7
        up, dn = ell * np.exp(e), ell * np.exp(-e)
        num = (P.kernel(x, z, up, 2.0, p) - P.kernel(x, z, dn, 2.0, p)) / (2 * h)
        assert np.abs(P.dkernel_dlogell(x, z, ell, 2.0, p)[d] - num).max() < 1e-7
        num = (P.phi_f64(x + e, z, ell, 2.0, p)[0] - P.phi_f64(x - e, z, ell, 2.0, p)[0]) / (2 * h)
        assert np.abs(P.dphi_dx(x, z, ell, 2.0, p)[d] - num).max() < 1e-6
    # delta = p / 2 exactly: u at its maximum, u' = 0
    u, du = P.warp(np.array([[p / 2]]), np.zeros((1, 1)), np.array([0.3]), p)
    assert abs(u[0, 0, 0] - 1 / 0.3) < 1e-15 and abs(du[0, 0, 0]) < 1e-15


@pytest.mark.parametrize("ell", [0.1, 0.3, 0.45, 1.5, 30.0])
def test_spectral_weights_sum_to_one_and_give_the_kernel(ell):
    from agpl_amd.sparse import periodic_spectral_weights

    w = periodic_spectral_weights(ell)
    assert abs(w[0] + 2 * w[1:].sum() - 1.0) < 1e-14 and (w > 0).all()
    ref = P.spectral_weights(ell, len(w) - 1)
    assert np.abs(w - ref).max() < 1e-13
    assert len(w) == 1 or ref[len(w):].sum() * 2 < 1e-16 + 1e-13
    for p in P.PERIODS:
        delta = np.linspace(-1.5 * p, 1.5 * p, 301)
        series = w[0] + 2 * (w[1:, None] * np.cos(2 * np.pi * np.arange(1, len(w))[:, None] * delta / p)).sum(0)
        kappa = np.exp(-np.sin(np.pi * delta / p) ** 2 / (2 * ell * ell))
        assert np.abs(series - kappa).max() < 1e-12


def test_gpu_cases_are_no_worse_conditioned_than_the_existing_kinds():
    """cond(K_ZZ + jitter I) of every case of tests/test_gpu_periodic.py against the worst case of tests/kernels_reference.py's own
    (a condition on the inputs): the float64 reference alone carries them."""
    worst = 0.0
    for kind in K.KINDS:
        for M, D, s2 in K.SHAPES:
            _, z, ell = K.workload(K.N, M, D)
            worst = max(worst, np.linalg.cond(K.kernel(kind, z, z, ell, s2, K.param_of(kind)) + K.JITTER * np.eye(M)))
    for D, M, ell in P.CASES:
        for p in P.PERIODS:
            _, z, ells = P.workload(8, M, D, ell, p)
            assert len(np.unique(np.floor(z / p))) == 1  # within one period
            cond = np.linalg.cond(P.kernel(z, z, ells, 1.0, p) + P.JITTER * np.eye(M))
            print(f"D={D} M={M} p={p}: cond {cond:.4g} (worst existing {worst:.4g})")
            assert cond <= worst, (D, M, p, cond, worst)
            Phi = P.phi_f64(P.workload(300, M, D, ell, p)[0], z, ells, 1.0, p)[0]
            assert np.abs(Phi).max() <= 1.0


def test_the_kind_on_the_host():
    import agpl_amd as A
    from agpl_amd import _ffi
    from agpl_amd.sparse import kernel_kind

    hdr = open(os.path.join(ROOT, "include", "agpl_kernels.h")).read()
    assert "AGPL_KERNEL_PERIODIC = AGPL_KERNEL_RQ + 2" in hdr and _ffi.KERNEL_PERIODIC == P.KIND == K.RQ + 2
    assert kernel_kind(("periodic", 2.5)) == (6, 2.5) and kernel_kind(("rq", 2)) == (4, 2.0)
    for bad in (("periodic", 0.0), ("periodic", -1.0), ("periodic", float("nan")), ("periodic", float("inf")), ("periodic",), "periodic"):
        with pytest.raises(A.ArgumentError):
            A.Plan.from_inputs(None, None, 1.0, kernel=bad)
    with pytest.raises(A.ArgumentError, match="period"):
        kernel_kind(("periodic", 0.0))
    with pytest.raises(A.ArgumentError, match="lengthscale"):
        A.spectral_frequencies(("periodic", 1.0), 8, 1, device="cpu")
    with pytest.raises(A.AGPLError, match="select_inducing_greedy") as e:
        A.select_inducing(None, 4, kernel=("periodic", 1.0))
    assert e.value.code == _ffi.ERR_UNSUPPORTED
    om, ph = A.spectral_frequencies(("periodic", 2.5), 64, 2, device="cpu", lengthscale=[0.3, 0.5])
    k = om.numpy() * 2.5 / (2 * np.pi * np.array([0.3, 0.5]))
    assert np.abs(k - np.round(k)).max() < 1e-12 and np.abs(k).max() >= 1


@pytest.mark.parametrize("D,p", [(1, 1.0), (3, 2.5)])
def test_greedy_inputs_have_clear_pivot_margins(D, p):
    """The inputs of tests/test_gpu_periodic.py's greedy test: every pick after the first (a tie by construction, resolved to the lowest
    index) beats the runner-up by more than GREEDY_MARGIN s2."""
    x, ells = P.greedy_inputs(D, p)
    piv, margins = P.greedy_pivots(x, P.GREEDY_M, ells, 1.0, p)
    print(f"D={D} p={p}: pivots {piv.tolist()} margins {np.array2string(margins, precision=2)}")
    assert piv[0] == 0 and len(set(piv.tolist())) == P.GREEDY_M and (margins > P.GREEDY_MARGIN).all()


def test_bound_gradients_analytic_against_autograd():
    """The analytic gradients of the sweep's bound (the rule's u and u' in closed form) against autograd through the whole bound, with
    an inducing input at delta = p / 2 from a point."""
    import hyper_reference as HR

    p, M, N, D = 2.5, 16, 60, 3
    x, z, ells = P.workload(N, M, D, 0.3, p)
    z[1] = x[0] + p / 2
    m, S, beta, gamma = HR.synthetic_q(M, 1, N, 3)[:4]
    g = P.bound_gradients(x, z, ells, 1.3, p, 1e-6, m, S, beta, gamma)
    assert np.abs(g["theta"] - g["auto_theta"]).max() <= 1e-10 * g["scale_theta"].max()
    assert np.abs(g["z"] - g["auto_z"]).max() <= 1e-10 * g["scale_z"].max()
    assert np.abs(g["auto_z"]).max() > 0 and np.abs(g["auto_theta"]).max() > 0


@pytest.mark.parametrize("source,names", [("agpl_kernels.hip", ["se_build_periodic_kernelILb0E"]),
                                          ("agpl_grad.hip", ["se_build_periodic_kernelILb1E"]),
                                          ("agpl_joint.hip", ["joint_cov_periodic_kernel"])])
def test_periodic_instantiations_keep_two_workgroups_per_cu(tmp_path, source, names):
    """What tests/test_kernels_cpu.py asserts of every se_build_kernel<kind>, for the periodic kernels (their own names): no private
    segment, no spilled VGPR, at most 256 VGPRs (two 256-thread workgroups per CU), the product on the matrix cores."""
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
