"""tests/split_reference.py held against itself and against the sources, without a GPU: on the data of every case of
tests/test_gpu_split_planes.py the numpy model of each contraction stays under half of its element-wise bars, every named wrong
variant -- restricted to one seam position / one stage -- leaves them, and the cross terms are visible (>= 4 bars) at every seam.
The seam constants are read from the sources: a step, ring, slice or stage size that moves fails here, instead of the GPU cases
quietly testing another place.

Measured here (max |model - float64| / bar; smallest |variant - float64| / bar over the cases and places):
    accumulation  model G <= 0.071, g <= 0.229;  A_lo_dropped 33.5, B_lo_dropped 45.9, lo_hi_from_wrong_operand 70.2,
                  truncated_hi_no_lo 135, stale_gamma 5.3e4
    marginal pass model mu, var, c <= 0.026 (banded), <= 0.007 (dense);  the banded cases, one stage: U_lo_dropped 31.4, Phi_lo_dropped
                  15.7, lo_hi_from_wrong_operand 15.7, truncated_hi_no_lo 47, stage_planes_dropped 47 (of var); the dense case, every stage
                  at once: U_lo_dropped 10.8, Phi_lo_dropped 5.4, lo_hi_from_wrong_operand 5.4, truncated 16.1, planes 16.1 (of var)
REQUIRED below is half of the smallest figure of a variant, never below 4.  Pairs that are dropped:
    * stale_gamma at the first step of a slice (there is no previous step whose record the slot could still hold);
    * every one-stage variant on the dense case (one stage is a sixteenth of each sum there: 0.3 .. 2.6 bars) -- the dense case takes
      the variants in every stage at once, which is what it is for."""
import subprocess

import numpy as np
import pytest

import split_reference as SR

REQUIRED_ACC = {"A_lo_dropped": 16.0, "B_lo_dropped": 22.0, "lo_hi_from_wrong_operand": 35.0, "truncated_hi_no_lo": 65.0, "stale_gamma": 2.5e4}
REQUIRED_MARG = {"U_lo_dropped": 15.0, "Phi_lo_dropped": 7.5, "lo_hi_from_wrong_operand": 7.5, "truncated_hi_no_lo": 23.0,
                 "stage_planes_dropped": 23.0}
REQUIRED_MARG_DENSE = {"U_lo_dropped": 5.4, "Phi_lo_dropped": 4.0, "lo_hi_from_wrong_operand": 4.0, "truncated_hi_no_lo": 8.0,
                       "stage_planes_dropped": 8.0}


def test_the_seam_constants_are_what_the_shapes_were_chosen_for():
    assert SR.constants() == SR.EXPECTED
    c = SR.constants()
    assert (SR.STEP, SR.RING, SR.PANEL) == (c["kStagePts"], c["kRing"], c["kPanel"])
    assert SR.STAGE == c["KS"] * c["KU"] and SR.TILE == c["NT2"]


def test_the_slice_plan_is_the_header_s(tmp_path):
    """slice_plan against agpl_slices.h itself, compiled with g++, on the accumulation cases."""
    src = tmp_path / "plan.cpp"
    calls = "".join(f"  show({c.N}, {SR.R.plan_padded(c.M)}, {c.L});\n" for c in SR.ACC_CASES)
    src.write_text('#include <stdio.h>\n#include "agpl_slices.h"\nstatic void show(int64_t N, int M, int L) {\n'
                   "  const agpl_slices p = agpl_slice_plan(N, M, L);\n  printf(\"%d\", p.nbig);\n"
                   "  for (int s = 0; s < p.ns; ++s) { int64_t b, e; agpl_slice_range(s, p.chunk, p.nbig, p.small, N, b, e); "
                   'printf(" %lld:%lld", (long long)b, (long long)e); }\n  printf("\\n");\n}\nint main() {\n' + calls + "  return 0;\n}\n")
    exe = tmp_path / "plan"
    subprocess.run(["g++", "-O1", "-std=c++17", "-I", SR.S.CSRC, str(src), "-o", str(exe)], check=True)
    lines = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines()
    for c, line in zip(SR.ACC_CASES, lines):
        sl, nbig = SR.slice_plan(*c)
        assert line == str(nbig) + "".join(f" {b}:{e}" for b, e in sl), c.id


def test_the_accumulation_cases_reach_their_seams():
    names = {c.id: [n for n, _ in SR.seam_positions(*c)] for c in SR.ACC_CASES}
    assert names["N33-M512-L1"] == ["first step", "ring slot 1"]  # (its second step is the ragged last one)
    for cid in ("N4097-M512-L1", "N9011-M1024-L1", "N9011-M768-L2", "N5003-M300-L1", "N352257-M512-L1"):
        assert {"first step", "ring slot 1", "ring slot 2", "ring slot 3", "ring wrapped", "last step of slice 0", "first step of slice 1",
                "last full step", "ragged last step", "inside a fine slice"} <= set(names[cid]), cid
    assert "inside a big slice" in names["N352257-M512-L1"]
    sl, nbig = SR.slice_plan(352257, 512, 1)
    assert nbig == 1 and sl[0] == (0, 4096) and sl[-1][1] - sl[-1][0] == 1  # one big slice, a ragged fine tail
    for c in SR.ACC_CASES:
        d = SR.acc_data(c)
        T = len(d.positions)
        for j, (pts, feats) in enumerate(d.bands):
            assert 1 <= pts.size <= 4 and pts[0] // SR.STEP == pts[-1] // SR.STEP == d.positions[j][1] // SR.STEP and pts[-1] < c.N
            assert np.all(feats % T == j)
        nz = np.abs(d.Phi_nz[d.Phi_nz != 0])
        assert nz.max() / nz.min() <= 16.5 and d.e == 14
        for a in range(c.M):  # one sign per feature
            col = d.Phi_nz[:, a]
            assert np.all(col >= 0) or np.all(col <= 0)


@pytest.mark.parametrize("case", SR.ACC_CASES, ids=lambda c: c.id)
def test_accumulation_model_within_and_variants_outside_the_bars(case):
    d = SR.acc_data(case)
    gamma, beta = SR.standin_gamma_beta(d)
    Gr, gr = SR.acc_reference(d, gamma, beta)
    bG, bg = SR.acc_bars(d, gamma, beta)
    G, g = SR.acc_model(d, gamma, beta)
    rG, rg, vis = SR.ratio(G, Gr, bG), SR.ratio(g, gr, bg), SR.acc_visibility(d, gamma, bG)
    print(f"SPLIT_CPU acc {case.id} model/bar G {rG:.3f} g {rg:.3f}; smallest cross term / bar {vis:.1f}")
    assert rG <= 0.5 and rg <= 0.5 and vis >= 4.0
    T = len(d.positions)
    off = (np.arange(case.M)[:, None] - np.arange(case.M)[None, :]) % T != 0
    assert np.all(bG[:, off] == 0) and np.all(Gr[:, off] == 0) and np.all(G[:, off] == 0)  # exact zeros between the bands
    for v in SR.ACC_VARIANTS:
        rs = []
        for j in range(T):
            if SR.acc_can_touch(d, v, j):
                Gv, gv = SR.acc_model(d, gamma, beta, v, j)
                rs.append(max(SR.ratio(Gv, Gr, bG), SR.ratio(gv, gr, bg)))
        print(f"SPLIT_CPU acc {case.id} {v} / bar: min {min(rs):.1f} max {max(rs):.1f} over {len(rs)} seam positions")
        assert len(rs) >= 1 and min(rs) >= REQUIRED_ACC[v] >= 4.0, (v, rs)


@pytest.mark.parametrize("case", SR.MARG_CASES, ids=lambda c: c.id)
def test_marginal_model_within_and_variants_outside_the_bars(case):
    d = SR.marg_data(case)
    N, M, L, kind = case
    v32 = d.v_int.astype(np.float32)
    for l in range(L):
        assert np.linalg.cond(d.U_int[l].T @ d.U_int[l]) < 1e6
        assert np.all(d.U_int[l][np.tril_indices(M)] > 0) and np.all(np.triu(d.U_int[l], 1) == 0)
        assert np.linalg.norm(d.U_int[l], 2) < 1.0  # I + G >= I: what an update can produce
    assert np.all(d.Phi >= 0)
    live = np.arange(M)[None, :] // SR.STAGE == d.stage_of[:, None]
    assert np.all((d.Phi != 0) == (live if kind == "banded" else np.ones_like(live)))
    nst = SR.S.cdiv(M, SR.STAGE)
    for t0 in range(0, N, SR.TILE):  # every live stage inside every tile that has the points for it
        assert set(d.stage_of[t0: t0 + SR.TILE]) == set(range(min(nst, N - t0)))
    ref = SR.marg_reference(d, d.U_int, v32)
    bars = SR.marg_bars(d, d.U_int, v32, ref)
    m = SR.marg_model(d, d.U_int, v32)
    r = [SR.ratio(m.mu, ref.mu, bars.mu), SR.ratio(m.var, ref.var, bars.var), SR.ratio(m.c, ref.c, bars.c)]
    vis = SR.marg_visibility(d, d.U_int, bars, whole=kind == "dense")
    print(f"SPLIT_CPU marg {case.id} model/bar mu {r[0]:.3f} var {r[1]:.3f} c {r[2]:.3f}; smallest cross term / bar {vis:.1f}")
    assert max(r) <= 0.5 and vis >= 4.0
    places = [SR.ALL] if kind == "dense" else sorted({0, 1, nst // 2, nst - 1})
    need = REQUIRED_MARG_DENSE if kind == "dense" else REQUIRED_MARG
    for v in SR.MARG_VARIANTS:
        rs = []
        for k in places:
            mv = SR.marg_model(d, d.U_int, v32, v, k)
            rs.append(SR.ratio(mv.var, ref.var, bars.var))
            if kind == "banded":  # (the dense case is judged by var: its mu and c see a lost Phi lo plane at 2.7 .. 5 bars)
                assert SR.ratio(mv.mu, ref.mu, bars.mu) >= 4.0 and SR.ratio(mv.c, ref.c, bars.c) >= 4.0, (v, k)
        print(f"SPLIT_CPU marg {case.id} {v} / bar of var: min {min(rs):.1f} max {max(rs):.1f} over stages {places}")
        assert min(rs) >= need[v] >= 4.0, (v, rs)
