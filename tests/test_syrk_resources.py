"""Register budget of the accumulation kernel (agpl_syrk.hip, syrk_strip_kernel), from the compiler's own resource report of a
gfx950 cross-compile (no GPU needed): two 512-thread workgroups' worth of waves per SIMD leave 256 VGPRs per lane, and the step
loops hold 128 accumulator registers -- a spilled register there means scratch traffic beside the hand-counted `vmcnt` waits.
The balanced column-block map of the diagonal tiles brought the kernel from 256 VGPRs with 4 spilled (20 bytes of private segment)
to no spill at all; this keeps it there."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "augmentedgplikelihoods.jl_amd", "csrc")
HIPCC = "/opt/rocm/bin/hipcc"


def test_syrk_strip_kernel_spills_nothing(tmp_path):
    if not os.path.exists(HIPCC):
        pytest.skip("no hipcc")
    flags = re.search(r"^COMMON\s*:=\s*(.*)$", open(os.path.join(CSRC, "Makefile")).read(), flags=re.M).group(1)
    flags = flags.replace("$(ARCH)", "gfx950").split()
    p = subprocess.run([HIPCC] + flags + ["--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", "-c",
                                          os.path.join(CSRC, "agpl_syrk.hip"), "-o", "syrk.o"],
                       cwd=tmp_path, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, check=True)
    blocks = re.split(r"remark: Function Name: ", p.stdout)[1:]
    mine = [b for b in blocks if "syrk_strip_kernel" in b.splitlines()[0]]
    assert len(mine) == 1, [b.splitlines()[0] for b in blocks]

    def field(name):
        return int(re.search(r"remark:\s+" + re.escape(name) + r":\s+(\d+)", mine[0]).group(1))

    print("VGPRs", field("VGPRs"), "VGPRs Spill", field("VGPRs Spill"), "ScratchSize", field("ScratchSize [bytes/lane]"))
    assert field("VGPRs Spill") == 0
    assert field("ScratchSize [bytes/lane]") == 0  # = the private segment
    assert field("VGPRs") <= 256
