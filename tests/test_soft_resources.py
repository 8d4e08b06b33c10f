"""Build-time guard on the soft trace kernel (CPU test: reads the notes of the gfx950 code object of csrc/rt_soft.o, the way
tests/test_relight_resources.py reads the relight kernel's).  The unit holds exactly one kernel, rt_soft_trace: no spilled register,
workgroups of 256, and a per-lane stack in scratch memory that stays at or below the 3 472 B the recursive rt_trace_rays<true>
reserves.  Its registers, scratch and LDS are printed here and recorded in docs/EVIDENCE.md ("Soft trace in one launch"); no bound is
put on the registers."""
import os
import re
import subprocess

import pytest

from test_kernel_resources import CSRC, TOOLS

pytestmark = pytest.mark.skipif(not all(os.path.exists(t) for t in TOOLS), reason="ROCm LLVM tools not installed")

KERNELS = ["rt_soft_trace"]
SCRATCH_CEILING = 3472


def test_the_soft_kernel_spills_nothing_and_keeps_its_stack_below_the_recursive_kernels(built, tmp_path):
    fat, co = tmp_path / "a.bin", tmp_path / "a.co"
    subprocess.run([TOOLS[0], "--dump-section", ".hip_fatbin=%s" % fat, os.path.join(CSRC, "rt_soft.o")], check=True)
    subprocess.run([TOOLS[1], "--unbundle", "--type=o", "--input=%s" % fat, "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", "--output=%s" % co], check=True)
    text = subprocess.run([TOOLS[2], "--notes", str(co)], check=True, capture_output=True, text=True).stdout
    kernels = {}
    for block in re.split(r"\n\s+- \.agpr_count:", text)[1:]:
        f = dict(re.findall(r"\.(name|vgpr_count|sgpr_count|vgpr_spill_count|sgpr_spill_count|private_segment_fixed_size|"
                            r"group_segment_fixed_size|max_flat_workgroup_size):\s+(\S+)", block))
        kernels[f["name"]] = {x: int(v) for x, v in f.items() if x != "name"}
    assert len(kernels) == 1, sorted(kernels)
    assert sorted(re.search(r"\d+(rt_soft_trace)", k).group(1) for k in kernels) == KERNELS, sorted(kernels)
    for name, r in sorted(kernels.items()):
        print("SOFT resources %s: %d VGPRs, %d SGPRs, %d B LDS, %d B scratch" % (name, r["vgpr_count"], r["sgpr_count"], r["group_segment_fixed_size"],
                                                                                r["private_segment_fixed_size"]))
        assert r["vgpr_spill_count"] == 0 and r["sgpr_spill_count"] == 0, (name, r)
        assert r["max_flat_workgroup_size"] == 256, name
        assert 0 < r["private_segment_fixed_size"] <= SCRATCH_CEILING, (name, r)
