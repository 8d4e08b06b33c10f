"""Build-time guard on the relight kernel (CPU test: reads the notes of the gfx950 code object of csrc/rt_relight.o, the way
tests/test_lighting_resources.py reads the sampled lights').  The unit holds exactly one kernel, rt_relight_kernel: no scratch memory,
no spilled register, no LDS, workgroups of 256.  Its register counts are printed here and recorded in docs/EVIDENCE.md ("Relit
nodes"); no bound is put on them."""
import os
import re
import subprocess

import pytest

from test_kernel_resources import CSRC, TOOLS

pytestmark = pytest.mark.skipif(not all(os.path.exists(t) for t in TOOLS), reason="ROCm LLVM tools not installed")

KERNELS = ["rt_relight_kernel"]


def test_the_relight_kernel_uses_no_scratch_no_lds_and_spills_nothing(built, tmp_path):
    fat, co = tmp_path / "a.bin", tmp_path / "a.co"
    subprocess.run([TOOLS[0], "--dump-section", ".hip_fatbin=%s" % fat, os.path.join(CSRC, "rt_relight.o")], check=True)
    subprocess.run([TOOLS[1], "--unbundle", "--type=o", "--input=%s" % fat, "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", "--output=%s" % co], check=True)
    text = subprocess.run([TOOLS[2], "--notes", str(co)], check=True, capture_output=True, text=True).stdout
    kernels = {}
    for block in re.split(r"\n\s+- \.agpr_count:", text)[1:]:
        f = dict(re.findall(r"\.(name|vgpr_count|sgpr_count|vgpr_spill_count|sgpr_spill_count|private_segment_fixed_size|"
                            r"group_segment_fixed_size|max_flat_workgroup_size):\s+(\S+)", block))
        kernels[f["name"]] = {x: int(v) for x, v in f.items() if x != "name"}
    assert len(kernels) == 1, sorted(kernels)
    assert sorted(re.search(r"\d+(rt_relight_\w*?kernel)", k).group(1) for k in kernels) == KERNELS, sorted(kernels)
    for name, r in sorted(kernels.items()):
        print("RELIGHT resources %s: %d VGPRs, %d SGPRs, %d B LDS, %d B scratch" % (name, r["vgpr_count"], r["sgpr_count"], r["group_segment_fixed_size"],
                                                                                   r["private_segment_fixed_size"]))
        assert r["private_segment_fixed_size"] == 0 and r["vgpr_spill_count"] == 0 and r["sgpr_spill_count"] == 0, (name, r)
        assert r["group_segment_fixed_size"] == 0, name
        assert r["max_flat_workgroup_size"] == 256, name
