"""Build-time guard on the gather kernel (CPU test: reads the notes of the gfx950 code objects of csrc/rt_gather.o and csrc/rt_soft.o,
the way tests/test_ambient_resources.py reads the ambient kernels').  The unit holds exactly one kernel, rt_gather_kernel: workgroups of
256, no LDS, no spilled register, and a per-lane stack in scratch memory no larger than rt_soft_trace's - the same tree walk
(csrc/rt_soft_walk.h) keeps it -, whose figure is read from rt_soft.o here and not typed in.  The registers of both kernels are printed
and recorded in docs/EVIDENCE.md ("Gathered light"); no bound is put on them."""
import os
import re
import subprocess

import pytest

from test_kernel_resources import CSRC, TOOLS

pytestmark = pytest.mark.skipif(not all(os.path.exists(t) for t in TOOLS), reason="ROCm LLVM tools not installed")


def kernels_of(obj, tmp_path):
    fat, co = tmp_path / (obj + ".bin"), tmp_path / (obj + ".co")
    subprocess.run([TOOLS[0], "--dump-section", ".hip_fatbin=%s" % fat, os.path.join(CSRC, obj)], check=True)
    subprocess.run([TOOLS[1], "--unbundle", "--type=o", "--input=%s" % fat, "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", "--output=%s" % co], check=True)
    text = subprocess.run([TOOLS[2], "--notes", str(co)], check=True, capture_output=True, text=True).stdout
    kernels = {}
    for block in re.split(r"\n\s+- \.agpr_count:", text)[1:]:
        f = dict(re.findall(r"\.(name|vgpr_count|sgpr_count|vgpr_spill_count|sgpr_spill_count|private_segment_fixed_size|"
                            r"group_segment_fixed_size|max_flat_workgroup_size):\s+(\S+)", block))
        kernels[f["name"]] = {x: int(v) for x, v in f.items() if x != "name"}
    return kernels


def test_the_gather_kernel_spills_nothing_uses_no_lds_and_keeps_the_soft_kernels_stack(built, tmp_path):
    gather, soft = kernels_of("rt_gather.o", tmp_path), kernels_of("rt_soft.o", tmp_path)
    assert len(gather) == 1 and re.search(r"\d+rt_gather_kernel", next(iter(gather))), sorted(gather)
    assert len(soft) == 1 and re.search(r"\d+rt_soft_trace", next(iter(soft))), sorted(soft)
    (name, r), (soft_name, s) = next(iter(gather.items())), next(iter(soft.items()))
    for k, v in ((name, r), (soft_name, s)):
        print("GATHER resources %s: %d VGPRs, %d SGPRs, %d B LDS, %d B scratch" % (k, v["vgpr_count"], v["sgpr_count"], v["group_segment_fixed_size"],
                                                                                  v["private_segment_fixed_size"]))
    assert r["max_flat_workgroup_size"] == 256
    assert r["group_segment_fixed_size"] == 0
    assert r["vgpr_spill_count"] == 0 and r["sgpr_spill_count"] == 0, r
    assert 0 < r["private_segment_fixed_size"] <= s["private_segment_fixed_size"], (r, s)
