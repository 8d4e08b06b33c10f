"""Build-time guard on the texel blit (CPU test: reads the notes of the gfx950 code object of csrc/rt_texels.o, the way
tests/test_nodes_resources.py reads the node kernels').  rt_texels_blit is a copy of one dword per work-item: no scratch memory, no
spilled register, workgroups of 256.  Its register counts are recorded in docs/EVIDENCE.md ("Texel edits"); no bound is put on them."""
import os
import re
import subprocess

import pytest

from test_kernel_resources import CSRC, TOOLS

pytestmark = pytest.mark.skipif(not all(os.path.exists(t) for t in TOOLS), reason="ROCm LLVM tools not installed")


def test_the_texel_blit_uses_no_scratch_and_spills_nothing(built, tmp_path):
    fat, co = tmp_path / "t.bin", tmp_path / "t.co"
    subprocess.run([TOOLS[0], "--dump-section", ".hip_fatbin=%s" % fat, os.path.join(CSRC, "rt_texels.o")], check=True)
    subprocess.run([TOOLS[1], "--unbundle", "--type=o", "--input=%s" % fat, "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", "--output=%s" % co], check=True)
    text = subprocess.run([TOOLS[2], "--notes", str(co)], check=True, capture_output=True, text=True).stdout
    kernels = {}
    for block in re.split(r"\n\s+- \.agpr_count:", text)[1:]:
        f = dict(re.findall(r"\.(name|vgpr_count|sgpr_count|vgpr_spill_count|sgpr_spill_count|private_segment_fixed_size|"
                            r"group_segment_fixed_size|max_flat_workgroup_size):\s+(\S+)", block))
        kernels[f["name"]] = {x: int(v) for x, v in f.items() if x != "name"}
    assert len(kernels) == 1 and re.search(r"\d+rt_texels_blit", next(iter(kernels))), sorted(kernels)
    r = next(iter(kernels.values()))
    print("TEXELS resources rt_texels_blit: %d VGPRs, %d SGPRs, %d B LDS, %d B scratch" % (r["vgpr_count"], r["sgpr_count"], r["group_segment_fixed_size"],
                                                                                      r["private_segment_fixed_size"]))
    assert r["private_segment_fixed_size"] == 0 and r["vgpr_spill_count"] == 0 and r["sgpr_spill_count"] == 0, r
    assert r["max_flat_workgroup_size"] == 256
