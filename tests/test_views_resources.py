"""Build-time guard on the view generator (CPU test: reads the notes of the gfx950 code object of csrc/rt_views.o, the way
tests/test_texels_resources.py reads the texel blit's).  rt_view_rays_kernel is one ray per work-item, a few dozen FP64 operations and
three 16-byte stores: no scratch memory, no spilled register, no LDS, workgroups of 256.  Its register counts are recorded in
docs/EVIDENCE.md ("Views"); no bound is put on them."""
import os
import re
import subprocess

import pytest

from test_kernel_resources import CSRC, TOOLS

pytestmark = pytest.mark.skipif(not all(os.path.exists(t) for t in TOOLS), reason="ROCm LLVM tools not installed")


def test_the_view_generator_uses_no_scratch_and_spills_nothing(built, tmp_path):
    fat, co = tmp_path / "v.bin", tmp_path / "v.co"
    subprocess.run([TOOLS[0], "--dump-section", ".hip_fatbin=%s" % fat, os.path.join(CSRC, "rt_views.o")], check=True)
    subprocess.run([TOOLS[1], "--unbundle", "--type=o", "--input=%s" % fat, "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", "--output=%s" % co], check=True)
    text = subprocess.run([TOOLS[2], "--notes", str(co)], check=True, capture_output=True, text=True).stdout
    kernels = {}
    for block in re.split(r"\n\s+- \.agpr_count:", text)[1:]:
        f = dict(re.findall(r"\.(name|vgpr_count|sgpr_count|vgpr_spill_count|sgpr_spill_count|private_segment_fixed_size|"
                            r"group_segment_fixed_size|max_flat_workgroup_size):\s+(\S+)", block))
        kernels[f["name"]] = {x: int(v) for x, v in f.items() if x != "name"}
    assert len(kernels) == 1 and re.search(r"\d+rt_view_rays_kernel", next(iter(kernels))), sorted(kernels)
    r = next(iter(kernels.values()))
    print("VIEWS resources rt_view_rays_kernel: %d VGPRs, %d SGPRs, %d B LDS, %d B scratch" % (r["vgpr_count"], r["sgpr_count"], r["group_segment_fixed_size"],
                                                                                         r["private_segment_fixed_size"]))
    assert r["private_segment_fixed_size"] == 0 and r["vgpr_spill_count"] == 0 and r["sgpr_spill_count"] == 0, r
    assert r["group_segment_fixed_size"] == 0
    assert r["max_flat_workgroup_size"] == 256
