"""Build-time guard on the wavefront kernels (CPU test: reads the gfx950 code object of csrc/rt_nodes.o, the way
tests/test_kernel_resources.py reads the trace kernels').  The point of the level-by-level form is that one level of intersectWorld needs
no stack: the shade, spawn and fold kernels use no scratch memory and spill no register (the recursive rt_trace_rays<true> reserves
3 472 bytes per lane).  Their register counts are recorded in docs/EVIDENCE.md ("Wavefront ray lists"); no bound is put on them."""
import os
import re
import subprocess

import pytest

from test_kernel_resources import CSRC, TOOLS

pytestmark = pytest.mark.skipif(not all(os.path.exists(t) for t in TOOLS), reason="ROCm LLVM tools not installed")
KERNELS = ("rt_nodes_shade", "rt_nodes_spawn_count", "rt_nodes_spawn_scan", "rt_nodes_spawn_scatter", "rt_nodes_fold")


def node_kernel_notes(obj, tmp_path):
    fat, co = tmp_path / "n.bin", tmp_path / "n.co"
    subprocess.run([TOOLS[0], "--dump-section", ".hip_fatbin=%s" % fat, obj], check=True)
    subprocess.run([TOOLS[1], "--unbundle", "--type=o", "--input=%s" % fat, "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", "--output=%s" % co], check=True)
    text = subprocess.run([TOOLS[2], "--notes", str(co)], check=True, capture_output=True, text=True).stdout
    out = {}
    for block in re.split(r"\n\s+- \.agpr_count:", text)[1:]:
        f = dict(re.findall(r"\.(name|vgpr_count|sgpr_count|vgpr_spill_count|sgpr_spill_count|private_segment_fixed_size|"
                            r"group_segment_fixed_size|max_flat_workgroup_size):\s+(\S+)", block))
        for k in KERNELS:
            if re.search(r"\d+%sE" % k, f.get("name", "")):
                out[k] = {x: int(v) for x, v in f.items() if x != "name"}
    return out


def test_node_kernels_use_no_scratch_and_spill_nothing(built, tmp_path):
    k = node_kernel_notes(os.path.join(CSRC, "rt_nodes.o"), tmp_path)
    assert sorted(k) == sorted(KERNELS)
    for name, r in k.items():
        print("NODES resources %s: %d VGPRs, %d SGPRs, %d B LDS, %d B scratch" % (name, r["vgpr_count"], r["sgpr_count"], r["group_segment_fixed_size"],
                                                                                 r["private_segment_fixed_size"]))
        assert r["private_segment_fixed_size"] == 0 and r["vgpr_spill_count"] == 0 and r["sgpr_spill_count"] == 0, (name, r)
        assert r["max_flat_workgroup_size"] == 256
