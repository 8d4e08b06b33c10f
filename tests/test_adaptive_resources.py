"""Build-time guard on the adaptive-supersampling kernels (CPU test: reads the gfx950 code object of csrc/rt_adaptive.o, the way
tests/test_nodes_resources.py reads the wavefront kernels').  rt_adaptive_mark is integer work on loaded dwords: no scratch memory, no
spill.  rt_adaptive_refine<REFRACT, K> is rt_retrace's trace with another way of finding its samples: it spills nothing, and its
reflection-only forms need no more private memory than rt_retrace<false, *> (the explicit recursion stack of the strict arithmetic)."""
import os
import re
import subprocess

import pytest

from test_kernel_resources import CSRC, TOOLS

pytestmark = pytest.mark.skipif(not all(os.path.exists(t) for t in TOOLS), reason="ROCm LLVM tools not installed")
FIELDS = r"\.(name|vgpr_count|sgpr_count|vgpr_spill_count|sgpr_spill_count|private_segment_fixed_size|group_segment_fixed_size|max_flat_workgroup_size):\s+(\S+)"


def notes_by_name(obj, tmp_path, pattern):
    """{groups of `pattern` in the kernel's mangled name: its resource notes} for the kernels of `obj` whose name matches"""
    fat, co = tmp_path / (os.path.basename(obj) + ".bin"), tmp_path / (os.path.basename(obj) + ".co")
    subprocess.run([TOOLS[0], "--dump-section", ".hip_fatbin=%s" % fat, obj], check=True)
    subprocess.run([TOOLS[1], "--unbundle", "--type=o", "--input=%s" % fat, "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", "--output=%s" % co], check=True)
    text = subprocess.run([TOOLS[2], "--notes", str(co)], check=True, capture_output=True, text=True).stdout
    out = {}
    for block in re.split(r"\n\s+- \.agpr_count:", text)[1:]:
        f = dict(re.findall(FIELDS, block))
        m = re.search(pattern, f.get("name", ""))
        if m:
            out[m.groups()] = {x: int(v) for x, v in f.items() if x != "name"}
    return out


def test_adaptive_kernels_spill_nothing_and_keep_to_retrace_scratch(built, tmp_path):
    obj = os.path.join(CSRC, "rt_adaptive.o")
    mark = notes_by_name(obj, tmp_path, r"\d+(rt_adaptive_mark)E")
    assert list(mark) == [("rt_adaptive_mark",)]
    refine = notes_by_name(obj, tmp_path, r"rt_adaptive_refineILb([01])ELj([234])E")
    assert sorted(refine) == [(r, k) for r in "01" for k in "234"]
    retrace = notes_by_name(os.path.join(CSRC, "rt_kernel_strict.o"), tmp_path, r"rt_retraceILb([01])ELb([01])E")
    assert sorted(retrace) == [(r, s) for r in "01" for s in "01"]
    for name, r in list(mark.items()) + sorted(refine.items()) + sorted(retrace.items()):
        print("ADAPTIVE resources %s: %d VGPRs, %d SGPRs, %d B LDS, %d B scratch, spills %d v / %d s" % (
            "<%s>" % ", ".join(name), r["vgpr_count"], r["sgpr_count"], r["group_segment_fixed_size"], r["private_segment_fixed_size"],
            r["vgpr_spill_count"], r["sgpr_spill_count"]))
    m = mark[("rt_adaptive_mark",)]
    assert m["vgpr_spill_count"] == 0 and m["sgpr_spill_count"] == 0 and m["private_segment_fixed_size"] == 0 and m["group_segment_fixed_size"] == 0, m
    assert m["max_flat_workgroup_size"] == 256
    retrace_private = max(r["private_segment_fixed_size"] for (refract, _), r in retrace.items() if refract == "0")
    for (refract, k), r in refine.items():
        assert r["vgpr_spill_count"] == 0, (refract, k, r)
        assert r["group_segment_fixed_size"] == 0, (refract, k, r)           # the bytes are summed with cross-lane operations: no LDS
        assert r["max_flat_workgroup_size"] == 256
        if refract == "0":
            assert r["private_segment_fixed_size"] <= retrace_private, (refract, k, r, retrace_private)
