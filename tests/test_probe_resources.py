"""Build-time guard on the probe kernel (CPU test: reads the notes of the gfx950 code objects of csrc/rt_probe.o and csrc/rt_soft.o, the
way tests/test_gather_resources.py reads the gather kernel's).  The unit holds exactly one kernel, rt_probe_kernel: workgroups of at most
the CAP its header comment names, no spilled register, no STATIC LDS (the colours' slots are dynamic: 24 n_samples bytes per launch), and
a per-lane stack in scratch memory no larger than rt_soft_trace's - the same tree walk (csrc/rt_soft_walk.h) keeps it -, whose figure is
read from rt_soft.o here and not typed in.  The registers are printed and recorded in docs/EVIDENCE.md ("Probes"); no bound is put on
them."""
import os
import re

import pytest

from test_gather_resources import kernels_of
from test_kernel_resources import CSRC, TOOLS

pytestmark = pytest.mark.skipif(not all(os.path.exists(t) for t in TOOLS), reason="ROCm LLVM tools not installed")


def test_the_probe_kernel_spills_nothing_has_no_static_lds_and_keeps_the_soft_kernels_stack(built, tmp_path):
    probe, soft = kernels_of("rt_probe.o", tmp_path), kernels_of("rt_soft.o", tmp_path)
    assert len(probe) == 1 and re.search(r"\d+rt_probe_kernel", next(iter(probe))), sorted(probe)
    assert len(soft) == 1 and re.search(r"\d+rt_soft_trace", next(iter(soft))), sorted(soft)
    (name, r), (soft_name, s) = next(iter(probe.items())), next(iter(soft.items()))
    for k, v in ((name, r), (soft_name, s)):
        print("PROBE resources %s: %d VGPRs, %d SGPRs, %d B LDS, %d B scratch" % (k, v["vgpr_count"], v["sgpr_count"], v["group_segment_fixed_size"],
                                                                                 v["private_segment_fixed_size"]))
    # the CAP the kernel's header comment names, and the header's constant
    comment = open(os.path.join(CSRC, "rt_probe.hip")).read().split("#include", 1)[0]
    named = re.search(r"CAP is (\d+)", comment)
    define = re.search(r"#define RT_PROBE_CAP (\d+)u", open(os.path.join(CSRC, "rt_probe.h")).read())
    assert named and define and int(named.group(1)) == int(define.group(1))
    assert r["max_flat_workgroup_size"] == int(named.group(1))
    assert r["group_segment_fixed_size"] == 0
    assert r["vgpr_spill_count"] == 0 and r["sgpr_spill_count"] == 0, r
    assert 0 < r["private_segment_fixed_size"] <= s["private_segment_fixed_size"], (r, s)
