"""How many workgroups of its trace kernel a compute unit holds, by the HIP runtime's own count for the kernel's registers and the
launch's dynamic LDS (include/rt_hip.h: rt_scene_trace_occupancy - nothing is launched, the test takes milliseconds).  Six waves per SIMD
for the few-sphere one-wave kernels are 24 one-wave workgroups per CU: both the 80 VGPRs (tests/test_six_wave_resources.py) and the
6 400 bytes of LDS for eight spheres (csrc/rt_launch.hip: lds_for) have to admit them.  The launches this change leaves alone - the
four-wave form of the first frame, default14's general kernel - report what the parent commit's library reported, recorded with the
parent's source plus this one entry point (docs/EVIDENCE.md, "Six waves per SIMD")."""
import pytest

import rt_host
from test_gpu_prologue_loads import plib  # noqa: F401  (fixture: the product library)

pytestmark = pytest.mark.gpu

# (workgroups per CU, dynamic LDS bytes) by the parent commit's library: h8's first frame (four-wave workgroups) and default14
PARENT = {
    ("h8", True): (5, 22272),
    ("default14", False): (5, 29120),
    ("default14", True): (5, 29120),
}


def occupancy(lib, scene_name, four_waves):
    r = rt_host.Renderer(rt_host.flatten_scene(rt_host.load_scene(scene_name)), 0, lib)
    try:
        return r.trace_occupancy(four_waves)
    finally:
        r.close()


def test_h8_second_frame_holds_24_one_wave_workgroups(plib):  # noqa: F811
    n, lds = occupancy(plib, "h8", False)
    print("h8, one-wave workgroups: %d per CU, %d bytes of LDS each" % (n, lds))
    assert lds == 8 * 160 + 10 * 64 * 8          # eight material records and ten doubles of fold state per lane
    assert n >= 24, (n, lds)


@pytest.mark.parametrize("scene,four_waves", [("h8", True), ("default14", False), ("default14", True)])
def test_untouched_launches_report_the_parents_count(plib, scene, four_waves):  # noqa: F811
    got = occupancy(plib, scene, four_waves)
    print(scene, "four_waves" if four_waves else "steady", got)
    assert got == PARENT[(scene, four_waves)]
