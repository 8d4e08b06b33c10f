"""Second-node bits on the GPU (rt_kernel_trace.h: the first-bounce walk): a wave of the few-sphere reflection-only product kernels
whose launch-table entry carries SELF bits (rt_block.h: rt_second_node_bits) leaves the named mirrors out of its first-bounce walk.
(SKY and the DARK bits are read by no kernel: docs/EVIDENCE.md.)  Every frame must be BYTE FOR BYTE what the kernel stores when it
ignores the bits - the test library's RT_NO_SECOND_NODE - with as many samples marked for the exact launch (rt_stats.exact_samples).
rt_test_second_node_waves counts the waves that left a candidate out, so that no comparison is vacuous: above 0, at most four per
entry with such a bit, and 0 with the switch.  Each frame is rendered twice: a camera's first frame runs the four-wave form of the
kernel, the second the one-wave form; both read the bits."""
import copy
import ctypes as C
import os

import pytest

import rt_host
from objects_util import fresh, gpu_table, host_table, tlib  # noqa: F401  (fixture: the test library)
from test_first_bounce import FIRST_BOUNCE, PLAIN, h8, reflecting_sky, stating, table, two_mirrors
from test_second_node import SECOND_NODE

pytestmark = pytest.mark.gpu

SWITCH = "RT_NO_SECOND_NODE"


@pytest.fixture(scope="module")
def lib(tlib):  # noqa: F811
    tlib.rt_test_second_node_waves.restype = C.c_int
    tlib.rt_test_second_node_waves.argtypes = [C.c_int, C.POINTER(C.c_ulonglong)]
    return tlib


def waves(lib):
    """Waves that left a candidate out of their first-bounce walk since the last call; drains the device."""
    a = C.c_ulonglong()
    assert lib.rt_test_second_node_waves(0, C.byref(a)) == 0, lib.rt_last_error()
    return a.value


def shot(lib, r, w, h):
    n = w * h * 4
    d = lib.rt_alloc_device(0, n)
    assert d, lib.rt_last_error()
    try:
        waves(lib)
        st = r.render_tiles(w, h, d, rt_host.RtTiles(h, 0, 1, 1), want_stats=True)
        took = waves(lib)
        host = C.create_string_buffer(n)
        assert lib.rt_copy_to_host(0, host, d, n) == 0, lib.rt_last_error()
    finally:
        lib.rt_free_device(0, d)
    return host.raw, int(st.exact_samples), took


def both(lib, scene, w, h, steps=()):
    """Per setting of the switch: a fresh upload, two frames (four-wave, one-wave), then per step - a callable that edits the resident
    scene - two more.  Returns the two lists of (frame, exact_samples, waves that left a candidate out)."""
    out = []
    for off in (False, True):
        if off:
            os.environ[SWITCH] = "1"
        try:
            r = rt_host.Renderer(rt_host.flatten_scene(scene), 0, lib)
            try:
                frames = [shot(lib, r, w, h), shot(lib, r, w, h)]
                for step in steps:
                    step(r)
                    frames += [shot(lib, r, w, h), shot(lib, r, w, h)]
            finally:
                r.close()
        finally:
            os.environ.pop(SWITCH, None)
        out.append(frames)
    return out


def same(on, off):
    assert len(on) == len(off)
    for k, (a, b) in enumerate(zip(on, off)):
        assert b[2] == 0, (k, b[2])
        assert a[1] == b[1], (k, a[1], b[1])
        assert a[0] == b[0], "frame %d differs" % k
    return [a[2] for a in on]


def host_entries(lib, scene, w, h):
    """Entries of the host table with a SELF bit."""
    rows = stating(table(lib, rt_host.flatten_scene(scene), w, h, SECOND_NODE))
    return int((((rows[:, 1] >> 24) & 3) != 0).sum()) if len(rows) else 0


def counted(lib, took, scene, w, h):
    """Both forms of the kernel acted on the bits: above 0, at most four waves per entry."""
    n = host_entries(lib, scene, w, h)
    assert n > 0 and all(0 < t <= 4 * n for t in took), (took, n)


@pytest.mark.parametrize("wh", [(1001, 563), (256, 144)])
def test_h8(lib, wh):
    s = h8()
    counted(lib, same(*both(lib, s, *wh)), s, *wh)


def test_h8_supersample_2(lib):
    s = h8(supersample=2)
    counted(lib, same(*both(lib, s, 500, 280)), s, 500, 280)


def test_two_mirrors_facing_each_other(lib):
    s = two_mirrors()
    counted(lib, same(*both(lib, s, 320, 180)), s, 320, 180)


def test_the_switch_of_the_sets_ignores_the_bits_too(lib):
    """RT_NO_FIRST_BOUNCE implies RT_NO_SECOND_NODE: no wave acts on a bit, and the frame is the same."""
    s = h8()
    on = both(lib, s, 256, 144)[0]
    os.environ["RT_NO_FIRST_BOUNCE"] = "1"
    try:
        r = rt_host.Renderer(rt_host.flatten_scene(s), 0, lib)
        try:
            off = [shot(lib, r, 256, 144), shot(lib, r, 256, 144)]
        finally:
            r.close()
    finally:
        os.environ.pop("RT_NO_FIRST_BOUNCE", None)
    same(on, off)


@pytest.mark.parametrize("name,wh,ss", [("h8", (1001, 563), 1), ("h8", (320, 184), 2), ("two_mirrors", (320, 180), 1)])
def test_the_gpu_build_states_the_hosts_words(lib, name, wh, ss):
    """The table as the library builds it on the GPU is the host build's word for word, with and without the flag."""
    s = two_mirrors() if name == "two_mirrors" else h8(supersample=ss)
    blob = rt_host.flatten_scene(s)
    r = rt_host.Renderer(blob, 0, lib)
    try:
        for tiles in ((wh[1], 0, 1, 1), (16, 1, 2, (wh[1] // 16) // 2)):
            for flags in (SECOND_NODE, FIRST_BOUNCE, PLAIN | 128 | 256, PLAIN | 256):
                assert gpu_table(lib, r, *wh, tiles, flags, ss) == host_table(lib, blob, *wh, tiles, flags)
    finally:
        r.close()


def sky_index(s):
    return next(k for k, o in enumerate(s["objects"]) if o["r2"] == 25000000)


def edited(lib, scene_after, step, w=1001, h=563):
    """h8 resident, two frames, the edit, two frames: the last ones equal a fresh upload's of `scene_after` (and the switch changes
    nothing).  Returns the waves per frame."""
    on, off = both(lib, h8(), w, h, steps=[step])
    took = same(on, off)
    want = fresh(lib, scene_after, w, h)
    assert on[2][0] == want and on[3][0] == want
    return took


def test_recolouring_the_skybox(lib):
    """Nothing of the statement depends on the background's colour: the table stays, the walks still leave the mirrors out."""
    s = h8()
    i = sky_index(s)
    s["objects"][i]["mtl"]["color"] = [0.25, 0.5, 0.125]
    took = edited(lib, s, lambda r: r.set_objects([s["objects"][i]], i))
    assert took[1] > 0 and took[3] > 0, took


def test_restyling_the_skybox_to_a_texture(lib):
    """No constant background (no sky marks, another launch table): the walks still leave the mirrors out."""
    s = h8()
    i = sky_index(s)
    tex = next(o for o in s["objects"] if o["mtl"]["sampler"]["kind"] == 1)
    s["objects"][i]["mtl"]["sampler"] = copy.deepcopy(tex["mtl"]["sampler"])
    took = edited(lib, s, lambda r: r.set_objects([s["objects"][i]], i))
    assert took[1] > 0 and took[3] > 0, took


def test_restyling_the_skybox_to_a_mirror(lib):
    """No set is stated beside an enclosing sphere that reflects, so no bit either."""
    s = reflecting_sky()
    i = sky_index(s)
    took = edited(lib, s, lambda r: r.set_objects([s["objects"][i]], i))
    assert took[1] > 0 and took[2] == 0 and took[3] == 0, took


def test_moving_a_light(lib):
    s = h8()
    s["lights"][0] = [-4.0, 8.0, 6.0]
    took = edited(lib, s, lambda r: r.set_lights(s["lights"][:1], 0))
    assert took[3] > 0, took


def test_moving_a_mirror_next_to_another(lib):
    """The moved mirror's rays now reach its neighbour: the table is rebuilt and its blocks keep that neighbour in their walks."""
    s = h8()
    i = next(k for k, o in enumerate(s["objects"]) if o["origin"] == [0, 1, -2])
    s["objects"][i]["origin"] = [-1.5, 1.0, 2.1]
    took = edited(lib, s, lambda r: r.set_objects([s["objects"][i]], i))
    assert took[3] > 0, took
