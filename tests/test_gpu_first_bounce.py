"""First-bounce sets on the GPU (rt_kernel_trace.h: the node after the primary): a wave of the few-sphere reflection-only product kernels
whose launch-table entry names the spheres its reflected rays can meet (rt_block.h: rt_first_bounce_set) tests those at its first
bounce instead of every loop sphere.  Every frame must be BYTE FOR BYTE what the kernel stores when it ignores the statement - the test
library's RT_NO_FIRST_BOUNCE - with as many samples marked for the exact launch (rt_stats.exact_samples).  rt_test_first_bounce_waves
counts the waves that walked a set, so that no comparison is vacuous: above 0 and at most the waves of the host table's stating entries
(four per entry; a wave none of whose primary rays meets a mirror never bounces and walks nothing - which waves those are is a
per-lane fact the host table does not hold, so the count is bounded, not matched).  Each frame is rendered twice and the second one
counts: a camera's first frame runs the four-wave form of the kernel (which walks the sets as well)."""
import ctypes as C
import os

import pytest

import rt_host
from objects_util import gpu_table, host_table, tlib  # noqa: F401  (fixture: the test library)
from test_first_bounce import CELLS, FIRST_BOUNCE, PLAIN, bench_moving_camera, h8, reflecting_sky, stating, table, two_mirrors

pytestmark = pytest.mark.gpu

SWITCH = "RT_NO_FIRST_BOUNCE"


@pytest.fixture(scope="module")
def lib(tlib):  # noqa: F811
    tlib.rt_test_first_bounce_waves.restype = C.c_int
    tlib.rt_test_first_bounce_waves.argtypes = [C.c_int, C.POINTER(C.c_ulonglong)]
    return tlib


def waves(lib):
    """Waves that walked a first-bounce set since the last call; drains the device."""
    a = C.c_ulonglong()
    assert lib.rt_test_first_bounce_waves(0, C.byref(a)) == 0, lib.rt_last_error()
    return a.value


def shot(lib, r, w, h, tiles=None, flags=0, keep=None):
    t = rt_host.RtTiles(*(tiles or (h, 0, 1, 1)))
    n = t.n_tiles * t.tile_rows * w * 4
    d = lib.rt_alloc_device(0, n)
    assert d, lib.rt_last_error()
    try:
        waves(lib)
        st = r.render_tiles(w, h, d, t, flags=flags, want_stats=True)
        took = waves(lib)
        host = C.create_string_buffer(n)
        assert lib.rt_copy_to_host(0, host, d, n) == 0, lib.rt_last_error()
    finally:
        lib.rt_free_device(0, d)
    return host.raw[:keep if keep is not None else n], int(st.exact_samples), took


def both(lib, scene, w, h, tiles=None, flags=0, keep=None, steps=()):
    """Per setting of the switch: a fresh upload, two frames, then per step - a callable that edits the resident scene - two more.
    Returns the two lists of (frame, exact_samples, set waves)."""
    out = []
    for off in (False, True):
        if off:
            os.environ[SWITCH] = "1"
        try:
            r = rt_host.Renderer(rt_host.flatten_scene(scene), 0, lib)
            try:
                frames = [shot(lib, r, w, h, tiles, flags, keep), shot(lib, r, w, h, tiles, flags, keep)]
                for step in steps:
                    step(r)
                    frames += [shot(lib, r, w, h, tiles, flags, keep), shot(lib, r, w, h, tiles, flags, keep)]
            finally:
                r.close()
        finally:
            os.environ.pop(SWITCH, None)
        out.append(frames)
    return out


def same(on, off):
    """Frames and exact_samples equal; the switch really ignores the sets.  Returns the set waves per frame."""
    assert len(on) == len(off)
    for k, (a, b) in enumerate(zip(on, off)):
        assert b[2] == 0, (k, b[2])
        assert a[1] == b[1], (k, a[1], b[1])
        assert a[0] == b[0], "frame %d differs" % k
    return [a[2] for a in on]


def host_waves(lib, scene, w, h, tiles=None):
    return 4 * len(stating(table(lib, rt_host.flatten_scene(scene), w, h, FIRST_BOUNCE, tiles)))


@pytest.mark.parametrize("wh", [(1001, 563), (640, 360)])
def test_h8(lib, wh):
    s = h8()
    took = same(*both(lib, s, *wh))
    assert 0 < took[1] <= host_waves(lib, s, *wh), took


def test_h8_supersample_2(lib):
    s = h8(supersample=2)
    took = same(*both(lib, s, 320, 184))
    assert 0 < took[1] <= host_waves(lib, s, 320, 184), took


def test_two_mirrors_facing_each_other(lib):
    s = two_mirrors()
    took = same(*both(lib, s, 256, 256))
    assert 0 < took[1] <= host_waves(lib, s, 256, 256), took


def test_a_frame_after_set_camera(lib):
    s = h8()
    moved = h8()
    moved["camera"] = bench_moving_camera(s, 5, 64)
    took = same(*both(lib, s, 640, 360, steps=[lambda r: r.set_camera(moved["camera"])]))
    assert 0 < took[1] <= host_waves(lib, s, 640, 360), took
    assert 0 < took[3] <= host_waves(lib, moved, 640, 360), took


def test_rgb24_band_of_two_interleaved_ranks(lib):
    s, w, h = h8(), 640, 360
    tiles = (16, 1, 2, (h // 16) // 2)
    took = same(*both(lib, s, w, h, tiles=tiles, flags=rt_host.RT_FLAG_RGB24, keep=tiles[3] * 16 * w * 3))
    assert 0 < took[1] <= host_waves(lib, s, w, h, tiles), took


def test_depth_1_and_a_refracting_scene_walk_no_set(lib):
    for s, wh in ((h8(segs=1), (640, 360)), (rt_host.load_scene("default14"), (320, 180))):
        took = same(*both(lib, s, *wh))
        assert took == [0, 0], took


def test_a_reflecting_enclosing_sphere_walks_no_set(lib):
    """Lanes of a mirror's silhouette block that miss the mirror bounce off the skybox: no set is stated, none is walked, and the restyle
    that makes the skybox a mirror (and the one that takes it back) invalidates the table with the sets."""
    took = same(*both(lib, reflecting_sky(), 1001, 563))
    assert took == [0, 0], took
    s, r = h8(), reflecting_sky()
    i = next(k for k, o in enumerate(s["objects"]) if o["r2"] == 25000000)
    steps = [lambda rr: rr.set_objects([r["objects"][i]], i), lambda rr: rr.set_objects([s["objects"][i]], i)]
    took = same(*both(lib, s, 1001, 563, steps=steps))
    assert took[1] > 0 and took[2] == 0 and took[3] == 0 and took[5] == took[1], took


@pytest.mark.parametrize("name,wh,ss", [("h8", (1001, 563), 1), ("h8", (320, 184), 2), ("two_mirrors", (256, 256), 1)])
def test_the_gpu_build_states_the_hosts_words(lib, name, wh, ss):
    """The table as the library builds it on the GPU is the host build's word for word, with and without the sets."""
    s = two_mirrors() if name == "two_mirrors" else h8(supersample=ss)
    blob = rt_host.flatten_scene(s)
    r = rt_host.Renderer(blob, 0, lib)
    try:
        for tiles in ((wh[1], 0, 1, 1), (16, 1, 2, (wh[1] // 16) // 2)):
            for flags in (FIRST_BOUNCE, PLAIN | 128, CELLS):
                assert gpu_table(lib, r, *wh, tiles, flags, ss) == host_table(lib, blob, *wh, tiles, flags)
    finally:
        r.close()
