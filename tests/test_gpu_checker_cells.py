"""Checker cells on the GPU (rt_kernel.hip: trace_pixel, one_cell): a wave of the few-sphere one-wave kernels whose launch-table entry
states that its 64 samples lie inside ONE checker cell (rt_block.h: rt_column_cell) takes the cell's colour from the table and skips
the sampler.  Every frame must be BYTE FOR BYTE what the kernel stores when it ignores the statement - the test library's
RT_NO_CHECKER_CELLS - with as many samples marked for the exact launch (rt_stats.exact_samples); rt_test_cell_waves counts the waves
that used the statement, so that no comparison is vacuous, and must equal the host table's count of flagged waves."""
import copy
import ctypes as C
import os

import pytest

import rt_host
from objects_util import gpu_table, host_table, tlib  # noqa: F401  (fixture: the test library)
from test_checker_cells import CELLS, flagged_waves, h8, pole_scene, scaled, table, floor_of

pytestmark = pytest.mark.gpu

SWITCH = "RT_NO_CHECKER_CELLS"


@pytest.fixture(scope="module")
def lib(tlib):  # noqa: F811
    for f in (tlib.rt_test_cell_waves, tlib.rt_test_uniform_waves):
        f.restype = C.c_int
        f.argtypes = [C.c_int, C.POINTER(C.c_ulonglong)]
    return tlib


def waves(lib):
    """(waves that used a table cell, waves that took the uniform-material path) since the last call; drains the device."""
    a, b = C.c_ulonglong(), C.c_ulonglong()
    assert lib.rt_test_cell_waves(0, C.byref(a)) == 0, lib.rt_last_error()
    assert lib.rt_test_uniform_waves(0, C.byref(b)) == 0, lib.rt_last_error()
    return a.value, b.value


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
    """Per setting of the switch: a fresh upload, two frames (the first runs the four-wave form), then per step - a callable that
    edits the resident scene - two more.  Returns the two lists of (frame, exact_samples, (cell waves, uniform waves))."""
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
    """Frames, exact_samples and the uniform path's waves equal; the switch really ignores the cells; a camera's first frame (the
    four-wave form) uses none.  Returns the cell waves per frame."""
    assert len(on) == len(off)
    for k, (a, b) in enumerate(zip(on, off)):
        assert b[2][0] == 0, (k, b[2])
        assert a[2][1] == b[2][1], (k, a[2], b[2])
        assert a[1] == b[1], (k, a[1], b[1])
        assert a[0] == b[0], "frame %d differs" % k
        if k == 0:
            assert a[2][0] == 0, (k, a[2])
    return [a[2][0] for a in on]


def host_count(lib, scene, w, h, tiles=None):
    return len(flagged_waves(table(lib, rt_host.flatten_scene(scene), w, h, CELLS, tiles)))


def test_h8_headline_frame(lib):
    """Every flagged wave of the host table shows nothing but the childless floor, all lanes on it: the path accepts each of them."""
    s = h8()
    took = same(*both(lib, s, 3840, 2160))
    assert took[1] == host_count(lib, s, 3840, 2160) > 20000, took


def test_h8_ragged_size(lib):
    s = h8()
    took = same(*both(lib, s, 1001, 563))
    assert took[1] == host_count(lib, s, 1001, 563) > 0, took


def test_h8_moving_camera_and_edits(lib):
    """Two of the benchmark's orbit positions, then the floor's sampler from checker to colour and back, then a light move."""
    import bench
    s = h8()
    i = s["objects"].index(floor_of(s))
    plain = copy.deepcopy(s["objects"][i])
    plain["mtl"]["sampler"] = {"kind": 0}
    steps = [lambda r, k=k: r.set_camera(bench.moving_camera(s, k, 64)) for k in (5, 40)]
    steps += [lambda r: r.set_objects([plain], i), lambda r: r.set_objects([s["objects"][i]], i), lambda r: r.set_lights([[4.0, 9.0, 6.0]], 0)]
    took = same(*both(lib, s, 1920, 1080, steps=steps))
    assert took[1] > 0 and took[3] > 0 and took[5] > 0, took
    assert took[2] == 0 and took[4] == 0, took                 # the first frame from a moved camera: the four-wave form
    assert took[7] == 0, took                                  # a colour floor: no cell to state
    assert took[9] == took[5] and took[11] == took[5], took    # the checker is back; lights do not enter the statement


def test_h8_supersample_2(lib):
    s = h8(supersample=2)
    took = same(*both(lib, s, 1001, 563))
    assert took[1] == host_count(lib, s, 1001, 563) > 0, took


@pytest.mark.parametrize("factor", [0.1, 10.0])
def test_scaled_frequencies(lib, factor):
    s = scaled(factor)
    took = same(*both(lib, s, 1920, 1080))
    assert took[1] == host_count(lib, s, 1920, 1080), took


def test_largest_admitted_frequency(lib):
    same(*both(lib, scaled(freq=(131072.0, 131072.0)), 1920, 1080))


def test_poles_and_branch_cut_on_screen(lib):
    s = pole_scene()
    took = same(*both(lib, s, 1920, 1080))
    assert took[1] == host_count(lib, s, 1920, 1080) > 0, took


@pytest.mark.parametrize("rank", [0, 1])
def test_h8_interleaved_tiles_of_two_ranks(lib, rank):
    tiles = (16, rank, 2, (2160 // 16 - rank + 1) // 2)
    took = same(*both(lib, h8(), 3840, 2160, tiles=tiles))
    assert took[1] == host_count(lib, h8(), 3840, 2160, tiles) > 0, took


def test_rgb24_and_compact_bands(lib):
    s, w, h = h8(), 1920, 1080
    took = same(*both(lib, s, w, h, flags=rt_host.RT_FLAG_RGB24, keep=w * h * 3))
    assert took[1] > 0
    r = rt_host.Renderer(rt_host.flatten_scene(s), 0, lib)
    try:
        n, bb = r.compact_count(w, h, (h, 0, 1, 1))
    finally:
        r.close()
    flags = rt_host.RT_FLAG_RGB24 | rt_host.RT_FLAG_NO_SKY | rt_host.RT_FLAG_COMPACT
    took = same(*both(lib, s, w, h, flags=flags, keep=n * bb))
    assert took[1] > 0


def test_many_sphere_kernel_is_left_without_it(lib):
    """lcg64_ss1: rt_trace<0,0,0,1,1> takes the uniform-material path but not this change (no scalar register to spare)."""
    took = same(*both(lib, rt_host.load_scene("lcg64_ss1"), 1280, 720))
    assert took[1] == 0


@pytest.mark.parametrize("name,wh,ss", [("h8", (3840, 2160), 1), ("h8", (1001, 563), 2), ("pole", (1280, 720), 1)])
def test_the_gpu_build_states_the_hosts_words(lib, name, wh, ss):
    """The table as the library builds it on the GPU, with the cells, is the host build's word for word."""
    s = pole_scene() if name == "pole" else h8(supersample=ss)
    blob = rt_host.flatten_scene(s)
    r = rt_host.Renderer(blob, 0, lib)
    try:
        for tiles in ((wh[1], 0, 1, 1), (16, 1, 2, (wh[1] // 16) // 2)):
            assert gpu_table(lib, r, *wh, tiles, CELLS, ss) == host_table(lib, blob, *wh, tiles, CELLS)
    finally:
        r.close()
