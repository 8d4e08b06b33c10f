"""The uniform-material path of the one-wave product kernels (rt_kernel.hip: trace_pixel, UNI): a wave whose launch-table entry names ONE
primary candidate shades with that sphere's material in scalar registers.  The path performs the general path's own statements, so every
frame must be BYTE FOR BYTE what the general path stores - the test library's RT_NO_UNIFORM_BLOCKS keeps every wave on it - and the
samples marked for the second, exact launch (rt_stats.exact_samples) must be as many.  rt_test_uniform_waves counts the waves that took
the path, so that no comparison is vacuous: taken where it is meant to be, and not where it is not."""
import copy
import ctypes as C
import os

import pytest

import rt_host
from objects_util import tlib  # noqa: F401  (fixture: the test library)

pytestmark = pytest.mark.gpu

W4K, H4K = 3840, 2160
FLOOR_R2 = 250000.0
SWITCH = "RT_NO_UNIFORM_BLOCKS"


@pytest.fixture(scope="module")
def lib(tlib):  # noqa: F811
    tlib.rt_test_uniform_waves.restype = C.c_int
    tlib.rt_test_uniform_waves.argtypes = [C.c_int, C.POINTER(C.c_ulonglong)]
    return tlib


def waves(lib):
    """Waves that took the path since the last call (drains the device, resets the counter)."""
    n = C.c_ulonglong()
    assert lib.rt_test_uniform_waves(0, C.byref(n)) == 0, lib.rt_last_error()
    return n.value


def shot(lib, r, w, h, tiles=None, flags=0, keep=None):
    """One call's output bytes (the first `keep` of them), its exact_samples, and the waves that took the path."""
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


class general_path:
    """The test library's switch: inside the block every wave takes the general path."""

    def __init__(self, on):
        self.on = on

    def __enter__(self):
        if self.on:
            os.environ[SWITCH] = "1"

    def __exit__(self, *a):
        os.environ.pop(SWITCH, None)


def both(lib, scene, w, h, tiles=None, flags=0, keep=None, cameras=()):
    """[(frame, exact_samples, waves) per frame] with the path and with the switch: a fresh upload each, two frames, then two frames
    per camera of `cameras` (the first frame from a camera - an upload's or a move's - runs the four-wave form of the kernel, which
    never takes the path; the later ones run one-wave workgroups)."""
    out = []
    for off in (False, True):
        with general_path(off):
            r = rt_host.Renderer(rt_host.flatten_scene(scene), 0, lib)
            try:
                frames = [shot(lib, r, w, h, tiles, flags, keep), shot(lib, r, w, h, tiles, flags, keep)]
                for cam in cameras:
                    r.set_camera(cam)
                    frames.append(shot(lib, r, w, h, tiles, flags, keep))
                    frames.append(shot(lib, r, w, h, tiles, flags, keep))
            finally:
                r.close()
        out.append(frames)
    return out


def same(on, off):
    """Frames and exact_samples equal, the switch really off the path; returns the waves that took it, per frame."""
    assert len(on) == len(off)
    for k, (a, b) in enumerate(zip(on, off)):
        assert b[2] == 0, (k, b[2])
        assert a[1] == b[1], (k, a[1], b[1])
        assert a[0] == b[0], "frame %d differs" % k
    return [a[2] for a in on]


def floor(s):
    return next(i for i, o in enumerate(s["objects"]) if o["r2"] == FLOOR_R2)


def test_h8_headline_frame(lib):
    """3840x2160: about half the blocks are sky, and most of the rest show nothing but the floor."""
    _, took = same(*both(lib, rt_host.load_scene("h8"), W4K, H4K))
    assert took >= 0.3 * (W4K // 8) * (H4K // 8), took


def test_h8_ragged_size(lib):
    _, took = same(*both(lib, rt_host.load_scene("h8"), 1001, 563))
    assert took > 0


@pytest.mark.parametrize("rank", [0, 1])
def test_h8_interleaved_tiles_of_two_ranks(lib, rank):
    n_tiles = (H4K // 16 - rank + 1) // 2
    _, took = same(*both(lib, rt_host.load_scene("h8"), W4K, H4K, tiles=(16, rank, 2, n_tiles)))
    assert took > 0


@pytest.mark.parametrize("name,wh", [("cfg2", (1920, 1080)), ("h8_d8", (1920, 1080)), ("lcg64_ss1", (1280, 720))])
def test_other_reflection_only_scenes(lib, name, wh):
    """cfg2: a textured sphere alone in many blocks; h8_d8: depth 8; lcg64_ss1: the many-sphere one-wave kernel (materials in HBM)."""
    _, took = same(*both(lib, rt_host.load_scene(name), *wh))
    assert took > 0, name


def test_lcg64_supersampled_kernel_is_left_without_the_path(lib):
    """lcg64 as it is (supersample 2): rt_trace<0,0,1,1,1>, cfg5's kernel, which does not take the path (rt_kernel.hip: UNI_OK)."""
    s = rt_host.load_scene("lcg64")
    assert s["supersample"] == 2
    _, took = same(*both(lib, s, 1280, 720))
    assert took == 0


@pytest.mark.parametrize("name", ["h8", "cfg2"])
def test_supersample_2_few_spheres(lib, name):
    """2x2 supersampling in the few-sphere one-wave kernel, rt_trace<0,0,1,0,1>: four lanes per pixel, the box filter across the quad."""
    s = rt_host.load_scene(name)
    s["supersample"] = 2
    _, took = same(*both(lib, s, 1001, 563))
    assert took > 0
    _, took = same(*both(lib, s, 1920, 1080, flags=rt_host.RT_FLAG_RGB24, keep=1920 * 1080 * 3))
    assert took > 0


def test_general_kernel_never_takes_it(lib):
    _, took = same(*both(lib, rt_host.load_scene("default14"), 1280, 720))
    assert took == 0


def test_moved_camera(lib):
    """Two of the benchmark's orbit positions: the first frame after a move runs four-wave workgroups (no path), the next one-wave ones."""
    import bench
    s = rt_host.load_scene("h8")
    cams = [bench.moving_camera(s, k, 16) for k in (3, 11)]
    took = same(*both(lib, s, 1920, 1080, cameras=cams))
    assert took[1] > 0
    for k in (1, 2):
        assert took[2 * k] == 0 and took[2 * k + 1] > 0, took


def inside_scene():
    """The camera INSIDE a large childless checker sphere that is not the scene's enclosing one (a planet lies outside it)."""
    s = rt_host.load_scene("h8")
    objs = s["objects"]
    shell = copy.deepcopy(objs[floor(s)])
    shell["origin"], shell["r2"] = [0, 0, 0], 900.0
    shell["mtl"]["sampler"]["freqU"], shell["mtl"]["sampler"]["freqV"] = 40, 20
    keep = [o for o in objs if o["r2"] in (0.25, 16, 25000000) or o["origin"] == [0, 1, -2]]
    s["objects"] = keep + [shell]
    return s


def test_camera_inside_the_candidate(lib):
    """The launch table makes no statement about a sphere the camera is inside of (rt_block.h: rt_ball.everywhere): its blocks name
    no candidate, so the path is not meant to be taken there - and the frames are the general path's."""
    _, took = same(*both(lib, inside_scene(), 1280, 720))
    assert took == 0


def test_reflecting_floor_stays_on_the_general_path(lib):
    """albedo[3] > 0 on the floor: its blocks spawn rays and must not take the path (the two planets' blocks still may)."""
    s = rt_host.load_scene("h8")
    _, plain = same(*both(lib, s, 1920, 1080))
    s["objects"][floor(s)]["mtl"]["albedo"][3] = 0.3
    _, took = same(*both(lib, s, 1920, 1080))
    assert took < plain // 10, (took, plain)


def test_rgb24_band(lib):
    _, took = same(*both(lib, rt_host.load_scene("h8"), 1920, 1080, flags=rt_host.RT_FLAG_RGB24, keep=1920 * 1080 * 3))
    assert took > 0


def test_compact_band(lib):
    s, w, h = rt_host.load_scene("h8"), 1920, 1080
    r = rt_host.Renderer(rt_host.flatten_scene(s), 0, lib)
    try:
        n, bb = r.compact_count(w, h, (h, 0, 1, 1))
    finally:
        r.close()
    assert 0 < n * bb <= w * h * 4
    flags = rt_host.RT_FLAG_RGB24 | rt_host.RT_FLAG_NO_SKY | rt_host.RT_FLAG_COMPACT
    _, took = same(*both(lib, s, w, h, flags=flags, keep=n * bb))
    assert took > 0
