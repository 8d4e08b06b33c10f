"""The scalar loads a trace wave issues ahead of their uses (rt_kernel_entry.h: rt_head_batch - the launch-record fields of the prologue go out
beside the launch-table entry's load in the few-sphere one-wave kernels).  What can go wrong with such a batch is a field read at a moved
offset, or - for a batch of a one-candidate wave's sphere records, which was built, measured and dropped (docs/EVIDENCE.md) - a load issued
for an entry it does not belong to: the bits under `cand & 255` mean something else in sky runs, multi-candidate and empty entries.  So the
shapes are the smallest that hold every entry kind, and each is held to three yardsticks:
  * the SECOND frame of a resident scene (one-wave workgroups: the kernels with the batch) equals, byte for byte, its FIRST frame
    (the four-wave form of the kernel, which has no batch and never takes the uniform-material path),
  * and the test library's second frame with RT_NO_UNIFORM_BLOCKS (every wave on the general path),
  * and it stays within 1 LSB of the C restatement (oracle/rt_oracle.c).
The product library's two frames are held to the same bytes: its kernels are a build of their own (no RT_TESTING)."""
import copy
import ctypes as C
import os

import pytest

import oracle_util as ou
import rt_host
from objects_util import tlib  # noqa: F401  (fixture: the test library)

pytestmark = pytest.mark.gpu

SWITCH = "RT_NO_UNIFORM_BLOCKS"
FLOOR_R2 = 250000.0


@pytest.fixture(scope="module")
def lib(tlib):  # noqa: F811
    tlib.rt_test_uniform_waves.restype = C.c_int
    tlib.rt_test_uniform_waves.argtypes = [C.c_int, C.POINTER(C.c_ulonglong)]
    return tlib


@pytest.fixture(scope="module")
def plib(built):
    return rt_host.load_library()


def uniform_waves(lib):
    n = C.c_ulonglong()
    assert lib.rt_test_uniform_waves(0, C.byref(n)) == 0, lib.rt_last_error()
    return n.value


def frames(lib, scene, w, h, tiles, camera=None, count=False):
    """[first frame, second frame] of a fresh upload (after one set_camera if `camera`), and the waves of the second that took the
    uniform-material path (test library only)."""
    t = rt_host.RtTiles(*tiles)
    n = t.n_tiles * t.tile_rows * w * 4
    r = rt_host.Renderer(rt_host.flatten_scene(scene), 0, lib)
    out, took = [], None
    try:
        if camera is not None:
            r.set_camera(camera)
        for k in range(2):
            d = lib.rt_alloc_device(0, n)
            assert d, lib.rt_last_error()
            try:
                if count:
                    uniform_waves(lib)
                r.render_tiles(w, h, d, t)
                if count:
                    took = uniform_waves(lib)
                host = C.create_string_buffer(n)
                assert lib.rt_copy_to_host(0, host, d, n) == 0, lib.rt_last_error()
                out.append(host.raw)
            finally:
                lib.rt_free_device(0, d)
    finally:
        r.close()
    return out, took


def restatement(scene, w, h, tiles):
    """The C restatement's rows of the call's output band, tile after tile."""
    blob = rt_host.flatten_scene(scene)
    tile_rows, first, stride, n_tiles = tiles
    return b"".join(ou.c_oracle_render(blob, w, h, (first + k * stride) * tile_rows, min(h, (first + k * stride + 1) * tile_rows)) for k in range(n_tiles))


def hold(lib, plib, scene, w, h, tiles=None, camera=None):
    """The three yardsticks of the module's docstring; returns (and prints) the waves of the second frame that completed the uniform-material path."""
    tiles = tiles or (h, 0, 1, 1)
    (first, second), took = frames(lib, scene, w, h, tiles, camera, count=True)
    os.environ[SWITCH] = "1"
    try:
        (_, general), none = frames(lib, scene, w, h, tiles, camera, count=True)
    finally:
        os.environ.pop(SWITCH, None)
    assert none == 0, none                                        # the switch really kept every wave off the path
    assert second == first, "one-wave frame differs from the four-wave frame"
    assert second == general, "one-wave frame differs from the general path's"
    (pfirst, psecond), _ = frames(plib, scene, w, h, tiles, camera)
    assert psecond == pfirst, "product library: one-wave frame differs from the four-wave frame"
    assert psecond == second, "product library's frame differs from the test library's"
    shown = copy.deepcopy(scene)
    if camera is not None:
        shown["camera"] = camera
    ora = restatement(shown, w, h, tiles)
    assert len(ora) == len(second), (len(ora), len(second))
    lsb, frac = ou.max_lsb(second, ora)
    print("%dx%d: uniform-material waves %d, |gpu - restatement| <= %d LSB in %.2e of the channels" % (w, h, took, lsb, frac))
    assert lsb <= 1, (lsb, frac)
    return took


def h8():
    return rt_host.load_scene("h8")


def floor_of(s):
    return next(o for o in s["objects"] if o["r2"] == FLOOR_R2)


def with_loop_spheres(n_loop):
    """h8 (7 spheres in the loops and the enclosing sky sphere) with small plain spheres added in a row on the floor in front of the camera."""
    s = h8()
    proto = next(o for o in s["objects"] if o["r2"] == 1)
    k = 0
    while len(s["objects"]) - 1 < n_loop:
        o = copy.deepcopy(proto)
        o["origin"], o["r2"] = [-2.5 + 1.0 * k, 0.3, 4.0], 0.09
        o["mtl"]["albedo"] = [0, 0.8, 0.3, 0.0, 0]
        s["objects"].insert(0, o)
        k += 1
    return s


# (every frame of h8 below its horizon shows blocks of nothing but the floor: one-candidate entries; above it sky runs; the spheres' blocks
#  name two candidates or none - and the ragged sizes add blocks with rows_valid < 8 and slots behind the table's last entry)
@pytest.mark.parametrize("w,h", [(64, 40), (33, 9), (1001, 563)])
def test_h8_sizes(lib, plib, w, h):
    """64x40: whole blocks only; 33x9: a partial block in both directions (rows_valid = 1, a width that is no multiple of 32);
    1001x563: many blocks of every kind."""
    took = hold(lib, plib, h8(), w, h)
    if (w, h) == (1001, 563):                  # (as tests/test_gpu_uniform_blocks.py holds this frame: waves do complete the uniform-material path.  The small
        assert took > 0                        #  frames need not: every wave of the one-wave kernels uses the batch, whichever path it takes)


def test_h8_supersample_2(lib, plib):
    """rt_trace<0,0,1,0,1>: four lanes per pixel, blocks of 32 x 2 pixels."""
    s = h8()
    s["supersample"] = 2
    hold(lib, plib, s, 64, 40)


def test_cfg2_textures(lib, plib):
    """Textured spheres alone in their blocks: a one-candidate wave's sampler word names the texture descriptor."""
    hold(lib, plib, rt_host.load_scene("cfg2"), 64, 40)


def test_one_sphere_without_enclosing_sphere(lib, plib):
    """The floor alone: no enclosing sphere, so sky entries without sky_fast (their waves trace, and take the miss colour)."""
    s = h8()
    s["objects"] = [floor_of(s)]
    hold(lib, plib, s, 64, 40)


@pytest.mark.parametrize("n_loop", [12, 13])
def test_most_loop_spheres(lib, plib, n_loop):
    """12 spheres in the loops: the largest scene the few-sphere kernels run (rt_scene.hip: more than RT_SGRID_MIN_LOOP take the many-sphere
    variant); 13: the first scene of the many-sphere one-wave kernel, which keeps its own prologue."""
    s = with_loop_spheres(n_loop)
    assert len(s["objects"]) == n_loop + 1
    hold(lib, plib, s, 64, 40)


@pytest.mark.parametrize("rank", [0, 1])
def test_h8_interleaved_tiles_of_two_ranks(lib, plib, rank):
    """64x48 in tiles of 16 rows dealt to two ranks: rank 0 renders tiles 0 and 2, rank 1 tile 1."""
    hold(lib, plib, h8(), 64, 48, tiles=(16, rank, 2, 2 - rank))


def test_h8_after_set_camera(lib, plib):
    """One camera move after the upload: the first frame from the new camera runs the four-wave form, the second one-wave workgroups."""
    import bench
    s = h8()
    hold(lib, plib, s, 64, 40, camera=bench.moving_camera(s, 3, 16))
