"""The scalar side of the one-wave few-sphere trace kernels: a wave's launch-table entry and what addresses it (rt_kernel_entry.h), and the
arms of the uniform-material path that were restructured for the scalar unit (rt_kernel_trace.h: the sampler's decision tree, the light
loop's no_occluder test; rt_kernel_math.h: rt_pow_spec<UNI>, rt_sqrt_nn's clamp).

ENTRY ADDRESSING.  A wave's first load is its launch-table entry, at (workgroup % 8) * stride + workgroup / 8 (/ 32: one-wave workgroups)
of the table; words 1 to 3 are read again later from the same slot.  What can go wrong with a change to how that address is formed is a
field read at a moved offset, a stride that is not the table's, or a kernel (rt_retrace, the four-wave form) launched with another
argument list than it reads.  So: tables of 1, 7, 8, 9 and 33 entries (the stride is ceil(n / 8)), ragged sizes, a two-frame batch, an
odd frame whose centre row and column go through rt_retrace, and a moved camera's first frame (one workgroup per block: zero slots behind
the last entry) - each held, as tests/test_gpu_prologue_loads.py holds its shapes, to
  * second frame (one-wave workgroups) == first frame (four-wave workgroups), byte for byte, in the test and the product library,
  * == the test library's second frame with every wave on the general path,
  * within 1 LSB of the C restatement (oracle/rt_oracle.c).

UNIFORM-PATH ARMS.  A 64x16 band of one floor sphere - the last 16 rows of a 64x64 frame from h8's camera (the reference's camera cannot
pitch, main.js:187-191, and a 16-row frame has the horizon in it): four blocks, every wave's entry names one candidate and all its 64 rays
meet the floor 17 degrees and more below the horizon.  Per arm of the path - sampler kind, the albedo tests,
the specular power's walk for one scalar exponent, the light loop's masks, depth 1, a shadow scan that runs - the frame bytes and
exact_samples with the path equal those with RT_NO_UNIFORM_BLOCKS (as tests/test_gpu_uniform_blocks.py compares them), and
rt_test_uniform_waves says that the path was taken."""
import copy
import ctypes as C
import os

import pytest

import oracle_util as ou
import rt_host
import test_gpu_prologue_loads as pl          # hold, frames, restatement: the three yardsticks
from objects_util import tlib  # noqa: F401  (fixture: the test library)

pytestmark = pytest.mark.gpu

SWITCH = "RT_NO_UNIFORM_BLOCKS"


@pytest.fixture(scope="module")
def lib(tlib):  # noqa: F811
    for f in (tlib.rt_test_uniform_waves, tlib.rt_test_cell_waves):
        f.restype = C.c_int
        f.argtypes = [C.c_int, C.POINTER(C.c_ulonglong)]
    return tlib


@pytest.fixture(scope="module")
def plib(built):
    return rt_host.load_library()


def low_camera(s):
    """The scene from h8's own camera position lowered to 0.1 above the floor (the sphere's surface lies at y = -0.1 there), looking along -z as
    h8's camera does (the reference's camera cannot pitch: main.js:187-191 scales the ray's components): the horizon lies within a pixel of
    the frame's centre row, so the rows further below show the floor alone (checked with the C restatement: rows 8 .. 15 of a 64x16 frame,
    rows 24 .. 31 of a 32-row frame 32 and 1056 pixels across)."""
    s = copy.deepcopy(s)
    s["camera"]["origin"] = [0.0, 0.002, 10.0]
    return s


def floor_alone(**mtl):
    """h8's floor (a checker sphere of radius 500) under h8's two lights and from h8's camera, nothing else; `mtl`: entries of its material replaced."""
    s = pl.h8()
    f = pl.floor_of(s)
    f["mtl"].update(copy.deepcopy(mtl))
    s["objects"] = [f]
    return s


# ---------------------------------------------------------------------------------------------------------------- entry addressing
@pytest.mark.parametrize("w,h", [(32, 8), (224, 8), (256, 8), (288, 8), (96, 24), (100, 20), (33, 9)])
def test_entry_address_h8(lib, plib, w, h):
    """h8 as it is (sky runs above the horizon, the spheres' blocks, floor blocks): the issue's shapes.  100x20: a width that is no multiple of
    32, a height that is no multiple of 8; 33x9: odd both ways - its centre row and column are traced again by rt_retrace."""
    pl.hold(lib, plib, pl.h8(), w, h)


@pytest.mark.parametrize("entries", [1, 7, 8, 9, 33])
def test_entry_address_table_sizes(lib, plib, entries):
    """One row of `entries` floor blocks (the last 8-row tile of a 32-row frame; no sky run merges any): a table of exactly that many
    entries - below, at and above the eight XCDs' round, and five rounds.  Every block is a one-candidate block: its waves take the
    uniform-material path (all but the few with a sample in the boundary test's band)."""
    s = low_camera(pl.h8())
    s["objects"] = [o for o in s["objects"] if o["r2"] >= pl.FLOOR_R2]          # the floor and the enclosing sphere: no other candidate
    took = pl.hold(lib, plib, s, 32 * entries, 32, tiles=(8, 3, 1, 1))           # rows 24 .. 31 of a 32-row frame: the floor alone
    assert 0 < took <= 4 * entries, took


def test_entry_address_moved_camera_first_frame(lib, plib):
    """The first frame from a moved camera: the host does not know the rebuilt table's size yet and launches one workgroup per block - the
    slots behind the last entry are zero and their workgroups leave at once (rows_valid == 0)."""
    import bench
    s = pl.h8()
    pl.hold(lib, plib, s, 100, 20, camera=bench.moving_camera(s, 3, 16))


def batch_frames(lib, scene, w, h, n_frames):
    """[first call, second call] of a fresh upload: n_frames frames per call in one launch (blockIdx.z), each call's frames as a list."""
    n = w * h * 4
    r = rt_host.Renderer(rt_host.flatten_scene(scene), 0, lib)
    out = []
    try:
        for _ in range(2):
            d = lib.rt_alloc_device(0, n * n_frames)
            assert d, lib.rt_last_error()
            try:
                r.render_batch(w, h, d, (h, 0, 1, 1), n_frames, n)
                host = C.create_string_buffer(n * n_frames)
                assert lib.rt_copy_to_host(0, host, d, n * n_frames) == 0, lib.rt_last_error()
                out.append([host.raw[k * n:(k + 1) * n] for k in range(n_frames)])
            finally:
                lib.rt_free_device(0, d)
    finally:
        r.close()
    return out


@pytest.mark.parametrize("which", ["test", "product"])
def test_entry_address_two_frame_batch(lib, plib, which):
    """blockIdx.z = 1: the second frame of a batch reads the same table."""
    s, w, h = pl.h8(), 100, 20
    first, second = batch_frames(lib if which == "test" else plib, s, w, h, 2)
    assert second == first, "one-wave batch differs from the four-wave batch"
    assert second[1] == second[0], "the batch's frames differ"
    lsb, _ = ou.max_lsb(second[1], pl.restatement(s, w, h, (h, 0, 1, 1)))
    assert lsb <= 1, lsb


# ---------------------------------------------------------------------------------------------------------------- uniform-path arms
W, H = 64, 16
BAND = (H, 3, 1, 1)                  # the band: tile 3 of four 16-row tiles of a W x 64 frame


def waves(lib, f):
    n = C.c_ulonglong()
    assert f(0, C.byref(n)) == 0, lib.rt_last_error()
    return n.value


def second_frame(lib, scene, off):
    """The second frame (one-wave workgroups) of a fresh upload, its exact_samples, and the waves of it that took the uniform-material path
    and that took their checker cell from the table; `off`: with RT_NO_UNIFORM_BLOCKS."""
    n = W * H * 4
    if off:
        os.environ[SWITCH] = "1"
    try:
        r = rt_host.Renderer(rt_host.flatten_scene(scene), 0, lib)
        try:
            for k in range(2):
                d = lib.rt_alloc_device(0, n)
                assert d, lib.rt_last_error()
                try:
                    waves(lib, lib.rt_test_uniform_waves), waves(lib, lib.rt_test_cell_waves)
                    st = r.render_tiles(W, 4 * H, d, BAND, want_stats=True)
                    took, cells = waves(lib, lib.rt_test_uniform_waves), waves(lib, lib.rt_test_cell_waves)
                    host = C.create_string_buffer(n)
                    assert lib.rt_copy_to_host(0, host, d, n) == 0, lib.rt_last_error()
                finally:
                    lib.rt_free_device(0, d)
        finally:
            r.close()
    finally:
        os.environ.pop(SWITCH, None)
    return host.raw, int(st.exact_samples), took, cells


def arm(lib, scene, taken=True):
    """Frame bytes and exact_samples equal with the path and without; returns (frame, waves on the path, waves with a stated cell)."""
    on, off = second_frame(lib, scene, False), second_frame(lib, scene, True)
    assert off[2] == 0, off[2]                                   # the switch really kept every wave off the path
    assert on[1] == off[1], (on[1], off[1])
    assert on[0] == off[0], "the path's frame differs from the general path's"
    print("uniform-material waves %d of %d, %d with a stated cell" % (on[2], (W // 8) * (H // 8), on[3]))
    if taken:
        assert on[2] > 0
    return on[0], on[2], on[3]


CHECKER = {"kind": 2, "colors": [[1, 1, 0], [1, 0, 1]]}


@pytest.mark.parametrize("kind", ["colour", "texture", "checker_cell_stated", "checker_cell_not_stated"])
def test_uniform_sampler_kinds(lib, kind):
    sampler = {"colour": {"kind": 0}, "texture": {"kind": 1, "texture": 0},
               "checker_cell_stated": dict(CHECKER, freqU=6, freqV=3),            # cells of hundreds of units, the view in the middle of one
               "checker_cell_not_stated": dict(CHECKER, freqU=100000, freqV=50000)}[kind]     # cells of 0.03 units: a wave's column (0.4 units across) spans several
    _, took, cells = arm(lib, floor_alone(sampler=sampler, color=[0.9, 0.6, 0.3]))
    if kind == "checker_cell_stated":
        assert cells > 0
    if kind == "checker_cell_not_stated":
        assert cells == 0


@pytest.mark.parametrize("albedo", [[0.2, 0, 0, 0, 0], [0.1, 0.7, 0, 0, 0]], ids=["a1_a2_zero", "a2_zero"])
def test_uniform_albedo_tests(lib, albedo):
    """a1 = a2 = 0: the light loop is not entered; a2 = 0: no specular term, no power."""
    arm(lib, floor_alone(albedo=albedo))


@pytest.mark.parametrize("exponent", [0, 1, 2, 3, 50, 64, 1023, 2.5])
def test_uniform_specular_exponents(lib, exponent):
    """The scalar walk from set bit to set bit: no bit (1.0), one bit at the bottom, one higher up, two adjacent, several, a single high
    one, ten set bits; 2.5: no integer - OCML's pow out of line."""
    arm(lib, floor_alone(specular_exponent=exponent, albedo=[0, 0.3, 0.9, 0, 0]))


@pytest.mark.parametrize("n_lights", [0, 1, 2, 3])
def test_uniform_light_counts(lib, n_lights):
    """The entry's shadow masks cover lights 0 and 1; a third light scans every sphere."""
    s = floor_alone()
    s["lights"] = [[5, 10, 5], [5, 10, 0], [-4, 8, 6]][:n_lights]
    arm(lib, s)


def test_uniform_depth_1(lib):
    s = floor_alone()
    s["segs"] = 1
    arm(lib, s)


def test_uniform_shadow_scan_runs(lib):
    """A small sphere 39 degrees above the camera's horizontal, on the way from light 0 to the floor the band shows: the floor blocks are still
    one-candidate blocks, their shadow masks name the sphere, and the scan runs on the path - the frame differs from the one without it."""
    plain = floor_alone()
    s = copy.deepcopy(plain)
    ball = copy.deepcopy(next(o for o in pl.h8()["objects"] if o["r2"] == 1))
    ball["origin"], ball["r2"] = [3.0, 6.0, 5.4], 0.09             # at 0.4 of the way from the light [5, 10, 5] to the floor at [0, 0, 6]
    s["objects"].insert(0, ball)
    lit, _, _ = arm(lib, plain)
    shadowed, _, _ = arm(lib, s)
    assert shadowed != lit, "no shadow in the frame: the scene does not test what it is meant to"
