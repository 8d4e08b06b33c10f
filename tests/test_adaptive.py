"""Adaptive supersampling without a GPU (include/rt_hip.h: rt_adaptive_work_bytes, rt_render_adaptive_device): the workspace arithmetic,
the argument checks that come before a scene or a device is touched, and the two rules of csrc/rt_adaptive.h - the criterion (the test
library's rt_test_adaptive_mask, a plain host loop over the function the kernel calls) against rt_host.adaptive_mask in numpy, and the
box rule against (sum + k k // 2) // (k k)."""
import ctypes as C
import os

import numpy as np
import pytest

import oracle_util as ou
import rt_host
from test_gpu_adaptive import BEYOND_ONE_TURN, HOLES, LARGEST_EXTENTS      # (tables only: importing the module needs no GPU)

OK, INVALID, STATE = 0, -1, -5


@pytest.fixture(scope="module")
def lib(built):
    lib = rt_host.load_library(rt_host.TEST_LIB_PATH)
    lib.rt_test_adaptive_mask.restype = C.c_int
    lib.rt_test_adaptive_mask.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p]
    lib.rt_test_adaptive_box.restype = C.c_uint32
    lib.rt_test_adaptive_box.argtypes = [C.c_uint32, C.c_uint32]
    lib.rt_test_adaptive_refine_grid.restype = C.c_uint32
    lib.rt_test_adaptive_refine_grid.argtypes = [C.c_uint32, C.c_uint32, C.c_uint32]
    return lib


def test_status_codes_are_the_headers():
    text = open(os.path.join(rt_host.ROOT, "include", "rt_hip.h")).read()
    for name, value in (("RT_OK", OK), ("RT_ERR_INVALID", INVALID), ("RT_ERR_STATE", STATE)):
        assert ("%s = %d" % (name, value)) in text, name


# ------------------------------------------------------------------ the workspace
def test_work_bytes(lib):
    for w, h in [(1, 1), (1, 70), (64, 64), (131, 60), (3840, 2160), (32768, 1), (32768, 32768)]:
        assert lib.rt_adaptive_work_bytes(w, h) == 16 + 4 * w * h, (w, h)
        assert rt_host.adaptive_work_bytes(w, h, lib) == 16 + 4 * w * h
    for w, h in [(0, 0), (0, 5), (5, 0), (32769, 1), (1, 32769), (65536, 65536), (2 ** 32 - 1, 1)]:
        assert lib.rt_adaptive_work_bytes(w, h) == 0, (w, h)
    sides = [1, 2, 63, 64, 65, 1000, 32767, 32768]
    for h in sides:                                     # non-decreasing in each side over the frames the call accepts
        row = [lib.rt_adaptive_work_bytes(w, h) for w in sides]
        col = [lib.rt_adaptive_work_bytes(h, w) for w in sides]
        assert row == sorted(row) and col == sorted(col)


# ------------------------------------------------------------------ the argument checks
def call(lib, scene=None, w=64, h=48, k=4, t=32, out=0x1000, mask=0, work=0x2000, work_bytes=None, flags=0):
    wb = lib.rt_adaptive_work_bytes(w, h) if work_bytes is None else work_bytes
    return lib.rt_render_adaptive_device(scene, w, h, k, t, C.c_void_p(out), C.c_void_p(mask), C.c_void_p(work), wb, None, flags, None)


BAD = {
    "k 0": dict(k=0), "k 1": dict(k=1), "k 5": dict(k=5), "k 2^32 - 1": dict(k=2 ** 32 - 1),
    "threshold 257": dict(t=257), "threshold 2^32 - 1": dict(t=2 ** 32 - 1),
    "w 0": dict(w=0), "h 0": dict(h=0),
    "k w above 65536": dict(w=16385, k=4, work_bytes=1 << 40), "k h above 65536": dict(h=21846, k=3, work_bytes=1 << 40),
    "w above 65536": dict(w=65537, k=2, work_bytes=1 << 40),
    "NULL output": dict(out=0), "NULL workspace": dict(work=0),
    "misaligned output": dict(out=0x1002), "misaligned workspace": dict(work=0x2001),
    "workspace one byte short": dict(work_bytes=16 + 4 * 64 * 48 - 1), "no workspace bytes": dict(work_bytes=0),
    "RT_FLAG_COUNT": dict(flags=rt_host.RT_FLAG_COUNT), "RT_FLAG_RGB24": dict(flags=rt_host.RT_FLAG_RGB24),
    "RT_FLAG_NO_SKY | RT_FLAG_STRICT_FP": dict(flags=rt_host.RT_FLAG_NO_SKY | rt_host.RT_FLAG_STRICT_FP), "an unknown flag": dict(flags=1 << 20),
}


@pytest.mark.parametrize("case", list(BAD))
def test_bad_arguments_are_invalid_before_the_scene_is_looked_at(lib, case):
    assert call(lib, None, **BAD[case]) == INVALID, (case, lib.rt_last_error())
    assert lib.rt_last_error()


def test_valid_arguments_reach_the_scene_check(lib):
    for kw in [dict(), dict(k=2), dict(k=3, t=0), dict(t=256), dict(flags=rt_host.RT_FLAG_STRICT_FP), dict(mask=0x3001), dict(w=16384, h=16384, k=4, work_bytes=1 << 40),
               dict(w=1, h=1, k=2)]:
        assert call(lib, None, **kw) == STATE, (kw, lib.rt_last_error())


# ------------------------------------------------------------------ the criterion
def library_mask(lib, frame, w, h, t):
    frame = np.ascontiguousarray(frame, np.uint8)
    assert frame.size == w * h * 4
    out = np.full(w * h + 8, 0xEE, np.uint8)            # (8 bytes behind the mask: nothing is written there)
    assert lib.rt_test_adaptive_mask(frame.ctypes.data, w, h, t, out.ctypes.data) == OK, lib.rt_last_error()
    assert (out[w * h:] == 0xEE).all()
    return out[:w * h].reshape(h, w)


def both(lib, frame, w, h, t):
    got, want = library_mask(lib, frame, w, h, t), rt_host.adaptive_mask(frame, w, h, t)
    assert want.shape == (h, w) and want.dtype == np.uint8 and set(np.unique(want)) <= {0, 1}
    assert (got == want).all(), (w, h, t, np.argwhere(got != want)[:8])
    return want


def flat(w, h, rgb=(100, 100, 100), a=255):
    f = np.empty((h, w, 4), np.uint8)
    f[...] = (*rgb, a)
    return f


def test_one_bright_pixel_marks_itself_and_its_4_neighbours(lib):
    f = flat(7, 5)
    f[2, 3, :3] = (200, 100, 100)
    m = both(lib, f, 7, 5, 32)
    want = np.zeros((5, 7), np.uint8)
    want[2, 2:5] = 1; want[1, 3] = 1; want[3, 3] = 1
    assert (m == want).all()                            # (the diagonals stay)


@pytest.mark.parametrize("channel", [0, 1, 2])
@pytest.mark.parametrize("t", [1, 8, 32, 255])
def test_a_difference_equal_to_the_threshold_marks_and_one_below_does_not(lib, channel, t):
    for a, b in [(0, t), (255 - t, 255), (255, 255 - t)]:
        f = flat(2, 1, (a, a, a))
        f[0, 1, channel] = b
        assert both(lib, f, 2, 1, t).all()
        if t < 255:
            assert not both(lib, f, 2, 1, t + 1).any()
        f = f.reshape(2, 1, 4)                          # the same two pixels one above the other
        assert both(lib, f, 1, 2, t).all()


def test_alpha_differences_mark_nothing(lib):
    f = flat(6, 4)
    f[..., 3] = np.arange(24, dtype=np.uint8).reshape(4, 6) * 10
    assert not both(lib, f, 6, 4, 1).any()


def test_corners_and_edges(lib):
    for y, x in [(0, 0), (0, 8), (5, 0), (5, 8), (0, 4), (5, 4), (3, 0), (3, 8)]:
        f = flat(9, 6)
        f[y, x, 1] = 0
        m = both(lib, f, 9, 6, 64)
        want = np.zeros((6, 9), np.uint8)
        for dy, dx in [(0, 0), (0, 1), (0, -1), (1, 0), (-1, 0)]:
            if 0 <= y + dy < 6 and 0 <= x + dx < 9:
                want[y + dy, x + dx] = 1
        assert (m == want).all(), (y, x)


def test_thin_frames_and_the_extreme_thresholds(lib):
    rng = np.random.default_rng(5)
    for w, h in [(1, 1), (1, 9), (9, 1), (2, 2), (64, 1), (65, 3), (130, 2)]:
        f = rng.integers(0, 256, (h, w, 4), dtype=np.uint8)
        assert both(lib, f, w, h, 0).all(), (w, h)      # 0 marks all: a 1 x 1 frame's only pixel too
        assert not both(lib, f, w, h, 256).any(), (w, h)
        for t in (1, 16, 100, 255):
            both(lib, f, w, h, t)
    assert not both(lib, flat(1, 1), 1, 1, 1).any()      # no neighbour, nothing to differ from
    f = flat(5, 5)
    assert both(lib, f, 5, 5, 0).all() and not both(lib, f, 5, 5, 1).any()


def test_random_frames(lib):
    rng = np.random.default_rng(11)
    for w, h in [(33, 17), (128, 5)]:
        f = (rng.integers(0, 256, (h, w, 4)) // 32 * 32).astype(np.uint8)
        for t in (1, 32, 33, 64, 224, 225):
            both(lib, f, w, h, t)


@pytest.mark.parametrize("name", ["h8_240x135", "default14_160x90", "cfg2_240x135", "lcg64_ss1_192x192"])
def test_golden_frames(lib, name):
    entry = next(f for f in ou.manifest()["frames"] if f["name"] == name)
    frame, w, h = ou.golden_frame(entry), entry["w"], entry["h"]
    shares = {}
    for t in (8, 32, 64):
        shares[t] = float(both(lib, frame, w, h, t).mean())
    print("ADAPTIVE refined share of %s at T = 8, 32, 64: %s" % (name, ", ".join("%.1f %%" % (100 * shares[t]) for t in (8, 32, 64))))
    assert shares[8] >= shares[32] >= shares[64] > 0.0


# ------------------------------------------------------------------ the box rule
@pytest.mark.parametrize("k", [2, 3, 4])
def test_box_rule(lib, k):
    n = k * k
    sums = {0, 255 * n, 255 * n - 1, 1}
    for q in (0, 1, 2, 100, 254):                       # one below and at the step from q to q + 1: sum + n // 2 == (q + 1) n
        step = (q + 1) * n - n // 2
        sums |= {step - 1, step}
    for s in sorted(sums):
        assert 0 <= s <= 255 * n
        assert lib.rt_test_adaptive_box(s, k) == (s + n // 2) // n, (k, s)
    assert lib.rt_test_adaptive_box(0, k) == 0 and lib.rt_test_adaptive_box(255 * n, k) == 255
    assert all(lib.rt_test_adaptive_box(s, k) == (s + n // 2) // n for s in range(255 * n + 1))


# ------------------------------------------------------------------ the refine launch's grid, and the GPU cases that must outrun it
CAP = 8192                                              # (today's; the cap itself is found below, not assumed by the GPU cases)


def frame_of(px):
    """A frame of exactly px pixels with both sides in 1..32768 if there is one (the hook is plain arithmetic and takes any)."""
    return next(((px // h, h) for h in range(1, 4097) if px % h == 0 and px // h <= 32768), (px, 1))


@pytest.mark.parametrize("k", [2, 3, 4])
def test_refine_grid(lib, k):
    """rt_adaptive_refine_grid(w, h, k) = min(ceil(w h / (4 waves x 64 // k^2 pixels)), 8192): small frames, frames at the cap, and the
    cap plus or minus one workgroup - each of those as exactly that many workgroups' pixels, one pixel fewer and one more."""
    per_wg = 4 * (64 // (k * k))
    want = lambda w, h: min(-(-w * h // per_wg), CAP)
    frames = [(1, 1), (per_wg, 1), (per_wg + 1, 1), (1, per_wg + 1), (131, 60), (240, 135), (3840, 2160), (32768, 1), (1, 32768), (16384, 16384)]
    for wgs in (CAP - 1, CAP, CAP + 1):
        for px in (wgs * per_wg - 1, wgs * per_wg, wgs * per_wg + 1):
            w, h = frame_of(px)
            assert w * h == px
            frames += [(w, h), (h, w)]
    got = {(w, h): lib.rt_test_adaptive_refine_grid(w, h, k) for w, h in frames}
    assert got == {(w, h): want(w, h) for w, h in frames}
    assert got[frame_of((CAP - 1) * per_wg)] == CAP - 1 and got[frame_of((CAP - 1) * per_wg + 1)] == CAP
    assert got[frame_of(CAP * per_wg + 1)] == CAP and got[frame_of((CAP + 1) * per_wg + 1)] == CAP and got[(1, 1)] == 1


@pytest.mark.parametrize("k,w,h", BEYOND_ONE_TURN)
def test_the_large_gpu_cases_outrun_one_turn_and_end_in_a_partly_filled_wave(lib, k, w, h):
    """What makes tests/test_gpu_adaptive.py's T = 0 cases reach the second turn of rt_adaptive_refine's loop, against the library's
    own grid: one turn cannot hold the fully refined frame, and what is left over does not fill its last wave."""
    ppw = 64 // (k * k)
    turn = lib.rt_test_adaptive_refine_grid(w, h, k) * 4 * ppw
    assert w * h > turn
    assert (w * h - turn) % ppw != 0
    assert w * h - turn < turn                          # (and it is the second turn that ends the list: a few seconds' frame)
    assert call(lib, None, w=w, h=h, k=k, t=0) == STATE  # the call admits the frame


def test_every_k_has_a_large_gpu_case_and_the_case_with_holes_can_outrun_one_turn(lib):
    assert sorted(c[0] for c in BEYOND_ONE_TURN) == [2, 3, 4]
    name, w, h, k, t = HOLES
    assert 0 < t < 256 and k == 4
    # check() caps the refined share of such a frame at 0.60: a list under that cap must still be able to exceed one turn
    assert 0.60 * w * h > lib.rt_test_adaptive_refine_grid(w, h, k) * 4 * (64 // (k * k))
    assert call(lib, None, w=w, h=h, k=k, t=t) == STATE


def test_the_largest_extents_are_admitted_and_one_more_is_not(lib):
    for w, h, k in LARGEST_EXTENTS:
        assert max(k * w, k * h) == 65536 and max(w, h) - 1 <= 0x7fff
        assert call(lib, None, w=w, h=h, k=k, t=16) == STATE, (w, h, k, lib.rt_last_error())
        bigger = dict(w=w + 1, h=h) if w > h else dict(w=w, h=h + 1)
        assert call(lib, None, k=k, t=16, work_bytes=1 << 40, **bigger) == INVALID
    assert {(w > h, k) for w, h, k in LARGEST_EXTENTS} == {(True, 4), (False, 4), (True, 2), (False, 2)}
