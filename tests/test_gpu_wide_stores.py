"""The 16-byte frame stores of the product trace kernels on the GPU (rt_kernel.hip, A10; csrc/rt_wide.h; rt_device.h: rt_wide_stores_of).

Every frame is rendered by the test library twice, with and without RT_NO_WIDE_STORES (one 4-byte store per pixel, the epilogue
every launch had before), and the two must agree BYTE FOR BYTE; the same frames lie within the suite's usual 1 LSB of the C
restatement's rows, alpha is 255 everywhere, and the output buffer stands between two guards of 256 bytes - and, where a batch has a
stride or a band rows past the frame, between and behind its frames - filled with a pattern that must be intact afterwards.
tests/test_wide_stores.py has enumerated the stores of these shapes on the CPU beforehand.

Each frame size is rendered four times per setting: after rt_scene_set_camera with the scene's own camera (the first frame from a
camera runs the four-wave form of its kernel, the second the one-wave form where the variant has one) and again after a camera move."""
import ctypes as C
import os

import numpy as np
import pytest

import oracle_util as ou
import rt_host
from objects_util import tlib  # noqa: F401  (fixture: the test library)
from test_wide_stores import FALLBACK_WIDTHS, HEIGHTS, SCENES, WIDE_WIDTHS, entries, scene_of, sky_runs

pytestmark = pytest.mark.gpu

SWITCH = "RT_NO_WIDE_STORES"
GUARD, PATTERN = 256, 0xA5


def moved(scene):
    import bench
    s = dict(scene)
    s["camera"] = {k: [float(x) for x in v] for k, v in bench.moving_camera(scene, 5, 64).items()}
    return s


def shot(lib, r, w, h, tiles, n_frames=1, gap=0, offset=0):
    """One launch into a guarded buffer: `offset` bytes between the front guard and `out`, `gap` bytes between the frames of a batch.
    Returns the frames' bands (bytes each); asserts that every byte outside them still holds the pattern."""
    t = rt_host.RtTiles(*tiles)
    band = t.n_tiles * t.tile_rows * w * 4
    stride = band + gap
    n = GUARD + offset + n_frames * stride + GUARD
    d = lib.rt_alloc_device(0, n)
    assert d, lib.rt_last_error()
    try:
        assert d % 256 == 0
        assert lib.rt_memset_device(0, d, PATTERN, n) == 0, lib.rt_last_error()
        out = d + GUARD + offset
        if n_frames == 1:
            r.render_tiles(w, h, out, t)
        else:
            r.render_batch(w, h, out, t, n_frames, stride)
        host = C.create_string_buffer(n)
        assert lib.rt_copy_to_host(0, host, d, n) == 0, lib.rt_last_error()
    finally:
        lib.rt_free_device(0, d)
    a = np.frombuffer(host.raw, dtype=np.uint8)
    keep = np.ones(n, bool)
    frames = []
    for f in range(n_frames):
        lo = GUARD + offset + f * stride
        keep[lo:lo + band] = False
        frames.append(a[lo:lo + band].tobytes())
    assert (a[keep] == PATTERN).all(), "a store outside the frames' bands"
    return frames


def band_rows_of(h, tiles):
    """(rows of the band that are rows of the frame, the frame rows they are)"""
    rows, t_rows, first, step, n_tiles = [], *tiles
    for i in range(n_tiles):
        for j in range(t_rows):
            fr = (first + i * step) * t_rows + j
            if fr < h:
                rows.append((i * t_rows + j, fr))
    return rows


def oracle_rows(scene, w, h):
    return np.frombuffer(ou.c_oracle_render(rt_host.flatten_scene(scene), w, h), dtype=np.uint8).reshape(h, w, 4).astype(np.int16)


def check(frame, ora, w, h, tiles):
    """One band against the C restatement's rows: 1 LSB, alpha 255; band rows past the frame's last row untouched."""
    got = np.frombuffer(frame, dtype=np.uint8).reshape(-1, w, 4)
    rows = band_rows_of(h, tiles)
    b, f = [x[0] for x in rows], [x[1] for x in rows]
    assert int(np.abs(got[b].astype(np.int16) - ora[f]).max()) <= 1
    assert (got[b][:, :, 3] == 255).all()
    rest = np.ones(got.shape[0], bool)
    rest[b] = False
    assert (got[rest] == PATTERN).all()


def both(lib, scene, shapes, **kw):
    """Per setting of the switch one upload; per (w, h, tiles) of `shapes` four launches (module docstring).  Asserts the statement
    of the module docstring for every frame."""
    cams = (scene, moved(scene))
    got = []
    for off in (False, True):
        if off:
            os.environ[SWITCH] = "1"
        try:
            r = rt_host.Renderer(rt_host.flatten_scene(scene), 0, lib)
            try:
                frames = []
                for w, h, tiles in shapes:
                    for s in cams:
                        r.set_camera(s["camera"])
                        frames += [shot(lib, r, w, h, tiles, **kw), shot(lib, r, w, h, tiles, **kw)]
            finally:
                r.close()
        finally:
            os.environ.pop(SWITCH, None)
        got.append(frames)
    assert got[0] == got[1], "the 16-byte stores and the 4-byte stores leave different bytes"
    k = 0
    for w, h, tiles in shapes:
        for s in cams:
            ora = oracle_rows(s, w, h)                       # computed once per camera and size, shared by its frames
            for launch in got[0][k:k + 2]:
                for frame in launch:
                    check(frame, ora, w, h, tiles)
            k += 2


@pytest.mark.parametrize("scene", SCENES)
@pytest.mark.parametrize("w", WIDE_WIDTHS + FALLBACK_WIDTHS)
def test_whole_frames(tlib, scene, w):  # noqa: F811
    both(tlib, scene_of(scene), [(w, h, (h, 0, 1, 1)) for h in HEIGHTS])


def test_640_has_the_sky_runs(tlib):  # noqa: F811
    """The run lengths the frames above store, off the host table: 1 to 5 (every wave residue) and 8 or more."""
    runs = set()
    for s in SCENES:
        for h in HEIGHTS:
            runs |= set(sky_runs(entries(tlib, rt_host.flatten_scene(scene_of(s)), 640, h, (h, 0, 1, 1))))
    assert {1, 2, 3, 4, 5} <= runs and max(runs) >= 8, runs


@pytest.mark.parametrize("scene", ["h8", "h8_ss2"])
@pytest.mark.parametrize("rank", [0, 1])
def test_interleaved_tiles_of_two_ranks(tlib, scene, rank):  # noqa: F811
    w, h = 640, 72                           # 16-row tiles: four and a half of them, dealt to two ranks (lrow != frow)
    both(tlib, scene_of(scene), [(w, h, (16, rank, 2, (-(-h // 16) - rank + 1) // 2))])


@pytest.mark.parametrize("gap", [0, 80, 4])
def test_batch_of_two_frames(tlib, gap):  # noqa: F811
    """A stride of whole 16-byte units takes the 16-byte stores, one of 4 bytes more the fallback."""
    both(tlib, scene_of("h8"), [(132, 17, (17, 0, 1, 1)), (640, 9, (9, 0, 1, 1))], n_frames=2, gap=gap)


@pytest.mark.parametrize("offset", [4, 16])
def test_offset_output(tlib, offset):  # noqa: F811
    """`out` 4 bytes past a 16-byte boundary: the fallback; 16 bytes: the 16-byte stores."""
    both(tlib, scene_of("h8"), [(132, 17, (17, 0, 1, 1)), (640, 9, (9, 0, 1, 1))], offset=offset)
