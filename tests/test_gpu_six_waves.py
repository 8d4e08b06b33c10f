"""Six waves per SIMD for the few-sphere one-wave trace kernels (rt_trace<0,0,0,0,1> and <0,0,1,0,1>: 80 VGPRs, 6 400 bytes of LDS for eight
spheres).  The change moves data - the cull rectangles and texture descriptors out of the staged LDS image, a finished lane's colour into
its own fold-state slots, the work-item id into v_mbcnt, two material words read a second time - and no arithmetic, so the yardstick is byte equality: the SECOND frame of each case (one-wave workgroups; the first frame of a resident
scene runs the four-wave form) is held to the sha256 of the same frame from the PARENT commit's product library, recorded once on the GPU
with that library in place of the tree's (docs/EVIDENCE.md, "Six waves per SIMD").  The test library's second frame is held to the same
bytes.  The cases are the smallest that reach every region the change touches."""
import ctypes as C
import hashlib

import pytest

import rt_host
import test_gpu_prologue_loads as pl          # h8, with_loop_spheres
from objects_util import tlib  # noqa: F401  (fixture: the test library)
from test_gpu_prologue_loads import plib  # noqa: F401  (fixture: the product library)

pytestmark = pytest.mark.gpu


def _h8(**kw):
    s = pl.h8()
    s.update(kw)
    return s


def _moved(s):
    import bench
    return bench.moving_camera(s, 3, 16)


# name -> (scene, w, h, tiles, flags, frames of the batch, camera move before the first frame)
CASES = {
    "h8_96x24": (lambda: pl.h8(), 96, 24, None, 0, 1, False),                       # mirrors, bounces to depth 3, floor, horizon, sky runs
    "h8_33x9": (lambda: pl.h8(), 33, 9, None, 0, 1, False),                         # odd width, a partly valid last block row, narrow stores
    "h8_ss2_48x16": (lambda: _h8(supersample=2), 48, 16, None, 0, 1, False),        # rt_trace<0,0,1,0,1>
    "h8_d8_64x16": (lambda: rt_host.load_scene("h8_d8"), 64, 16, None, 0, 1, False),   # deep chains through the fold state
    "cfg2_64x16": (lambda: rt_host.load_scene("cfg2"), 64, 16, None, 0, 1, False),  # textures (descriptors read from HBM now) and a sphere checker
    "h8_rgb24_band": (lambda: pl.h8(), 64, 64, (16, 2, 1, 1), rt_host.RT_FLAG_RGB24, 1, False),   # the epilogue's 24-bit stores, a band
    "h8_batch2_64x16": (lambda: pl.h8(), 64, 16, None, 0, 2, False),                # two frames in one launch (grid z)
    "h8_moved_camera": (lambda: pl.h8(), 64, 16, None, 0, 1, True),                 # the second frame from a moved camera
    "h8_9_spheres": (lambda: pl.with_loop_spheres(8), 64, 16, None, 0, 1, False),   # the staged image is the materials alone: one sphere more
    "h8_16_spheres": (lambda: pl.with_loop_spheres(15), 64, 16, None, 0, 1, False), # ... and the first scene size of the many-sphere kernels
}

# sha256 of the second frame, by the parent commit's product library (recorded with it on the GPU; never from the tree under test)
PARENT_SHA256 = {
    "cfg2_64x16": "77acd2bd36d3f07303533533032e59261cb463cb70c141d5341c35d1be8f7fad",
    "h8_16_spheres": "ad6c1fde7bcf0b868574a78425ce035f64680fa1757e538f0cccd6381cc05749",
    "h8_33x9": "1f405c2d667504d4468b50f885372d6f8ec045ab67fda3c4f033c5e0194c2915",
    "h8_96x24": "388768b7e32acc4b0d659b9d08335b577e265d851e5fdac59fa9cb0de24591f3",
    "h8_9_spheres": "a772789f4d86ab6bdc58a1b06315f04482903edd9a8a524ec76bafd8f9f90a49",
    "h8_batch2_64x16": "54c19a2e8faf601aa50ba0707ad4e5a813422da1f6a479d57cdb4c8d7dbbc4a3",
    "h8_d8_64x16": "cbcc1ba9cb16720e4b6ef03610f69157050083b303e367cf5539411364697b41",
    "h8_moved_camera": "a28e8179fc603c379ff7cb1bb55d87636a0842465aac15f082aeed4655d13fa6",
    "h8_rgb24_band": "37edec2a59c0e3ec839449408c8bbb886e6957997181e84931d085cf15d31f3b",
    "h8_ss2_48x16": "0dbc83c5ce3020de243693d59ce52b101b7e2ddf5038b0f7dd5b2ee309313b0e",
}


def second_frame(lib, name):
    make, w, h, tiles, flags, n_frames, moved = CASES[name]
    scene = make()
    t = rt_host.RtTiles(*(tiles or (h, 0, 1, 1)))
    per_frame = t.n_tiles * t.tile_rows * w * (3 if flags & rt_host.RT_FLAG_RGB24 else 4)
    n = per_frame * n_frames
    r = rt_host.Renderer(rt_host.flatten_scene(scene), 0, lib)
    try:
        if moved:
            r.set_camera(_moved(scene))
        out = None
        for _ in range(2):
            d = lib.rt_alloc_device(0, n)
            assert d, lib.rt_last_error()
            try:
                if n_frames == 1:
                    r.render_tiles(w, h, d, t, flags=flags)
                else:
                    r.render_batch(w, h, d, t, n_frames, per_frame, flags=flags)
                host = C.create_string_buffer(n)
                assert lib.rt_copy_to_host(0, host, d, n) == 0, lib.rt_last_error()
                out = host.raw
            finally:
                lib.rt_free_device(0, d)
        return out
    finally:
        r.close()


@pytest.mark.parametrize("name", sorted(CASES))
def test_second_frame_is_the_parents(tlib, plib, name):  # noqa: F811
    frame = second_frame(plib, name)
    sha = hashlib.sha256(frame).hexdigest()
    print(name, "sha256", sha)
    assert len(set(frame[i:i + 4] for i in range(0, len(frame) - 3, 4))) > 8, "a flat frame: the case does not test what it is meant to"
    assert sha == PARENT_SHA256[name]
    assert hashlib.sha256(second_frame(tlib, name)).hexdigest() == sha, "the test library's frame differs from the product library's"
