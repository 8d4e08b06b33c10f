"""TEST INFRASTRUCTURE for the GPU tests of resident-scene edits (tests/test_gpu_objects.py, tests/test_gpu_restyle.py): the test
library, the scenes, and the yardsticks a moved or restyled scene is held to - a fresh upload of the edited blob (every
sphere-dependent region of the scene and its launch table word for word, every frame byte for byte) and the C restatement."""
import ctypes as C

import numpy as np
import pytest

import oracle_util as ou
import rt_host

FAST, STRICT = 0, rt_host.RT_FLAG_STRICT_FP
SKYBOX_R2 = 25000000.0
PARTS = range(7)           # records, geometry, ordering B, LDS images, shadow grids, bounce table, camera block


@pytest.fixture(scope="module")
def tlib(built):
    lib = rt_host.load_library(rt_host.TEST_LIB_PATH)
    assert lib.rt_init(1) == 0, lib.rt_last_error()
    lib.rt_test_scene_state.restype = C.c_longlong
    lib.rt_test_scene_state.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_size_t]
    lib.rt_test_upload_count.restype = C.c_int
    lib.rt_test_upload_count.argtypes = []
    lib.rt_test_launch_table.restype = C.c_int
    lib.rt_test_launch_table.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.POINTER(rt_host.RtTiles), C.c_int, C.POINTER(C.c_uint32),
                                         C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]
    return lib


def load(name):
    if name.startswith("many:"):
        import soak_gpu_parity as soak
        sc = soak.draw_scene(int(name[5:]), False, True)[0]
        sc["segs"] = max(sc["segs"], 2)
    else:
        sc = rt_host.load_scene(name)
    if sc.get("supersample", 1) > 2:
        sc["supersample"] = 1
    return sc


def set_objects(r, scene, first, end):
    r.set_objects(scene["objects"][first:end], first)


def state(lib, r):
    out = []
    for part in PARTS:
        n = lib.rt_test_scene_state(r.handle, part, None, 0)
        assert n >= 0, lib.rt_last_error()
        buf = C.create_string_buffer(max(n, 1))
        assert lib.rt_test_scene_state(r.handle, part, buf, n) == n, lib.rt_last_error()
        out.append(buf.raw[:n])
    return out


def gpu_table(lib, r, w, h, tiles, ranked, ss):
    t = rt_host.RtTiles(*tiles)
    n, nb = C.c_uint32(), C.c_uint32()
    rows_per_wg = 2 if ss == 2 else 8
    blocks = ((w + 31) // 32) * t.n_tiles * ((t.tile_rows + rows_per_wg - 1) // rows_per_wg)
    out = (C.c_uint32 * (4 * (blocks + 8)))()
    assert lib.rt_test_launch_table(r.handle, w, h, C.byref(t), ranked, out, C.byref(n), C.byref(nb)) == 0, lib.rt_last_error()
    assert nb.value == blocks
    return n.value, bytes(out)[:((blocks + 7) // 8) * 8 * 16]


def host_table(lib, blob, w, h, tiles, ranked):
    buf = C.create_string_buffer(blob, len(blob))
    t = rt_host.RtTiles(*tiles)
    n, nb = C.c_uint32(), C.c_uint32()
    assert lib.rt_scene_launch_table(buf, len(blob), w, h, C.byref(t), ranked, None, C.byref(n), C.byref(nb)) == 0, lib.rt_last_error()
    out = (C.c_uint32 * (32 * ((nb.value + 7) // 8)))()
    assert lib.rt_scene_launch_table(buf, len(blob), w, h, C.byref(t), ranked, out, C.byref(n), C.byref(nb)) == 0
    return n.value, bytes(out)


class Frames:
    """Device buffers for a few frames of `tiles`, rendered without host waits and read back at the end."""

    def __init__(self, lib, w, h, tiles, n_frames=1):
        self.lib, self.w, self.h, self.t = lib, w, h, rt_host.RtTiles(*tiles)
        self.n = self.t.n_tiles * self.t.tile_rows * w * 4 * n_frames
        self.n_frames = n_frames
        self.bufs = []

    def render(self, r, flags=0):
        d = self.lib.rt_alloc_device(0, self.n)
        assert d, self.lib.rt_last_error()
        self.bufs.append(d)
        if self.n_frames == 1:
            r.render_tiles(self.w, self.h, d, self.t, flags=flags)
        else:
            r.render_batch(self.w, self.h, d, self.t, self.n_frames, self.n // self.n_frames, flags=flags)

    def read(self):
        out = []
        for d in self.bufs:
            host = C.create_string_buffer(self.n)
            assert self.lib.rt_copy_to_host(0, host, d, self.n) == 0, self.lib.rt_last_error()
            out.append(host.raw)
            self.lib.rt_free_device(0, d)
        self.bufs = []
        return out


def fresh(lib, scene, w, h, tiles=None, flags=0, n_frames=1):
    r = rt_host.Renderer(rt_host.flatten_scene(scene), 0, lib)
    try:
        f = Frames(lib, w, h, tiles or (h, 0, 1, 1), n_frames)
        f.render(r, flags)
        return f.read()[0]
    finally:
        r.close()


def oracle_gap(frame, scene, w, h):
    """(largest difference in LSB, fraction of channels that differ) of a whole RGBA8 frame against the C restatement."""
    ora = np.frombuffer(ou.c_oracle_render(rt_host.flatten_scene(scene), w, h), dtype=np.uint8).astype(np.int16)
    d = np.abs(np.frombuffer(frame, dtype=np.uint8).astype(np.int16) - ora)
    return int(d.max()), float((d > 0).mean())


def near_oracle(frame, scene, w, h):
    return oracle_gap(frame, scene, w, h)[0] <= 1
