"""TEST INFRASTRUCTURE for the texel edits of a resident scene (tests/test_texels.py, tests/test_gpu_texels.py): where a blob keeps
its textures, texel edits done in numpy on a scene dict (the expected values: a fresh upload of the edited scene never runs the code
under test), and the two hooks of the test library (rt_test_scene_texels, rt_test_texel_edits)."""
import copy
import ctypes as C
import struct

import numpy as np

import rt_host
from texture_util import SHAPES, texels

N_TEXTURES_OFFSET, TEXTURES_OFFSET_OFFSET = 176, 200        # in rt_scene_header (include/rt_hip.h)
OK, INVALID, STATE = 0, -1, -5


def texture(shape):
    """The index of the texture of this (width, height) among texture_util.SHAPES."""
    return SHAPES.index(shape)


def descriptors(blob):
    """[(width, height, texels_offset)] of a blob."""
    n, = struct.unpack_from("<I", blob, N_TEXTURES_OFFSET)
    off, = struct.unpack_from("<Q", blob, TEXTURES_OFFSET_OFFSET)
    return [struct.unpack_from("<IIQ", blob, off + rt_host.TEXDESC_BYTES * k) for k in range(n)]


def first_texel(blob):
    d = descriptors(blob)
    return min(o for _, _, o in d) if d else len(blob)


def texel_bytes(scene):
    """What a fresh upload of `scene` holds from its first texel to the end of its blob."""
    blob = scene if isinstance(scene, (bytes, bytearray)) else rt_host.flatten_scene(scene)
    return bytes(blob[first_texel(blob):])


def rows_of(w, h, seed, pitch=0):
    """h source rows of w texels (texture_util.texels) as bytes: packed, or `pitch` bytes apart with 0xEE between the rows (bytes an
    edit must not store) - the last row ends with its texels."""
    t = np.frombuffer(texels(w, h, seed), np.uint8).reshape(h, 4 * w)
    if pitch in (0, 4 * w):
        return t.tobytes()
    out = np.full((h, pitch), 0xEE, np.uint8)
    out[:, :4 * w] = t
    return out.tobytes()[:(h - 1) * pitch + 4 * w]


def edited(scene, k, x, y, w, h, seed):
    """A copy of `scene` (texture dicts shared but for texture k) in which the rectangle of texture k holds texels(w, h, seed)."""
    s = dict(scene)
    s["textures"] = list(scene["textures"])
    t = dict(s["textures"][k])
    a = np.frombuffer(t["texels"], np.uint8).reshape(t["height"], t["width"], 4).copy()
    a[y:y + h, x:x + w] = np.frombuffer(texels(w, h, seed), np.uint8).reshape(h, w, 4)
    t["texels"] = a.tobytes()
    s["textures"][k] = t
    return s


def with_texels(scene, k, data):
    """A copy of `scene` whose texture k holds `data` (bytes of its own size)."""
    s = dict(scene)
    s["textures"] = list(scene["textures"])
    assert len(data) == len(s["textures"][k]["texels"])
    s["textures"][k] = dict(s["textures"][k], texels=bytes(data))
    return s


def bind(lib):
    lib.rt_test_scene_texels.restype = C.c_longlong
    lib.rt_test_scene_texels.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
    lib.rt_test_texel_edits.restype = C.c_int
    lib.rt_test_texel_edits.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_uint32), C.c_uint32]
    return lib


def scene_texels(lib, r):
    """The resident scene's bytes from its first texel to the end of its blob (the device is drained first)."""
    n = lib.rt_test_scene_texels(r.handle, None, 0)
    assert n >= 0, lib.rt_last_error()
    buf = C.create_string_buffer(max(n, 1))
    assert lib.rt_test_scene_texels(r.handle, buf, n) == n, lib.rt_last_error()
    return buf.raw[:n]


def library_edits(lib, a, b, cap=16):
    """rt_test_texel_edits(a, b): a list of (texture, first_row, rows), or -1."""
    assert len(a) == len(b)
    out = (C.c_uint32 * (3 * cap))()
    n = lib.rt_test_texel_edits(C.create_string_buffer(bytes(a), len(a)), C.create_string_buffer(bytes(b), len(b)), len(a), out, cap)
    return n if n < 0 else [tuple(out[3 * i:3 * i + 3]) for i in range(n)]


def numpy_edits(a, b):
    """The same list from a numpy diff of the texel ranges of two blobs with equal descriptors."""
    out = []
    for k, (w, h, off) in enumerate(descriptors(a)):
        ra = np.frombuffer(a, np.uint8, w * h * 4, off).reshape(h, 4 * w)
        rb = np.frombuffer(b, np.uint8, w * h * 4, off).reshape(h, 4 * w)
        rows = np.nonzero((ra != rb).any(axis=1))[0]
        if len(rows):
            out.append((k, int(rows[0]), int(rows[-1]) - int(rows[0]) + 1))
    return out


def deep(scene):
    return copy.deepcopy(scene)
