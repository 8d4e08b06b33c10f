"""Texel edits of a resident scene, the parts that need no GPU (include/rt_hip.h: rt_scene_set_texels, rt_scene_set_texels_device): the
declared and exported entry points, the argument checks that come before a device is touched, the blob diff rt_render's scene cache
turns into edits (csrc/rt_frame.hip: texel_edits, through the test library's rt_test_texel_edits) held to a numpy diff of the two
blobs, and the Python host's own size check.

The diff's rule for bytes no edit reaches - a descriptor, the padding between two textures: a difference there is -1, i.e. an upload
(the flatteners write zeros into the padding, so a blob that differs there was not made by one)."""
import ctypes as C
import os
import re
import struct

import numpy as np
import pytest

import rt_host
from lights_util import move_lights
from texels_util import INVALID, STATE, bind, descriptors, library_edits, numpy_edits, texture
from texture_util import texels, with_textures

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_texel_entry_points_are_declared_and_exported(built):
    header = open(os.path.join(ROOT, "include", "rt_hip.h")).read()
    args = (r"\(rt_scene_dev \*scene, uint32_t texture, uint32_t x, uint32_t y, uint32_t w, uint32_t h,\s+const void \*%s,\s+"
            r"size_t pitch_bytes, void \*hip_stream\);")
    assert re.search(r"int rt_scene_set_texels" + args % "rgba", header)
    assert re.search(r"int rt_scene_set_texels_device" + args % "d_rgba", header)
    assert re.search(r"#define RT_ABI_VERSION\s+2u?\b", header)                 # the blob does not change
    assert "rt_scene_set_texels" in rt_host.ABI and "rt_scene_set_texels_device" in rt_host.ABI
    lib, tlib = rt_host.load_library(), rt_host.load_library(rt_host.TEST_LIB_PATH)
    for x in (lib, tlib):
        assert hasattr(x, "rt_scene_set_texels") and hasattr(x, "rt_scene_set_texels_device")
    for hook in ("rt_test_scene_texels", "rt_test_texel_edits"):
        assert hasattr(tlib, hook) and not hasattr(lib, hook), hook


def test_the_checks_that_need_no_scene_come_first(built):
    """RT_ERR_INVALID for the source, the pitch and the alignment also with a NULL scene (nothing touches a device: this passes
    without one); a NULL scene with valid arguments is RT_ERR_STATE."""
    src = C.create_string_buffer(64)
    p = C.addressof(src)
    for path in (None, rt_host.TEST_LIB_PATH):
        lib = rt_host.load_library(path)
        for fn in (lib.rt_scene_set_texels, lib.rt_scene_set_texels_device):
            assert fn(None, 0, 0, 0, 2, 2, None, 0, None) == INVALID              # NULL source, a rectangle of four texels
            assert b"NULL source" in lib.rt_last_error()
            assert fn(None, 0, 0, 0, 4, 1, p, 12, None) == INVALID                # pitch below 4 * w
            assert fn(None, 0, 0, 0, 2, 2, p, 10, None) == INVALID                # pitch no multiple of 4
            assert b"pitch" in lib.rt_last_error()
            assert fn(None, 0, 0, 0, 2, 2, p, 0, None) == STATE                   # valid arguments: the NULL scene is what is wrong
            assert fn(None, 0, 0, 0, 2, 2, p, 16, None) == STATE
            assert fn(None, 0, 0, 0, 0, 0, None, 0, None) == STATE                # (an empty rectangle needs no source)
        aligned = (p + 15) & ~15
        for off in (1, 2, 3):
            assert lib.rt_scene_set_texels_device(None, 0, 0, 0, 2, 2, aligned + off, 0, None) == INVALID
            assert b"aligned" in lib.rt_last_error()
            assert lib.rt_scene_set_texels(None, 0, 0, 0, 2, 2, aligned + off, 0, None) == STATE     # host memory: any alignment
        assert lib.rt_scene_set_texels_device(None, 0, 0, 0, 2, 2, aligned + 4, 0, None) == STATE


# ------------------------------------------------------------------ the blob diff
@pytest.fixture(scope="module")
def tlib(built):
    return bind(rt_host.load_library(rt_host.TEST_LIB_PATH))


@pytest.fixture(scope="module")
def blob():
    return rt_host.flatten_scene(with_textures(rt_host.load_scene("h8"), 1))


def poke(blob, at):
    b = bytearray(blob)
    b[at] ^= 0x5A
    return bytes(b)


def texel(blob, k, x, y):
    w, _, off = descriptors(blob)[k]
    return off + (y * w + x) * 4


def check(tlib, a, b, want):
    assert numpy_edits(a, b) == want                          # (the expected list is the numpy diff's, spelled out)
    assert library_edits(tlib, a, b) == want


def test_equal_blobs_give_no_edit(tlib, blob):
    check(tlib, blob, bytes(blob), [])


def test_one_byte_in_the_first_row_of_the_first_texture(tlib, blob):
    check(tlib, blob, poke(blob, texel(blob, 0, 0, 0) + 2), [(0, 0, 1)])
    k = texture((257, 129))
    check(tlib, blob, poke(blob, texel(blob, k, 256, 0) + 3), [(k, 0, 1)])


def test_one_byte_in_the_last_row_of_the_last_texture(tlib, blob):
    w, h, _ = descriptors(blob)[15]
    check(tlib, blob, poke(blob, texel(blob, 15, w - 1, h - 1) + 3), [(15, h - 1, 1)])
    assert texel(blob, 15, w - 1, h - 1) + 4 == len(blob)                       # the blob's last texel


def test_two_textures_change_at_once(tlib, blob):
    a, b = texture((2, 16384)), texture((16384, 2))
    other = poke(poke(blob, texel(blob, a, 1, 16000)), texel(blob, b, 9000, 1) + 1)
    check(tlib, blob, other, sorted([(a, 16000, 1), (b, 1, 1)]))


def test_rows_3_and_11_give_one_range(tlib, blob):
    k = texture((31, 17))
    check(tlib, blob, poke(poke(blob, texel(blob, k, 30, 3)), texel(blob, k, 0, 11) + 1), [(k, 3, 9)])


def test_a_changed_descriptor_is_an_upload(tlib, blob):
    off, = struct.unpack_from("<Q", blob, 200)
    for at in (off, off + 4, off + 8, off + 16 * 15 + 1):                        # a width, a height, an offset, the last width
        assert library_edits(tlib, blob, poke(blob, at)) == -1
    assert library_edits(tlib, blob, poke(blob, 176)) == -1                     # n_textures


def test_a_changed_padding_byte_is_an_upload(tlib, blob):
    d = descriptors(blob)
    assert d[0][:2] == (1, 1) and d[1][2] == d[0][2] + 8                        # four bytes of texels, four of padding
    for at in range(d[0][2] + 4, d[0][2] + 8):
        assert library_edits(tlib, blob, poke(blob, at)) == -1
    # ... also together with a texel that changed
    assert library_edits(tlib, poke(blob, d[0][2]), poke(blob, d[0][2] + 5)) == -1


def test_camera_and_light_changes_beside_a_texel_change_give_the_same_list(tlib):
    s0 = with_textures(rt_host.load_scene("h8"), 1)
    s1 = move_lights(s0, 3)
    s1["camera"] = dict(s1["camera"], origin=[c + 0.25 for c in s1["camera"]["origin"]])
    s1["light_intensity"], s1["starsSeed"] = 31.5, 9
    k = texture((5, 3))
    s1["textures"][k]["texels"] = texels(5, 3, 77)
    a, b = rt_host.flatten_scene(s0), rt_host.flatten_scene(s1)
    assert a[:208] != b[:208]
    check(tlib, a, b, [(k, 0, 3)])
    s1["objects"][2]["origin"][0] += 0.5                                         # ... and a sphere
    check(tlib, a, rt_host.flatten_scene(s1), [(k, 0, 3)])
    s1["fovDeg"] = 50                                                            # but no field of the header that no edit reaches
    assert library_edits(tlib, a, rt_host.flatten_scene(s1)) == -1


# ------------------------------------------------------------------ the Python host
class _NoLibrary:
    def __getattr__(self, name):
        raise AssertionError("the library was called (%s) for an argument the host must refuse" % name)


def test_set_texels_refuses_texels_of_the_wrong_size_before_any_library_call(blob):
    r = rt_host.Renderer.__new__(rt_host.Renderer)          # no __init__: no library, no GPU
    r.lib, r.handle, r.blob = _NoLibrary(), None, blob
    k = texture((5, 3))
    assert r.texture_size(k) == (5, 3)
    for bad in (np.zeros((3, 5, 3), np.uint8), np.zeros((5, 3, 4), np.uint8), np.zeros((3, 5, 4), np.uint16), np.zeros((2, 5, 4), np.uint8),
                bytes(59), bytes(61), "texels", None, [0] * 60):
        with pytest.raises(ValueError):
            r.set_texels(k, bad)
    with pytest.raises(ValueError):
        r.set_texels(k, np.zeros((2, 2, 4), np.uint8), x=1, y=1)             # the default rectangle runs to the edges: 4 x 2
    with pytest.raises(ValueError):
        r.set_texels(k, bytes(16), width=2, height=2, pitch=6)
    with pytest.raises(ValueError):
        r.set_texels(k, bytes(15), width=2, height=2)
    for bad in (16, -1, True, None, 1.0):
        with pytest.raises(ValueError):
            r.set_texels(bad, bytes(4), width=1, height=1)
    with pytest.raises(ValueError):
        r.set_texels(k, bytes(4), x=-1, width=1, height=1)
