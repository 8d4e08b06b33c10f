"""Views on a CPU (include/rt_hip.h: rt_view; csrc/rt_views.h): the host probe rt_view_rays - the restatement the GPU's generator is
held to - against values that never come from the header: the numpy restatements of tests/views_util.py, rt_host.primary_rays,
tools/panorama.py and Python's own sin / cos.  Every comparison is bitwise (float64 viewed as uint64).  No GPU."""
import ctypes as C
import math
import os
import shutil
import struct
import subprocess
import sys

import numpy as np
import pytest

import rt_host
import views_util as vu

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "html5-canvas-raytracer_amd", "csrc")
INCLUDE = os.path.join(HERE, "..", "include")
CXX = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("c++") or shutil.which("clang++")
sys.path.insert(0, os.path.join(HERE, "..", "tools"))

MODELS = [vu.REFERENCE, vu.PINHOLE, vu.ORTHO, vu.EQUIRECT]
FOV, SCALE = 52.0, 0.037
INVALID = -1


def oblique():
    return vu.look_at(*vu.OBLIQUE)


def make_view(model, w, h, cam=None, fov=FOV, scale=SCALE):
    o, ax, ay, az = cam or oblique()
    return rt_host.view(model, o, ax, ay, az, fov, scale, tables=rt_host.equirect_tables(w, h) if model == vu.EQUIRECT else None)


def restated(model, w, h, v, first_row=0, rows=None):
    lon, lat = getattr(v, "_tables", (None, None))
    return vu.rays(model, w, h, list(v.origin), list(v.axis_x), list(v.axis_y), list(v.axis_z), v.fov_deg, v.scale, lon, lat, first_row, rows)


@pytest.mark.parametrize("model", MODELS)
def test_the_probe_gives_the_restatements_bits(built, model):
    assert [sum(abs(c) > 0.05 for c in axis) for axis in oblique()[1:]] == [2, 3, 3]     # oblique: no axis is the world's (lookAt's axis_x has no y part)
    for w, h in vu.SIZES:
        v = make_view(model, w, h)
        got = rt_host.view_rays(v, w, h)
        assert got.shape == (w * h, 6)
        assert (vu.bits(got) == vu.bits(restated(model, w, h, v))).all(), (model, w, h)
    w, h, first, rows = vu.BAND
    v = make_view(model, w, h)
    band = rt_host.view_rays(v, w, h, first, rows)
    assert band.shape == (rows * w, 6)
    assert (vu.bits(band) == vu.bits(restated(model, w, h, v, first, rows))).all()
    assert (vu.bits(band) == vu.bits(rt_host.view_rays(v, w, h)[first * w:(first + rows) * w])).all()
    # 3x5 has the pixel whose X and Y are zero: a PINHOLE ray along axis_z, an ORTHO ray from the origin itself
    if model == vu.ORTHO:
        v = make_view(model, 3, 5)
        assert list(rt_host.view_rays(v, 3, 5)[2 * 3 + 1][:3]) == list(v.origin)


def test_reference_views_are_the_primary_rays(built):
    cams = []
    for name in ("default14", "h8"):
        s = rt_host.load_scene(name)
        cams.append((s, s["fovDeg"]))
    o, ax, ay, az = oblique()
    cams.append((dict(rt_host.load_scene("h8"), camera={"origin": o, "axisX": ax, "axisY": ay, "axisZ": az}, fovDeg=FOV), FOV))
    for scene, fov in cams:
        assert scene.get("supersample", 1) == 1
        cam = scene["camera"]
        v = rt_host.view(vu.REFERENCE, cam["origin"], cam["axisX"], cam["axisY"], cam["axisZ"], fov)
        for w, h in vu.SIZES:
            assert (vu.bits(rt_host.view_rays(v, w, h)) == vu.bits(rt_host.primary_rays(w, h, scene))).all(), (w, h)


def test_a_pinhole_is_the_reference_view_while_the_axes_are_the_worlds(built):
    """Origin 0 and axis k with its k-th component alone (the world's axes, any sign and length): q1's per-component sum has one
    non-zero term, the pinhole's has the same one, and adding zeros changes no bit - signs of zero included."""
    for ax, ay, az in [((-1, 0, 0), (0, 1, 0), (0, 0, -1)), ((2.5, 0, 0), (0, -0.75, 0), (0, 0, 1.25))]:
        a, b = (rt_host.view(m, (0, 0, 0), ax, ay, az, 60) for m in (vu.REFERENCE, vu.PINHOLE))
        for w, h in [(1, 1), (3, 5), (257, 3), (700, 9)]:
            assert (vu.bits(rt_host.view_rays(a, w, h)) == vu.bits(rt_host.view_rays(b, w, h))).all(), (ax, w, h)


def test_an_equirect_view_is_the_panorama_tools_rays(built):
    from panorama import panorama_rays
    w, h, eye = 64, 32, [0.5, 1.5, -2.0]
    lon, lat = vu.tables_numpy(w, h)
    tl, ta = rt_host.equirect_tables(w, h)                    # (aligned arrays, overwritten with numpy's values)
    tl[:], ta[:] = lon, lat
    v = rt_host.view(vu.EQUIRECT, eye, (1, 0, 0), (0, 1, 0), (0, 0, -1), tables=(tl, ta))
    assert (vu.bits(rt_host.view_rays(v, w, h)) == vu.bits(panorama_rays(w, h, eye))).all()


def test_the_librarys_tables_are_the_hosts_sines_and_cosines(built):
    """Both sides are the host's libm (Python's math.sin / math.cos call it), on the header's angle expressions in Python floats."""
    for w, h in [(1, 1), (64, 32), (257, 3), (700, 9)]:
        lon, lat = rt_host.equirect_tables(w, h)
        assert lon.shape == (2 * w,) and lat.shape == (2 * h,) and lon.ctypes.data % 16 == 0 and lat.ctypes.data % 16 == 0
        want_lon = [f(2.0 * math.pi * (x + 0.5) / w - math.pi) for x in range(w) for f in (math.sin, math.cos)]
        want_lat = [f(math.pi / 2.0 - math.pi * (y + 0.5) / h) for y in range(h) for f in (math.sin, math.cos)]
        assert (vu.bits(lon) == vu.bits(want_lon)).all() and (vu.bits(lat) == vu.bits(want_lat)).all(), (w, h)


def test_invalid_views_are_refused(built):
    lib = rt_host.load_library()
    w, h = 8, 4
    tables = rt_host.equirect_tables(w, h)

    def good(model):
        o, ax, ay, az = oblique()
        return rt_host.view(model, o, ax, ay, az, FOV, SCALE, tables=tables if model == vu.EQUIRECT else None)

    def refused(v, w=w, h=h, needle=None):
        out = np.zeros((max(w * h, 1) if w * h < (1 << 20) else 1, 6))
        assert lib.rt_view_validate(C.byref(v) if v is not None else None, w, h) == INVALID
        msg = lib.rt_last_error().decode()
        assert needle is None or needle in msg, msg
        assert lib.rt_view_rays(C.byref(v) if v is not None else None, w, h, 0, 0, C.c_void_p(out.ctypes.data)) == INVALID

    for model in MODELS:
        assert lib.rt_view_validate(C.byref(good(model)), w, h) == 0, lib.rt_last_error()
    refused(None, needle="NULL view")
    v = good(vu.PINHOLE); v.model = 4; refused(v, needle="model")
    v = good(vu.PINHOLE); v.reserved = 1; refused(v, needle="reserved")
    for bad_w, bad_h in [(0, 4), (8, 0), (1 << 16, 1 << 15), (0xFFFFFFFF, 0xFFFFFFFF)]:
        refused(good(vu.PINHOLE), bad_w, bad_h, needle="view size")
    assert lib.rt_view_validate(C.byref(good(vu.PINHOLE)), (1 << 16) - 1, 1 << 15) == 0           # 2^31 - 2^15 rays
    for field in ("origin", "axis_x", "axis_y", "axis_z"):
        for c, bad in [(0, math.nan), (1, math.inf), (2, -math.inf)]:
            v = good(vu.ORTHO); getattr(v, field)[c] = bad; refused(v, needle="non-finite")
    for model in (vu.REFERENCE, vu.PINHOLE):
        for fov in (0.0, -10.0, 180.0, 200.0, math.nan):
            v = good(model); v.fov_deg = fov; refused(v, needle="fov_deg")
    for model in (vu.ORTHO, vu.EQUIRECT):                          # ... which the other models do not read
        v = good(model); v.fov_deg = math.nan
        assert lib.rt_view_validate(C.byref(v), w, h) == 0
    for scale in (0.0, -1.0, math.inf, math.nan):
        v = good(vu.ORTHO); v.scale = scale; refused(v, needle="scale")
    v = good(vu.PINHOLE); v.scale = math.nan
    assert lib.rt_view_validate(C.byref(v), w, h) == 0
    for lon, lat in [(None, tables[1].ctypes.data), (tables[0].ctypes.data, None), (tables[0].ctypes.data + 8, tables[1].ctypes.data),
                     (tables[0].ctypes.data, tables[1].ctypes.data + 8)]:
        v = good(vu.EQUIRECT); v.lon, v.lat = lon, lat; refused(v, needle="tables")
    v = good(vu.PINHOLE); v.lon, v.lat = 8, 8                       # ... which the other models ignore
    assert lib.rt_view_validate(C.byref(v), w, h) == 0
    # the rows of rt_view_rays
    out = np.full((w * h + 1, 6), 7.0)
    v = good(vu.PINHOLE)
    assert lib.rt_view_rays(C.byref(v), w, h, 0, h, None) == INVALID
    for first, rows in [(0, h + 1), (h, 1), (1, h), (0xFFFFFFFF, 2)]:
        assert lib.rt_view_rays(C.byref(v), w, h, first, rows, C.c_void_p(out.ctypes.data)) == INVALID, (first, rows)
        assert "rows" in lib.rt_last_error().decode()
    assert lib.rt_view_rays(C.byref(v), w, h, h, 0, C.c_void_p(out.ctypes.data)) == 0
    assert lib.rt_view_rays(C.byref(v), w, h, 2, 0, C.c_void_p(out.ctypes.data)) == 0
    assert (out == 7.0).all()                                      # rows == 0 writes nothing
    assert lib.rt_view_rays(C.byref(v), w, h, 0, h, C.c_void_p(out.ctypes.data)) == 0
    assert (out[:-1] != 7.0).any(axis=1).all() and (out[-1] == 7.0).all()


def test_a_zero_axis_is_a_valid_view(built):
    lib = rt_host.load_library()
    for model in MODELS:
        v = make_view(model, 5, 3)
        v.axis_x[:] = [0.0, 0.0, 0.0]
        assert lib.rt_view_validate(C.byref(v), 5, 3) == 0
        got = rt_host.view_rays(v, 5, 3)
        assert np.isfinite(got).all() and (vu.bits(got) == vu.bits(restated(model, 5, 3, v))).all()
    z = rt_host.view(vu.PINHOLE, (1, 2, 3), (0, 0, 0), (0, 0, 0), (0, 0, 0))
    assert lib.rt_view_validate(C.byref(z), 5, 3) == 0
    got = rt_host.view_rays(z, 5, 3)                               # normal3D leaves the zero vector as it is
    assert (got[:, :3] == [1, 2, 3]).all() and (got[:, 3:] == 0).all()


def test_work_bytes(built):
    lib = rt_host.load_library()
    for w, h in [(0, 4), (8, 0), (1 << 16, 1 << 15), (0xFFFFFFFF, 0xFFFFFFFF)]:
        assert lib.rt_view_work_bytes(w, h) == 0
    for w, h in [(1, 1), (64, 48), (3840, 2160), (1, 70000), (3_000_000, 3), ((1 << 16) - 1, 1 << 15)]:
        b = rt_host.view_work_bytes(w, h)
        assert b >= 48 * w and b % (48 * w) == 0 and b <= 48 * w * h, (w, h, b)      # whole rows: at least one, at most the view's


def test_cube_views(built):
    """Six pinholes of 90 degrees.  At an odd size the centre pixel has X == Y == 0, so its direction is axis_z * proj_d through
    normal3D: per component f * p * (1 / sqrt(p p)) with p = proj_d - the face's own axis, up to the last bit of p * (1 / p) and the
    sign of a zero."""
    eye, n = [0.25, -1.5, 3.0], 5
    views = rt_host.cube_views(eye)
    want = [(1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1)]
    p = vu.proj_d(90.0, n)
    one = p * (1.0 / math.sqrt(p * p))
    assert abs(one - 1.0) <= 2.0 ** -52
    for v, f in zip(views, want):
        assert v.model == vu.PINHOLE and v.fov_deg == 90.0 and list(v.origin) == eye and tuple(v.axis_z) == f
        ax, ay, az = (np.array(list(a)) for a in (v.axis_x, v.axis_y, v.axis_z))
        assert (np.cross(az, ay) == ax).all()                                   # right = forward x up
        centre = rt_host.view_rays(v, n, n)[(n // 2) * n + n // 2]
        assert list(centre[:3]) == eye
        assert (vu.bits(np.abs(centre[3:])) == vu.bits(np.abs(np.array(f, np.float64) * one))).all(), (f, centre)
        assert all(math.copysign(1.0, c) == k for c, k in zip(centre[3:], f) if k != 0)


def test_stereo_views(built):
    o, ax, ay, az = oblique()
    ax = [3.0 * c for c in ax]                                      # not a unit vector: the eyes move along unit(axis_x)
    tables = rt_host.equirect_tables(8, 4)
    for model in MODELS:
        v = rt_host.view(model, o, ax, ay, az, FOV, SCALE, tables=tables if model == vu.EQUIRECT else None)
        sep = 0.065
        left, right = rt_host.stereo_views(v, sep)
        u = vu.unit_rows(np.array(ax, np.float64))
        for c in range(3):
            assert left.origin[c] == o[c] - float(u[c]) * (sep / 2.0) and right.origin[c] == o[c] + float(u[c]) * (sep / 2.0)
        for e in (left, right):
            assert bytes(e)[104:] == bytes(v)[104:] and bytes(e)[:8] == bytes(v)[:8] and bytes(e)[32:104] == bytes(v)[32:104]
        d = np.array(list(right.origin)) - np.array(list(left.origin))
        assert abs(np.linalg.norm(d) - sep) < 1e-15 and abs(float(d @ u) - sep) < 1e-15
        assert list(v.origin) == o                                  # the view itself is left as it was


@pytest.mark.skipif(CXX is None, reason="no host C++ compiler")
def test_the_header_compiles_without_hip_and_gives_the_probes_bits(built, tmp_path):
    exe = str(tmp_path / "views_check")
    subprocess.run([CXX, "-std=c++17", "-O1", "-ffp-contract=off", "-Wall", "-Werror", "-Wno-unused-function", "-I" + CSRC, "-I" + INCLUDE,
                    os.path.join(HERE, "host", "views_check.cpp"), "-o", exe], check=True)
    o, ax, ay, az = oblique()
    cases = [(m, w, h, 0, h) for m in MODELS for w, h in vu.SIZES] + [(m,) + vu.BAND for m in MODELS]
    blob = b""
    for m, w, h, first, rows in cases:
        lon, lat = rt_host.equirect_tables(w, h)
        blob += struct.pack("<6I14d", m, w, h, first, rows, 0, FOV, SCALE, *o, *ax, *ay, *az) + lon.tobytes() + lat.tobytes()
    (tmp_path / "in.bin").write_bytes(blob)
    subprocess.run([exe, str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], check=True)
    got = np.fromfile(str(tmp_path / "out.bin"), np.float64)
    at = 0
    for m, w, h, first, rows in cases:
        want = rt_host.view_rays(make_view(m, w, h), w, h, first, rows).reshape(-1)
        assert (vu.bits(got[at:at + want.size]) == vu.bits(want)).all(), (m, w, h, first, rows)
        at += want.size
    assert at == got.size
