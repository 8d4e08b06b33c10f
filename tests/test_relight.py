"""Relit nodes on a CPU (include/rt_hip.h: rt_scene_relight_nodes_device, rt_relight_rays, rt_trace_rays_soft): header and binding,
every refusal of the three entry points before a device is touched, the Python layer's own refusals, and the yardstick's index and
fold (tests/relight_util.py) against their statements.  None of it touches a device."""
import ctypes as C
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

import relight_util as rl
import rt_host

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
INCLUDE = os.path.join(ROOT, "include")
RT_ERR_INVALID, RT_ERR_STATE = -1, -5
SYMBOLS = ("rt_scene_relight_nodes_device", "rt_relight_rays", "rt_trace_rays_soft")


def test_both_libraries_export_the_symbols(built):
    for path in (rt_host.LIB_PATH, rt_host.TEST_LIB_PATH):
        lib = C.CDLL(path)
        for name in SYMBOLS:
            assert hasattr(lib, name), (path, name)


def test_header_and_binding_agree(built, tmp_path):
    """The header compiles as C and as C++; the three entry points have the stated types (a function-pointer assignment, as
    tests/test_nodes.py checks the wavefront form's); the binding has the same arguments; the ABI version stays."""
    cc = shutil.which("gcc") or shutil.which("cc")
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cc, "a C compiler is needed (the oracle is built with one)"
    proto = ('#include "rt_hip.h"\n'
             'int (*dev)(rt_scene_dev *, const struct rt_lighting *, const double *, uint64_t, const double *, const uint32_t *, const uint32_t *, rt_node *, void *, rt_stats *) = rt_scene_relight_nodes_device;\n'
             'int (*host)(const void *, size_t, const struct rt_lighting *, const double *, uint64_t, const double *, const uint32_t *, const uint32_t *, int, rt_node *, rt_stats *) = rt_relight_rays;\n'
             'int (*soft)(const void *, size_t, const struct rt_lighting *, const double *, uint32_t, uint64_t, const double *, uint32_t, int, const rt_ray_outputs *, rt_stats *, uint64_t *) = rt_trace_rays_soft;\n'
             'int version = RT_ABI_VERSION == 2u ? 1 : -1;\nchar check[RT_ABI_VERSION == 2u ? 1 : -1];\n')
    (tmp_path / "proto.c").write_text(proto)
    subprocess.run([cc, "-Wall", "-Werror", "-I", INCLUDE, "-c", "-o", str(tmp_path / "proto_c.o"), str(tmp_path / "proto.c")], check=True)
    if cxx:
        (tmp_path / "proto.cpp").write_text(proto)
        subprocess.run([cxx, "-std=c++17", "-Wall", "-Werror", "-I", INCLUDE, "-c", "-o", str(tmp_path / "proto_cpp.o"), str(tmp_path / "proto.cpp")], check=True)
    assert rt_host.RT_ABI_VERSION == 2                      # an addition: the ABI version stays
    lib = rt_host.load_library()
    for name in SYMBOLS:
        assert getattr(lib, name).argtypes == rt_host.ABI[name][1]
    assert len(rt_host.ABI["rt_scene_relight_nodes_device"][1]) == 10 and len(rt_host.ABI["rt_relight_rays"][1]) == 11
    assert len(rt_host.ABI["rt_trace_rays_soft"][1]) == 12


def test_bad_arguments_are_refused_before_a_device_is_touched(built):
    lib = rt_host.load_library()
    err = lambda: lib.rt_last_error().decode()
    A = rt_host.RtLighting
    blob = rt_host.flatten_scene(rt_host.load_scene("h8"))
    buf = C.create_string_buffer(blob, len(blob))
    offs = rt_host.lighting_offsets(8)
    n = 5
    raw = np.zeros(6 * n + 4)
    rays = raw[(raw.ctypes.data >> 3) & 1:][:6 * n]        # on a 16-byte boundary
    rays[:] = 1.0
    nodes = np.zeros(n + 1, rt_host.NODE_DTYPE)
    nodes.view(np.uint8)[:] = 7
    words = np.zeros(n + 1, np.uint32)
    rgb, rgba = np.full((n, 3), 7.0), np.full((n, 4), 7, np.uint8)
    out = rt_host.RtRayOutputs(rgb.ctypes.data, rgba.ctypes.data, None)
    good = dict(n_samples=4, n_offs=8, stride=1, reserved=0, base=0, light_radius=0.5)

    def desc(**kw):
        f = dict(good, **kw)
        return A(f["n_samples"], f["n_offs"], f["stride"], f["reserved"], f["base"], f["light_radius"])

    def dev(a=None, d=offs.ctypes.data, m=n, r=rays.ctypes.data, order=0, pix=0, nd=nodes.ctypes.data, s=None):
        return lib.rt_scene_relight_nodes_device(s, C.byref(a) if a is not False else None, C.c_void_p(d), m, C.c_void_p(r), C.c_void_p(order), C.c_void_p(pix),
                                                 C.c_void_p(nd), None, None)

    def host(a=None, d=offs.ctypes.data, m=n, r=rays.ctypes.data, pix=0, path=0, nd=nodes.ctypes.data, size=len(blob)):
        return lib.rt_relight_rays(buf, size, C.byref(a) if a is not False else None, C.c_void_p(d), m, C.c_void_p(r), C.c_void_p(pix), C.c_void_p(path), 0,
                                   C.c_void_p(nd), None)

    def soft(a=None, d=offs.ctypes.data, levels=1, m=n, r=rays.ctypes.data, segs=0, o=out, size=len(blob)):
        return lib.rt_trace_rays_soft(buf, size, C.byref(a) if a is not False else None, C.c_void_p(d), levels, m, C.c_void_p(r), segs, 0,
                                      C.byref(o) if o is not None else None, None, None)

    calls = {"device": dev, "host": host, "soft": soft}
    for name, call in calls.items():
        # what rt_lighting_validate refuses of the description
        for kw, text in (({"n_samples": 0}, "n_samples 0"), ({"n_samples": 1025, "n_offs": 2000}, "n_samples 1025"), ({"n_offs": 3}, "n_offs 3"),
                         ({"n_offs": 65537}, "n_offs 65537"), ({"light_radius": -1.0}, "light_radius"), ({"light_radius": math.nan}, "light_radius"),
                         ({"light_radius": math.inf}, "light_radius"), ({"reserved": 1}, "reserved")):
            assert call(desc(**kw)) == RT_ERR_INVALID and text in err(), (name, kw, err())
        assert call(False) == RT_ERR_INVALID and "NULL" in err(), name
        assert call(desc(), d=0) == RT_ERR_INVALID and "NULL" in err(), name              # a table that would be read
        # the list
        assert call(desc(), m=0) == RT_ERR_INVALID and call(desc(), m=2 ** 31) == RT_ERR_INVALID, name
        assert call(desc(), r=0) == RT_ERR_INVALID and "NULL" in err(), name
        assert call(desc(), r=rays.ctypes.data + 8) == RT_ERR_INVALID and "16" in err(), (name, err())
    # a table entry that is not finite: the entry points that see the table in host memory
    broken = offs.copy()
    broken[2, 1] = math.nan
    for call in (host, soft):
        assert call(desc(), d=broken.ctypes.data) == RT_ERR_INVALID and "non-finite" in err()
    # the device entry's own: nodes, the table's alignment, order and pix; then the scene
    assert dev(desc(), nd=0) == RT_ERR_INVALID and "NULL" in err()
    assert dev(desc(), nd=nodes.ctypes.data + 4) == RT_ERR_INVALID and "misaligned nodes" in err()
    assert dev(desc(), d=offs.ctypes.data + 4) == RT_ERR_INVALID and "misaligned" in err()
    assert dev(desc(), order=words.ctypes.data + 2) == RT_ERR_INVALID and "misaligned order" in err()
    assert dev(desc(), pix=words.ctypes.data + 2) == RT_ERR_INVALID and "misaligned order or pix" in err()
    assert dev(desc()) == RT_ERR_STATE and "NULL scene" in err()
    assert dev(desc(), order=words.ctypes.data, pix=words.ctypes.data + 4) == RT_ERR_STATE
    assert dev(desc(light_radius=0.0), d=0) == RT_ERR_STATE                                # point lights read no table
    # the host forms': the blob, the nodes, pix and path, the outputs, the depth
    assert host(desc(), size=len(blob) - 8) == RT_ERR_INVALID and soft(desc(), size=len(blob) - 8) == RT_ERR_INVALID
    assert host(desc(), nd=0) == RT_ERR_INVALID and host(desc(), nd=nodes.ctypes.data + 4) == RT_ERR_INVALID
    assert host(desc(), pix=words.ctypes.data + 2) == RT_ERR_INVALID and host(desc(), path=words.ctypes.data + 2) == RT_ERR_INVALID
    assert soft(desc(), o=None) == RT_ERR_INVALID
    assert soft(desc(), o=rt_host.RtRayOutputs(None, None, None)) == RT_ERR_INVALID
    assert soft(desc(), segs=17) == RT_ERR_INVALID
    hits = (rt_host.RtHit * n)()
    assert soft(desc(), o=rt_host.RtRayOutputs(rgb.ctypes.data, None, C.addressof(hits))) == RT_ERR_INVALID and "no hit records" in err()
    # with everything in order they fail loudly where there is no device (rt_init was not called) - also with no level to relight
    if lib.rt_device_count() < 0:
        assert host(desc()) == RT_ERR_STATE and soft(desc()) == RT_ERR_STATE and soft(desc(), levels=0) == RT_ERR_STATE
    assert (nodes.view(np.uint8) == 7).all() and (rgb == 7.0).all() and (rgba == 7).all()   # nothing was written


def test_the_python_layer(built):
    scene = rt_host.load_scene("h8")
    rays = np.ones((3, 6))
    with pytest.raises(ValueError):
        rt_host.relight_rays(scene, rays[:0], 2, 0.5)
    with pytest.raises(ValueError):
        rt_host.relight_rays(scene, rays, 2, 0.5, order="sorted")
    with pytest.raises(ValueError):
        rt_host.relight_rays(scene, rays, 2, 0.5, pix=[0, 1])
    with pytest.raises(ValueError):
        rt_host.relight_rays(scene, rays, 2, 0.5, offs=np.zeros((4, 2)))
    with pytest.raises(ValueError):
        rt_host.trace_rays_soft(scene, rays, 2, 0.5, want=("hits",))
    with pytest.raises(ValueError):
        rt_host.trace_rays_soft(scene, rays, 2, 0.5, levels=-1)
    with pytest.raises(ValueError):
        rt_host.trace_rays_soft(scene, np.ones((3, 5)), 2, 0.5)


def test_the_yardsticks_index_and_fold():
    """entries() is the stated expression in unsigned 64-bit arithmetic (rt_ambient.h's amb_entry), wraps included; fold() adds in
    order and divides once; moved_scene() is one multiply and one add per component."""
    e = rl.entries(4, 7, 3, 2, 2 ** 63, pix=[0, 1, 5, 2 ** 32 - 1])
    for i, p in enumerate([0, 1, 5, 2 ** 32 - 1]):
        for s in range(3):
            assert e[i, s] == ((((2 ** 63 + p) * 2) % 2 ** 64 + s) % 2 ** 64) % 7
    assert rl.entries(3, 5, 5, 0, 99).tolist() == [[0, 1, 2, 3, 4]] * 3
    assert rl.entries(2, 8, 2, 1, 2 ** 64 - 1).tolist() == [[7, 0], [0, 1]]                 # (2^64 - 1) % 8 = 7, then the sum wraps to 0
    x = np.array([[0.1, 0.2, 0.3], [1e308, 1e308, -1e308]])
    assert rl.fold(x)[0] == ((0.1 + 0.2) + 0.3) / 3.0 and np.isinf(rl.fold(x)[1])
    s = rl.moved_scene({"lights": [[5, 10, 5]], "textures": []}, [0.1, 0.2, 0.3], 0.7)
    assert s["lights"] == [[5 + 0.7 * 0.1, 10 + 0.7 * 0.2, 5 + 0.7 * 0.3]]
    assert rl.moved_scene({"lights": [[5, 10, 5]], "textures": []}, None, 0.0)["lights"] == [[5.0, 10.0, 5.0]]
