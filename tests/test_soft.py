"""The soft trace in one launch on a CPU (include/rt_hip.h: rt_scene_trace_rays_soft_device, rt_soft_view_work_bytes,
rt_scene_trace_view_soft_device, rt_trace_rays_soft_recursive, rt_trace_view_soft): header and binding, every refusal of the entry
points before a device is touched, and the Python layer's argument plumbing - "wavefront" stays the default method, and a caller who
does not name a method reaches the calls it reached before.  None of it touches a device."""
import ctypes as C
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

import rt_host

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
INCLUDE = os.path.join(ROOT, "include")
RT_ERR_INVALID, RT_ERR_STATE = -1, -5
SYMBOLS = ("rt_scene_trace_rays_soft_device", "rt_soft_view_work_bytes", "rt_scene_trace_view_soft_device", "rt_trace_rays_soft_recursive",
           "rt_trace_view_soft")


def test_both_libraries_export_the_symbols(built):
    for path in (rt_host.LIB_PATH, rt_host.TEST_LIB_PATH):
        lib = C.CDLL(path)
        for name in SYMBOLS:
            assert hasattr(lib, name), (path, name)


def test_header_and_binding_agree(built, tmp_path):
    """The header compiles as C and as C++; the entry points have the stated types (a function-pointer assignment, as
    tests/test_relight.py checks the relit nodes'); the binding has the same arguments; the ABI version stays."""
    cc = shutil.which("gcc") or shutil.which("cc")
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cc, "a C compiler is needed (the oracle is built with one)"
    proto = ('#include "rt_hip.h"\n'
             'int (*dev)(rt_scene_dev *, const struct rt_lighting *, const double *, uint32_t, uint64_t, const double *, const uint32_t *, uint32_t, uint32_t, const rt_ray_outputs *, void *, rt_stats *) = rt_scene_trace_rays_soft_device;\n'
             'size_t (*bytes)(uint32_t, uint32_t) = rt_soft_view_work_bytes;\n'
             'int (*vdev)(rt_scene_dev *, const rt_view *, uint32_t, uint32_t, const struct rt_lighting *, const double *, uint32_t, uint32_t, const rt_ray_outputs *, void *, size_t, void *, rt_stats *) = rt_scene_trace_view_soft_device;\n'
             'int (*host)(const void *, size_t, const struct rt_lighting *, const double *, uint32_t, uint64_t, const double *, uint32_t, int, const rt_ray_outputs *, rt_stats *) = rt_trace_rays_soft_recursive;\n'
             'int (*vhost)(const void *, size_t, const rt_view *, uint32_t, uint32_t, const struct rt_lighting *, const double *, uint32_t, uint32_t, const rt_ray_outputs *, rt_stats *) = rt_trace_view_soft;\n'
             'char check[RT_ABI_VERSION == 2u ? 1 : -1];\n')
    (tmp_path / "proto.c").write_text(proto)
    subprocess.run([cc, "-Wall", "-Werror", "-I", INCLUDE, "-c", "-o", str(tmp_path / "proto_c.o"), str(tmp_path / "proto.c")], check=True)
    if cxx:
        (tmp_path / "proto.cpp").write_text(proto)
        subprocess.run([cxx, "-std=c++17", "-Wall", "-Werror", "-I", INCLUDE, "-c", "-o", str(tmp_path / "proto_cpp.o"), str(tmp_path / "proto.cpp")], check=True)
    assert rt_host.RT_ABI_VERSION == 2                      # an addition: the ABI version stays
    lib = rt_host.load_library()
    for name in SYMBOLS:
        assert getattr(lib, name).argtypes == rt_host.ABI[name][1]
    assert [len(rt_host.ABI[name][1]) for name in SYMBOLS] == [12, 2, 13, 11, 11]


def test_the_workspace_figure(built):
    lib = rt_host.load_library()
    assert rt_host.soft_view_work_bytes(96, 54, lib) == 96 * 54 * 48 == rt_host.view_work_bytes(96, 54, lib)
    assert rt_host.soft_view_work_bytes(0, 54, lib) == 0 and rt_host.soft_view_work_bytes(96, 0, lib) == 0
    assert rt_host.soft_view_work_bytes(2 ** 16, 2 ** 15, lib) == 0 and rt_host.soft_view_work_bytes(2 ** 16, 2 ** 15 - 1, lib) > 0


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
    words = np.zeros(n + 1, np.uint32)
    rgb, rgba = np.full((n * 4, 3), 7.0), np.full((n * 4, 4), 7, np.uint8)
    out = rt_host.RtRayOutputs(rgb.ctypes.data, rgba.ctypes.data, None)
    hits = (rt_host.RtHit * n)()
    good = dict(n_samples=4, n_offs=8, stride=1, reserved=0, base=0, light_radius=0.5)
    view = rt_host.view(rt_host.RT_VIEW_PINHOLE, (0, 1, 5), (1, 0, 0), (0, 1, 0), (0, 0, -1), 60)
    W, H = 5, 4
    work = 4096                                             # (an address: no device entry gets far enough to read it)

    def desc(**kw):
        f = dict(good, **kw)
        return A(f["n_samples"], f["n_offs"], f["stride"], f["reserved"], f["base"], f["light_radius"])

    def dev(a=None, d=offs.ctypes.data, levels=1, m=n, r=rays.ctypes.data, order=0, pix_base=0, segs=0, o=out):
        return lib.rt_scene_trace_rays_soft_device(None, C.byref(a) if a is not False else None, C.c_void_p(d), levels, m, C.c_void_p(r), C.c_void_p(order),
                                                   pix_base, segs, C.byref(o) if o is not None else None, None, None)

    def host(a=None, d=offs.ctypes.data, levels=1, m=n, r=rays.ctypes.data, segs=0, o=out, size=len(blob)):
        return lib.rt_trace_rays_soft_recursive(buf, size, C.byref(a) if a is not False else None, C.c_void_p(d), levels, m, C.c_void_p(r), segs, 0,
                                                C.byref(o) if o is not None else None, None)

    def vdev(a=None, d=offs.ctypes.data, v=view, w=W, h=H, levels=1, segs=0, o=out, wk=work, wb=48 * W * H):
        return lib.rt_scene_trace_view_soft_device(None, C.byref(v) if v is not None else None, w, h, C.byref(a) if a is not False else None, C.c_void_p(d),
                                                   levels, segs, C.byref(o) if o is not None else None, C.c_void_p(wk), wb, None, None)

    def vhost(a=None, d=offs.ctypes.data, v=view, w=W, h=H, levels=1, segs=0, o=out, size=len(blob)):
        return lib.rt_trace_view_soft(buf, size, C.byref(v) if v is not None else None, w, h, C.byref(a) if a is not False else None, C.c_void_p(d), levels, segs,
                                      C.byref(o) if o is not None else None, None)

    calls = {"device": dev, "host": host, "view device": vdev, "view host": vhost}
    for name, call in calls.items():
        # what rt_lighting_validate refuses of the description
        for kw, text in (({"n_samples": 0}, "n_samples 0"), ({"n_samples": 1025, "n_offs": 2000}, "n_samples 1025"), ({"n_offs": 3}, "n_offs 3"),
                         ({"n_offs": 65537}, "n_offs 65537"), ({"light_radius": -1.0}, "light_radius"), ({"light_radius": math.nan}, "light_radius"),
                         ({"light_radius": math.inf}, "light_radius"), ({"reserved": 1}, "reserved")):
            assert call(desc(**kw)) == RT_ERR_INVALID and text in err(), (name, kw, err())
        assert call(False) == RT_ERR_INVALID and "NULL" in err(), name
        assert call(desc(), d=0) == RT_ERR_INVALID and "NULL" in err(), name              # a table that would be read
        # the depth and the outputs: a NULL struct, both outputs NULL, hit records, alignment
        assert call(desc(), segs=17) == RT_ERR_INVALID and "segs 17" in err(), name
        assert call(desc(), o=None) == RT_ERR_INVALID and "NULL outputs" in err(), name
        assert call(desc(), o=rt_host.RtRayOutputs(None, None, None)) == RT_ERR_INVALID and "every output is NULL" in err(), name
        assert call(desc(), o=rt_host.RtRayOutputs(rgb.ctypes.data, None, C.addressof(hits))) == RT_ERR_INVALID and "no hit records" in err(), name
        assert call(desc(), o=rt_host.RtRayOutputs(rgb.ctypes.data + 4, None, None)) == RT_ERR_INVALID and "misaligned output" in err(), name
        assert call(desc(), o=rt_host.RtRayOutputs(None, rgba.ctypes.data + 2, None)) == RT_ERR_INVALID and "misaligned output" in err(), name
    # the list
    for name, call in (("device", dev), ("host", host)):
        assert call(desc(), m=0) == RT_ERR_INVALID and call(desc(), m=2 ** 31) == RT_ERR_INVALID and "2^31 - 1" in err(), name
        assert call(desc(), r=0) == RT_ERR_INVALID and "NULL" in err(), name
        assert call(desc(), r=rays.ctypes.data + 8) == RT_ERR_INVALID and "16" in err(), (name, err())
    # a table entry that is not finite: the entry points that see the table in host memory
    broken = offs.copy()
    broken[2, 1] = math.nan
    for call in (host, vhost):
        assert call(desc(), d=broken.ctypes.data) == RT_ERR_INVALID and "non-finite" in err()
    # the device entry's own: pix_base, the table's alignment, the order; then the scene
    assert dev(desc(), pix_base=2 ** 31 - n + 1) == RT_ERR_INVALID and "above 2^31" in err()
    assert dev(desc(), m=2 ** 31 - 1, pix_base=2) == RT_ERR_INVALID and "above 2^31" in err()
    assert dev(desc(), d=offs.ctypes.data + 4) == RT_ERR_INVALID and "misaligned" in err()
    assert dev(desc(), order=words.ctypes.data + 2) == RT_ERR_INVALID and "misaligned order" in err()
    assert dev(desc()) == RT_ERR_STATE and "NULL scene" in err()
    assert dev(desc(), pix_base=2 ** 31 - n, order=words.ctypes.data) == RT_ERR_STATE      # (pix_base + n == 2^31 is in range)
    assert dev(desc(light_radius=0.0), d=0) == RT_ERR_STATE                                # point lights read no table
    assert dev(desc(), levels=0, segs=16) == RT_ERR_STATE
    # the view entries': the view, its size, the workspace; then the scene
    bad_view = rt_host.view(rt_host.RT_VIEW_PINHOLE, (0, 1, 5), (1, 0, 0), (0, 1, 0), (0, 0, -1), 180)
    for name, call in (("view device", vdev), ("view host", vhost)):
        assert call(desc(), v=None) == RT_ERR_INVALID and "NULL view" in err(), name
        assert call(desc(), v=bad_view) == RT_ERR_INVALID and "fov_deg" in err(), name
        assert call(desc(), w=0) == RT_ERR_INVALID and call(desc(), w=2 ** 16, h=2 ** 15) == RT_ERR_INVALID, name
    assert vdev(desc(), wk=0) == RT_ERR_INVALID and "workspace" in err()
    assert vdev(desc(), wk=work + 8) == RT_ERR_INVALID and "workspace" in err()
    assert vdev(desc(), wb=48 * W - 1) == RT_ERR_INVALID and "below one row" in err()
    assert vdev(desc(), d=offs.ctypes.data + 4) == RT_ERR_INVALID and "misaligned" in err()
    assert vdev(desc()) == RT_ERR_STATE and "NULL scene" in err()
    assert vdev(desc(), wb=48 * W) == RT_ERR_STATE
    # the host forms': the blob
    assert host(desc(), size=len(blob) - 8) == RT_ERR_INVALID and vhost(desc(), size=len(blob) - 8) == RT_ERR_INVALID
    # with everything in order they fail loudly where there is no device (rt_init was not called) - also with no level to sample
    if lib.rt_device_count() < 0:
        assert host(desc()) == RT_ERR_STATE and vhost(desc()) == RT_ERR_STATE and host(desc(), levels=0) == RT_ERR_STATE
    assert (rgb == 7.0).all() and (rgba == 7).all()                                         # nothing was written


class Recorder:
    """The typed library with the soft entry points replaced by recorders: which one a wrapper reaches, and with what."""

    def __init__(self, lib):
        self._lib, self.calls = lib, []

    def __getattr__(self, name):
        if name in ("rt_trace_rays_soft", "rt_trace_rays_soft_recursive", "rt_trace_view_soft", "rt_scene_trace_rays_soft_device",
                    "rt_scene_trace_view_soft_device"):
            def record(*args):
                self.calls.append((name, args))
                return 0
            return record
        if name == "rt_init":
            return lambda *a: 0
        return getattr(self._lib, name)


def _value(x):
    return x.value if hasattr(x, "value") else x


def test_the_python_layers_plumbing(built, monkeypatch):
    lib = Recorder(rt_host.load_library())
    monkeypatch.setattr(rt_host, "_init_once", lambda lib: None)
    scene = rt_host.load_scene("h8")
    rays = np.arange(18, dtype=np.float64).reshape(3, 6)
    offs = rt_host.lighting_offsets(8)
    # wavefront is the default: without the keyword, today's call with today's arguments
    rt_host.trace_rays_soft(scene, rays, 4, 0.5, offs=offs, stride=3, levels=2, segs=5, order_levels=True, base=9, lib=lib)
    rt_host.trace_rays_soft(scene, rays, 4, 0.5, offs=offs, stride=3, levels=2, segs=5, order_levels=True, base=9, lib=lib, method="wavefront")
    assert [c[0] for c in lib.calls] == ["rt_trace_rays_soft"] * 2
    for name, a in lib.calls:
        assert len(a) == 12 and a[4] == 2 and a[5] == 3 and a[7] == 5 and a[8] == 1
        d = a[2]._obj
        assert (d.n_samples, d.n_offs, d.stride, d.reserved, d.base, d.light_radius) == (4, 8, 3, 0, 9, 0.5)
    lib.calls.clear()
    # the recursive method: the new host form, `order` as its binned flag
    for order, flag in (("list", 0), ("binned", 1)):
        out = rt_host.trace_rays_soft(scene, rays, 4, 0.5, offs=offs, stride=3, levels=2, segs=5, base=9, want=("rgb", "rgba"), lib=lib, method="recursive", order=order)
        name, a = lib.calls.pop()
        assert name == "rt_trace_rays_soft_recursive" and len(a) == 11 and a[4] == 2 and a[5] == 3 and a[7] == 5 and a[8] == flag
        d = a[2]._obj
        assert (d.n_samples, d.n_offs, d.stride, d.base, d.light_radius) == (4, 8, 3, 9, 0.5)
        assert out["rgb"].shape == (3, 3) and out["rgba"].shape == (3, 4) and "level_counts" not in out
        assert _value(a[6]) % 16 == 0
    # without a table: lighting_offsets(n_samples), stride 0
    rt_host.trace_rays_soft(scene, rays, 5, 0.5, stride=4, lib=lib, method="recursive")
    d = lib.calls.pop()[1][2]._obj
    assert (d.n_samples, d.n_offs, d.stride) == (5, 5, 0)
    # the view: the default makes its rays on the host and goes through the wavefront list call; "recursive" hands the view over
    v = rt_host.view(rt_host.RT_VIEW_PINHOLE, (0, 1, 5), (1, 0, 0), (0, 1, 0), (0, 0, -1), 60)
    rt_host.trace_view_soft(scene, v, 4, 3, 4, 0.5, offs=offs, levels=2, lib=lib)
    name, a = lib.calls.pop()
    assert name == "rt_trace_rays_soft" and a[5] == 12
    out = rt_host.trace_view_soft(scene, v, 4, 3, 4, 0.5, offs=offs, stride=3, levels=2, segs=5, lib=lib, method="recursive")
    name, a = lib.calls.pop()
    assert name == "rt_trace_view_soft" and len(a) == 11 and (a[3], a[4], a[7], a[8]) == (4, 3, 2, 5) and out["rgba"].shape == (12, 4)
    assert not lib.calls
    # the refusals of the layer itself
    for kw in (dict(method="fused"), dict(order="sorted"), dict(order="binned"), dict(method="recursive", order_levels=True),
               dict(method="recursive", want=("level_counts", "rgb")), dict(method="recursive", want=("hits",)), dict(method="recursive", levels=-1)):
        with pytest.raises(ValueError):
            rt_host.trace_rays_soft(scene, rays, 2, 0.5, lib=lib, **kw)
    for kw in (dict(method="fused"), dict(method="recursive", order_levels=True), dict(method="recursive", want=("level_counts",))):
        with pytest.raises(ValueError):
            rt_host.trace_view_soft(scene, v, 4, 3, 2, 0.5, lib=lib, **kw)
    assert not lib.calls
    import inspect
    assert inspect.signature(rt_host.trace_rays_soft).parameters["method"].default == "wavefront"
    assert inspect.signature(rt_host.trace_view_soft).parameters["method"].default == "wavefront"


def test_the_renderers_plumbing(built):
    """Renderer.trace_rays_soft / trace_view_soft hand their arguments to the device entry points in the stated places."""
    lib = Recorder(rt_host.load_library())
    r = rt_host.Renderer.__new__(rt_host.Renderer)
    r.lib, r.handle, r.device = lib, 0x1000, 0
    lib.rt_scene_free = lambda handle: 0                    # (the recorder's: the handle names no scene)
    r.trace_rays_soft(7, 0x100, 0x200, 0x300, 0x400, 8, 4, 0.5, stride=3, base=9, levels=2, segs=5, order_ptr=0x500, pix_base=11, stream=0x600)
    name, a = lib.calls.pop()
    assert name == "rt_scene_trace_rays_soft_device" and len(a) == 12
    assert (a[0], _value(a[2]), a[3], a[4], _value(a[5]), _value(a[6]), a[7], a[8], _value(a[10]), a[11]) == (0x1000, 0x400, 2, 7, 0x100, 0x500, 11, 5, 0x600, None)
    d = a[1]._obj
    assert (d.n_samples, d.n_offs, d.stride, d.reserved, d.base, d.light_radius) == (4, 8, 3, 0, 9, 0.5)
    o = a[9]._obj
    assert (o.rgb, o.rgba, o.hits) == (0x200, 0x300, None)
    v = rt_host.view(rt_host.RT_VIEW_PINHOLE, (0, 1, 5), (1, 0, 0), (0, 1, 0), (0, 0, -1), 60)
    r.trace_view_soft(v, 4, 3, 0, 0x300, 0x400, 8, 4, 0.5, 0x700, 576, levels=2, segs=5)
    name, a = lib.calls.pop()
    assert name == "rt_scene_trace_view_soft_device" and len(a) == 13
    assert (a[0], a[2], a[3], _value(a[5]), a[6], a[7], _value(a[9]), a[10], _value(a[11])) == (0x1000, 4, 3, 0x400, 2, 5, 0x700, 576, None)
    o = a[8]._obj
    assert (o.rgb, o.rgba, o.hits) == (None, 0x300, None)
    r.handle = None                                         # (a handle that names no scene: nothing to free)
