"""Gathered light on a CPU (include/rt_hip.h: struct rt_gather): header and binding, the exported symbols, and every refusal, none of
which touches a device.  The segment of (receiver, sample) is csrc/rt_ambient.h's, unchanged and held to its restatement by
tests/test_ambient.py; the tree walk moved into csrc/rt_soft_walk.h without touching that header.  No GPU."""
import ctypes as C
import math
import shutil
import subprocess

import numpy as np
import pytest

import ambient_util as au
import rt_host
from test_ambient import INCLUDE, RT_ERR_INVALID, RT_ERR_STATE

SYMBOLS = ("rt_gather_validate", "rt_scene_gather_device", "rt_gather", "rt_gather_view_work_bytes", "rt_scene_gather_view_device", "rt_gather_view")
RT_MAX_SEGS = 16


def test_both_libraries_export_the_symbols(built):
    for path in (rt_host.LIB_PATH, rt_host.TEST_LIB_PATH):
        lib = C.CDLL(path)
        for name in SYMBOLS:
            assert hasattr(lib, name), (path, name)


def test_header_and_binding_agree(built, tmp_path):
    """A C compiler takes the header - the struct tag rt_gather beside the function rt_gather - and the prototypes; the description is 32
    bytes without padding, as the binding lays it out; the ABI version stays."""
    cc = shutil.which("gcc") or shutil.which("cc")
    assert cc, "a C compiler is needed (the oracle is built with one)"
    proto = tmp_path / "proto.c"
    proto.write_text('#include "rt_hip.h"\n'
                     'int (*val)(const struct rt_gather *, const double *) = rt_gather_validate;\n'
                     'int (*host)(const void *, size_t, const struct rt_gather *, const double *, uint64_t, const rt_hit *, const rt_gather_outputs *, rt_stats *) = rt_gather;\n'
                     'int (*dev)(rt_scene_dev *, const struct rt_gather *, const double *, uint64_t, const rt_hit *, const uint32_t *, const rt_gather_outputs *, void *, rt_stats *) = rt_scene_gather_device;\n'
                     'size_t (*wb)(uint32_t, uint32_t) = rt_gather_view_work_bytes;\n'
                     'int (*viewd)(rt_scene_dev *, const rt_view *, uint32_t, uint32_t, const struct rt_gather *, const double *, const rt_gather_outputs *, void *, size_t, void *, rt_stats *) = rt_scene_gather_view_device;\n'
                     'int (*view)(const void *, size_t, const rt_view *, uint32_t, uint32_t, const struct rt_gather *, const double *, const rt_gather_outputs *, rt_stats *) = rt_gather_view;\n')
    subprocess.run([cc, "-Wall", "-Werror", "-I", INCLUDE, "-c", "-o", str(tmp_path / "proto.o"), str(proto)], check=True)
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "rt_hip.h"\n'
                   'int main(void) { printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %u %u\\n", sizeof(struct rt_gather), offsetof(struct rt_gather, n_samples), '
                   'offsetof(struct rt_gather, n_dirs), offsetof(struct rt_gather, stride), offsetof(struct rt_gather, segs), offsetof(struct rt_gather, base), '
                   'offsetof(struct rt_gather, pix_base), offsetof(struct rt_gather, pix_stride), sizeof(rt_gather_outputs), offsetof(rt_gather_outputs, rgb), '
                   'offsetof(rt_gather_outputs, rgba), RT_ABI_VERSION, RT_MAX_SEGS); return 0; }\n')
    exe = tmp_path / "layout"
    subprocess.run([cc, "-Wall", "-Werror", "-I", INCLUDE, "-o", str(exe), str(src)], check=True)
    got = [int(x) for x in subprocess.check_output([str(exe)], text=True).split()]
    a = [C.sizeof(rt_host.RtGather)] + [getattr(rt_host.RtGather, f).offset for f, _ in rt_host.RtGather._fields_]
    o = [C.sizeof(rt_host.RtGatherOutputs)] + [getattr(rt_host.RtGatherOutputs, f).offset for f, _ in rt_host.RtGatherOutputs._fields_]
    assert got[:8] == a == [32, 0, 4, 8, 12, 16, 24, 28]
    assert sum(C.sizeof(t) for _, t in rt_host.RtGather._fields_) == 32                       # no hidden padding
    assert got[8:11] == o == [16, 0, 8]
    assert got[11] == 2 == rt_host.RT_ABI_VERSION          # an addition: the ABI version stays
    assert got[12] == RT_MAX_SEGS
    lib = rt_host.load_library()
    for name in SYMBOLS:
        assert getattr(lib, name).argtypes == rt_host.ABI[name][1] and getattr(lib, name).restype == rt_host.ABI[name][0]


def test_bad_arguments_are_refused_before_a_device_is_touched(built):
    lib = rt_host.load_library()
    err = lambda: lib.rt_last_error().decode()
    A, O = rt_host.RtGather, rt_host.RtGatherOutputs
    blob = rt_host.flatten_scene(rt_host.load_scene("h8"))
    buf = C.create_string_buffer(blob, len(blob))
    dirs = rt_host.ambient_dirs(8)
    hits = au.hand_built()
    n = len(hits)
    rgb, rgba, order = np.full(3 * n + 1, 7.0), np.full(n + 1, 7, np.uint32), np.zeros(n + 1, np.uint32)
    raw = np.zeros(6 * n + 4)
    aligned = raw[(raw.ctypes.data >> 3) & 1:][:6 * n]
    good_out = O(rgb.ctypes.data, rgba.ctypes.data)
    good = dict(n_samples=4, n_dirs=8, stride=1, segs=0, base=0, pix_base=0, pix_stride=n)
    view = rt_host.view(rt_host.RT_VIEW_PINHOLE, [0, 1, 5], [1, 0, 0], [0, 1, 0], [0, 0, -1], 60)

    def desc(**kw):
        f = dict(good, **kw)
        return A(f["n_samples"], f["n_dirs"], f["stride"], f["segs"], f["base"], f["pix_base"], f["pix_stride"])

    calls = {
        "validate": lambda a, d=dirs.ctypes.data: lib.rt_gather_validate(C.byref(a), C.c_void_p(d)),
        "host": lambda a, d=dirs.ctypes.data: lib.rt_gather(buf, len(blob), C.byref(a), C.c_void_p(d), n, C.c_void_p(hits.ctypes.data), C.byref(good_out), None),
        "view": lambda a, d=dirs.ctypes.data: lib.rt_gather_view(buf, len(blob), C.byref(view), 4, 3, C.byref(a), C.c_void_p(d), C.byref(good_out), None),
        "device": lambda a, d=dirs.ctypes.data: lib.rt_scene_gather_device(None, C.byref(a), C.c_void_p(d), n, C.c_void_p(hits.ctypes.data), None, C.byref(good_out), None, None),
        "view_device": lambda a, d=dirs.ctypes.data: lib.rt_scene_gather_view_device(C.c_void_p(1), C.byref(view), 4, 3, C.byref(a), C.c_void_p(d), C.byref(good_out),
                                                                                     C.c_void_p(aligned.ctypes.data), 10 ** 6, None, None),
    }
    for name, call in calls.items():
        # what rt_ambient_validate refuses of the shared fields, and the depth
        for kw, text in (({"n_samples": 0}, "n_samples 0"), ({"n_samples": 1025, "n_dirs": 2000}, "n_samples 1025"), ({"n_dirs": 3}, "n_dirs 3"),
                         ({"n_dirs": 65537}, "n_dirs 65537"), ({"segs": RT_MAX_SEGS + 1}, "segs 17"), ({"segs": 2 ** 32 - 1}, "segs 4294967295")):
            assert call(desc(**kw)) == RT_ERR_INVALID and text in err(), (name, kw, err())
        assert call(desc(), 0) == RT_ERR_INVALID and "NULL" in err(), name
    # a table entry that is not finite: the entry points that see the table in host memory
    for bad in (math.nan, math.inf, -math.inf):
        for at in (0, 23):
            broken = dirs.copy()
            broken.reshape(-1)[at] = bad
            for name in ("validate", "host", "view"):
                assert calls[name](desc(), broken.ctypes.data) == RT_ERR_INVALID and "non-finite" in err(), (name, bad, at)
            # ... but not an entry past n_dirs
            assert lib.rt_gather_validate(C.byref(desc(n_dirs=7, n_samples=4)), C.c_void_p(broken.ctypes.data)) == (0 if at == 23 else RT_ERR_INVALID)
    for ok in (desc(), desc(segs=RT_MAX_SEGS), desc(segs=1), desc(n_samples=8, stride=0), desc(n_samples=1024, n_dirs=65536, base=2 ** 64 - 1), desc(pix_stride=0)):
        table = rt_host.ambient_dirs(ok.n_dirs)
        assert lib.rt_gather_validate(C.byref(ok), C.c_void_p(table.ctypes.data)) == 0
    assert lib.rt_gather_validate(None, C.c_void_p(dirs.ctypes.data)) == RT_ERR_INVALID

    # the device form's: the count, the bound on pix at its edge and one past it, pointers, alignment, outputs, order; then the scene
    dev = lambda a=desc(), o=good_out, m=n, h=hits.ctypes.data, d=dirs.ctypes.data, order=0: lib.rt_scene_gather_device(
        None, C.byref(a), C.c_void_p(d), m, C.c_void_p(h), C.c_void_p(order), C.byref(o) if o is not None else None, None, None)
    assert dev(m=0) == RT_ERR_INVALID and "n 0" in err()
    assert dev(m=2 ** 31, a=desc(pix_stride=0)) == RT_ERR_INVALID and "n 2147483648" in err()
    # pix_base + (n_samples - 1) * pix_stride + n against 2^31: 3 pix_stride + pix_base + 6
    for pb, ps, fits in ((2 ** 31 - 6, 0, True), (2 ** 31 - 5, 0, False), (0, (2 ** 31 - 6) // 3, True), (2, (2 ** 31 - 6) // 3, True), (3, (2 ** 31 - 6) // 3, False),
                         (2 ** 32 - 1, 0, False), (0, 2 ** 32 - 1, False), (2 ** 32 - 1, 2 ** 32 - 1, False)):
        assert 3 * ((2 ** 31 - 6) // 3) + 2 + n == 2 ** 31 and n == 6
        rc = dev(a=desc(pix_base=pb, pix_stride=ps))
        assert rc == (RT_ERR_STATE if fits else RT_ERR_INVALID), (pb, ps, err())
        assert ("NULL scene" if fits else "above 2^31") in err(), (pb, ps, err())
    assert dev(a=desc(n_samples=1, n_dirs=1, pix_base=0, pix_stride=2 ** 32 - 1)) == RT_ERR_STATE      # (one sample: the stride is not used)
    assert dev(m=2 ** 31 - 1, a=desc(pix_base=1, pix_stride=0)) == RT_ERR_STATE and dev(m=2 ** 31 - 1, a=desc(pix_base=2, pix_stride=0)) == RT_ERR_INVALID
    assert dev(o=None) == RT_ERR_INVALID and "NULL outputs" in err()
    assert dev(o=O(None, None)) == RT_ERR_INVALID and "every output is NULL" in err()
    assert dev(o=O(rgb.ctypes.data + 4, None)) == RT_ERR_INVALID and "misaligned output" in err()
    assert dev(o=O(None, rgba.ctypes.data + 2)) == RT_ERR_INVALID and "misaligned output" in err()
    assert dev(h=0) == RT_ERR_INVALID and dev(h=hits.ctypes.data + 4) == RT_ERR_INVALID and "misaligned" in err()
    assert dev(d=0) == RT_ERR_INVALID and dev(d=dirs.ctypes.data + 4) == RT_ERR_INVALID and "misaligned" in err()
    assert dev(order=order.ctypes.data + 2) == RT_ERR_INVALID and "misaligned order" in err()
    for o in (good_out, O(rgb.ctypes.data, None), O(None, rgba.ctypes.data)):
        assert dev(o=o) == RT_ERR_STATE and "NULL scene" in err()
    assert dev(order=order.ctypes.data) == RT_ERR_STATE

    viewd = lambda a=desc(), s=1, w=4, wb=10 ** 6, wk=aligned.ctypes.data, o=good_out, d=dirs.ctypes.data: lib.rt_scene_gather_view_device(
        C.c_void_p(s), C.byref(view), w, 3, C.byref(a), C.c_void_p(d), C.byref(o), C.c_void_p(wk), wb, None, None)
    assert viewd(s=0) == RT_ERR_STATE and "NULL scene" in err()
    assert viewd(w=0) == RT_ERR_INVALID
    assert viewd(a=desc(pix_base=2 ** 31 - 11, pix_stride=0)) == RT_ERR_INVALID and "above 2^31" in err()      # n = w h = 12
    assert viewd(wb=4 * 128 - 1) == RT_ERR_INVALID and "below one row" in err()
    assert viewd(wk=0) == RT_ERR_INVALID and viewd(wk=aligned.ctypes.data + 8) == RT_ERR_INVALID and "workspace" in err()
    assert viewd(o=O(None, None)) == RT_ERR_INVALID and "every output is NULL" in err()
    assert viewd(d=dirs.ctypes.data + 4) == RT_ERR_INVALID and "misaligned" in err()

    # the host forms': the blob, the count and the bound, the records, the outputs
    host = lambda a=desc(), nbytes=len(blob), m=n, h=hits.ctypes.data, o=good_out: lib.rt_gather(buf, nbytes, C.byref(a), C.c_void_p(dirs.ctypes.data), m, C.c_void_p(h),
                                                                                                   C.byref(o) if o is not None else None, None)
    assert host(nbytes=len(blob) - 8) == RT_ERR_INVALID
    assert host(m=0) == RT_ERR_INVALID and host(m=2 ** 31, a=desc(pix_stride=0)) == RT_ERR_INVALID
    assert host(a=desc(pix_base=2 ** 31 - 5, pix_stride=0)) == RT_ERR_INVALID and "above 2^31" in err()
    assert host(h=0) == RT_ERR_INVALID and host(o=None) == RT_ERR_INVALID and host(o=O(None, None)) == RT_ERR_INVALID
    none = O(None, None)
    assert lib.rt_gather_view(buf, len(blob), C.byref(view), 4, 3, C.byref(desc()), C.c_void_p(dirs.ctypes.data), C.byref(none), None) == RT_ERR_INVALID
    assert lib.rt_gather_view(buf, len(blob), C.byref(view), 0, 3, C.byref(desc()), C.c_void_p(dirs.ctypes.data), C.byref(good_out), None) == RT_ERR_INVALID
    assert lib.rt_gather_view(buf, len(blob), C.byref(view), 4, 3, C.byref(desc(pix_base=2 ** 31 - 11, pix_stride=0)), C.c_void_p(dirs.ctypes.data), C.byref(good_out),
                              None) == RT_ERR_INVALID and "above 2^31" in err()
    assert rt_host.gather_view_work_bytes(4, 3) == 4 * 3 * 128 and rt_host.gather_view_work_bytes(0, 3) == 0 and rt_host.gather_view_work_bytes(65536, 65536) == 0
    assert (rgb == 7.0).all() and (rgba == 7).all() and (order == 0).all()       # nothing was written


def test_the_python_layer(built):
    scene = rt_host.load_scene("h8")
    with pytest.raises(ValueError):
        rt_host.gather(scene, au.hand_built(), 4, want=("open",))
    with pytest.raises(ValueError):
        rt_host.gather(scene, au.hand_built(), 4, want=())
    with pytest.raises(ValueError):
        rt_host.gather(scene, au.hand_built(), 4, dirs=np.zeros((4, 2)))
    with pytest.raises(ValueError):
        rt_host.gather(scene, au.hand_built()[:0], 4)
    # pix_stride None is the list's length, and the view's w h
    a, _ = rt_host._gather_args(6, 4, None, 1, 0, 0, 0, None, rt_host.load_library())
    assert (a.n_samples, a.n_dirs, a.pix_stride) == (4, 4, 6)
    a, _ = rt_host._gather_args(6, 4, rt_host.ambient_dirs(9), 3, 2, 2 ** 40, 5, 0, rt_host.load_library())
    assert (a.n_dirs, a.stride, a.segs, a.base, a.pix_base, a.pix_stride) == (9, 3, 2, 2 ** 40, 5, 0)


def test_the_gpu_cases_inputs_wrap_the_table_and_mix_the_records(built):
    """What tests/test_gpu_gather.py relies on and a CPU can say: the hand-built records hold scanned receivers (one inside a sphere), a
    miss and two records with a non-finite word; the walk (16, 64, 7) over 5 184 receivers reaches every entry and wraps; a base of
    2^40 + 3 moves the entries; the probe's segment of a record that is not scanned is six NaNs."""
    h = au.hand_built()
    assert au.scanned(h).tolist() == [True, True, False, False, False, True] and h["inside"].tolist() == [0, 1, 0, 0, 0, 1]
    n_samples, n_dirs, stride = 16, 64, 7
    e = {au.entry(0, i, stride, s, n_dirs) for i in range(96 * 54) for s in range(n_samples)}
    assert e == set(range(n_dirs)) and any(i * stride + n_samples - 1 >= n_dirs for i in range(96 * 54))
    assert [au.entry(2 ** 40 + 3, i, stride, 0, n_dirs) for i in range(8)] != [au.entry(0, i, stride, 0, n_dirs) for i in range(8)]
    rays, _ = rt_host.ambient_segments(h, 3, n_samples, dirs=rt_host.ambient_dirs(n_dirs), stride=stride, base=2 ** 40 + 3)
    assert np.isnan(rays[2:5]).all() and np.isfinite(rays[[0, 1, 5]]).all()
