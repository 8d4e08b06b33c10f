"""Probes on a CPU (include/rt_hip.h: rt_probe_outputs): the exported symbols, header and binding, every refusal - none of which touches
a device -, the spherical-harmonics weights against the numpy restatement of the header's operation order, and what rt_host.gather
refuses of `mapping` and `weights`.  No GPU."""
import ctypes as C
import math
import shutil
import subprocess

import numpy as np
import pytest

import ambient_util as au
import rt_host
from test_ambient import INCLUDE, RT_ERR_INVALID, RT_ERR_STATE

SYMBOLS = ("rt_probes_validate", "rt_scene_gather_probes_device", "rt_gather_probes", "rt_probe_sh9_weights")


def test_both_libraries_export_the_symbols(built):
    for path in (rt_host.LIB_PATH, rt_host.TEST_LIB_PATH):
        lib = C.CDLL(path)
        for name in SYMBOLS:
            assert hasattr(lib, name), (path, name)


def test_header_and_binding_agree(built, tmp_path):
    cc = shutil.which("gcc") or shutil.which("cc")
    assert cc, "a C compiler is needed (the oracle is built with one)"
    proto = tmp_path / "proto.c"
    proto.write_text('#include "rt_hip.h"\n'
                     'int (*val)(const struct rt_gather *, const double *, const double *, uint32_t) = rt_probes_validate;\n'
                     'int (*sh)(uint32_t, const double *, double *) = rt_probe_sh9_weights;\n'
                     'int (*host)(const void *, size_t, const struct rt_gather *, const double *, const double *, uint32_t, uint64_t, const rt_hit *, '
                     'const rt_probe_outputs *, rt_stats *) = rt_gather_probes;\n'
                     'int (*dev)(rt_scene_dev *, const struct rt_gather *, const double *, const double *, uint32_t, uint64_t, const rt_hit *, const uint32_t *, '
                     'const rt_probe_outputs *, void *, rt_stats *) = rt_scene_gather_probes_device;\n')
    subprocess.run([cc, "-Wall", "-Werror", "-I", INCLUDE, "-c", "-o", str(tmp_path / "proto.o"), str(proto)], check=True)
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "rt_hip.h"\n'
                   'int main(void) { printf("%zu %zu %zu %zu %u %u\\n", sizeof(rt_probe_outputs), offsetof(rt_probe_outputs, rgb), offsetof(rt_probe_outputs, rgba), '
                   'offsetof(rt_probe_outputs, coef), RT_PROBE_MAX_WEIGHTS, RT_ABI_VERSION); return 0; }\n')
    exe = tmp_path / "layout"
    subprocess.run([cc, "-Wall", "-Werror", "-I", INCLUDE, "-o", str(exe), str(src)], check=True)
    got = [int(x) for x in subprocess.check_output([str(exe)], text=True).split()]
    o = [C.sizeof(rt_host.RtProbeOutputs)] + [getattr(rt_host.RtProbeOutputs, f).offset for f, _ in rt_host.RtProbeOutputs._fields_]
    assert got[:4] == o == [24, 0, 8, 16]
    assert got[4] == 16 == rt_host.RT_PROBE_MAX_WEIGHTS
    assert got[5] == 2 == rt_host.RT_ABI_VERSION           # an addition: the ABI version stays
    lib = rt_host.load_library()
    for name in SYMBOLS:
        assert getattr(lib, name).argtypes == rt_host.ABI[name][1] and getattr(lib, name).restype == rt_host.ABI[name][0]


def test_bad_arguments_are_refused_before_a_device_is_touched(built):
    lib = rt_host.load_library()
    err = lambda: lib.rt_last_error().decode()
    A, O = rt_host.RtGather, rt_host.RtProbeOutputs
    blob = rt_host.flatten_scene(rt_host.load_scene("h8"))
    buf = C.create_string_buffer(blob, len(blob))
    dirs = rt_host.ambient_dirs(8)
    weights = rt_host.sh9_weights(dirs, lib=lib)
    hits = au.hand_built()
    n = len(hits)
    rgb, rgba, coef, order = np.full(3 * n + 1, 7.0), np.full(n + 1, 7, np.uint32), np.full(27 * n + 1, 7.0), np.zeros(n + 1, np.uint32)
    good_out = O(rgb.ctypes.data, rgba.ctypes.data, coef.ctypes.data)
    plain_out = O(rgb.ctypes.data, rgba.ctypes.data, None)
    good = dict(n_samples=4, n_dirs=8, stride=1, segs=0, base=0, pix_base=0, pix_stride=n)

    def desc(**kw):
        f = dict(good, **kw)
        return A(f["n_samples"], f["n_dirs"], f["stride"], f["segs"], f["base"], f["pix_base"], f["pix_stride"])

    P = C.c_void_p
    calls = {
        "validate": lambda a, d=dirs.ctypes.data, w=weights.ctypes.data, nw=9: lib.rt_probes_validate(C.byref(a), P(d), P(w), nw),
        "host": lambda a, d=dirs.ctypes.data, w=weights.ctypes.data, nw=9: lib.rt_gather_probes(buf, len(blob), C.byref(a), P(d), P(w), nw, n, P(hits.ctypes.data),
                                                                                                C.byref(good_out), None),
        "device": lambda a, d=dirs.ctypes.data, w=weights.ctypes.data, nw=9: lib.rt_scene_gather_probes_device(None, C.byref(a), P(d), P(w), nw, n, P(hits.ctypes.data),
                                                                                                             None, C.byref(good_out), None, None),
    }
    for name, call in calls.items():
        # what rt_gather_validate refuses of the description
        for kw, text in (({"n_samples": 0}, "n_samples 0"), ({"n_samples": 1025, "n_dirs": 2000}, "n_samples 1025"), ({"n_dirs": 3}, "n_dirs 3"),
                         ({"n_dirs": 65537}, "n_dirs 65537"), ({"segs": 17}, "segs 17")):
            assert call(desc(**kw)) == RT_ERR_INVALID and text in err(), (name, kw, err())
        assert call(desc(), 0) == RT_ERR_INVALID and "NULL" in err(), name
        # the weights: their count, and a count without a table or a table without a count
        assert call(desc(), nw=17) == RT_ERR_INVALID and "n_weights 17" in err(), name
        assert call(desc(), w=0) == RT_ERR_INVALID and "without a weight table" in err(), name
        assert call(desc(), nw=0) == RT_ERR_INVALID and "with a weight table" in err(), name
        assert call(desc(), w=weights.ctypes.data + 4) == RT_ERR_INVALID and "misaligned weights" in err(), name
    # a table entry or a weight that is not finite: the entry points that see the tables in host memory
    for bad in (math.nan, math.inf, -math.inf):
        for name in ("validate", "host"):
            broken = dirs.copy()
            broken.reshape(-1)[23] = bad
            assert calls[name](desc(), broken.ctypes.data) == RT_ERR_INVALID and "non-finite" in err(), (name, bad)
            for at in (0, 71):
                heavy = weights.copy()
                heavy.reshape(-1)[at] = bad
                assert calls[name](desc(), w=heavy.ctypes.data) == RT_ERR_INVALID and "not finite" in err(), (name, bad, at)
        # ... but not a weight of an entry past n_dirs
        heavy = weights.copy()
        heavy[7, 0] = bad
        assert lib.rt_probes_validate(C.byref(desc(n_dirs=7)), P(dirs.ctypes.data), P(heavy.ctypes.data), 9) == 0
    for nw in (1, 9, 16):
        assert lib.rt_probes_validate(C.byref(desc()), P(dirs.ctypes.data), P(np.ones((8, nw)).ctypes.data), nw) == 0
    assert lib.rt_probes_validate(C.byref(desc()), P(dirs.ctypes.data), None, 0) == 0              # the plain mean
    assert lib.rt_probes_validate(None, P(dirs.ctypes.data), None, 0) == RT_ERR_INVALID

    # the device form's: count, bound on pix, pointers, alignment, outputs, order; then the scene
    def dev(a=None, o=good_out, m=n, h=hits.ctypes.data, d=dirs.ctypes.data, w=weights.ctypes.data, nw=9, order=0):
        return lib.rt_scene_gather_probes_device(None, C.byref(a or desc()), P(d), P(w), nw, m, P(h), P(order), C.byref(o) if o is not None else None, None, None)

    assert dev(m=0) == RT_ERR_INVALID and "n 0" in err()
    assert dev(m=2 ** 31, a=desc(pix_stride=0)) == RT_ERR_INVALID and "n 2147483648" in err()
    assert dev(a=desc(pix_base=2 ** 31 - 5, pix_stride=0)) == RT_ERR_INVALID and "above 2^31" in err()
    assert dev(a=desc(pix_base=2 ** 31 - 6, pix_stride=0)) == RT_ERR_STATE and "NULL scene" in err()
    assert dev(o=None) == RT_ERR_INVALID and "NULL outputs" in err()
    assert dev(o=O(None, None, None), w=0, nw=0) == RT_ERR_INVALID and "every output is NULL" in err()
    assert dev(o=plain_out) == RT_ERR_INVALID and "together or not at all" in err()                   # weights without coef
    assert dev(o=good_out, w=0, nw=0) == RT_ERR_INVALID and "together or not at all" in err()         # coef without weights
    assert dev(o=O(rgb.ctypes.data + 4, None, coef.ctypes.data)) == RT_ERR_INVALID and "misaligned output" in err()
    assert dev(o=O(None, rgba.ctypes.data + 2, coef.ctypes.data)) == RT_ERR_INVALID and "misaligned output" in err()
    assert dev(o=O(None, None, coef.ctypes.data + 4)) == RT_ERR_INVALID and "misaligned output" in err()
    assert dev(h=0) == RT_ERR_INVALID and dev(h=hits.ctypes.data + 4) == RT_ERR_INVALID and "misaligned" in err()
    assert dev(d=0) == RT_ERR_INVALID and dev(d=dirs.ctypes.data + 4) == RT_ERR_INVALID and "misaligned" in err()
    assert dev(order=order.ctypes.data + 2) == RT_ERR_INVALID and "misaligned order" in err()
    for o, w, nw in ((good_out, weights.ctypes.data, 9), (O(None, None, coef.ctypes.data), weights.ctypes.data, 9), (plain_out, 0, 0),
                     (O(rgb.ctypes.data, None, None), 0, 0), (O(None, rgba.ctypes.data, None), 0, 0)):
        assert dev(o=o, w=w, nw=nw) == RT_ERR_STATE and "NULL scene" in err()
    # the host form's outputs
    host = lambda o, w=weights.ctypes.data, nw=9: lib.rt_gather_probes(buf, len(blob), C.byref(desc()), P(dirs.ctypes.data), P(w), nw, n, P(hits.ctypes.data),
                                                                       C.byref(o), None)
    assert host(O(None, None, None), 0, 0) == RT_ERR_INVALID and "every output is NULL" in err()
    assert host(plain_out) == RT_ERR_INVALID and host(good_out, 0, 0) == RT_ERR_INVALID and "together or not at all" in err()
    assert host(O(None, None, coef.ctypes.data + 4)) == RT_ERR_INVALID and "misaligned output" in err()
    # nothing was written
    assert (rgb == 7.0).all() and (rgba == 7).all() and (coef == 7.0).all()


def sh9_numpy(d):
    """include/rt_hip.h's operation order for rt_probe_sh9_weights, one numpy operation per operation"""
    x, y, z = d[:, 0], d[:, 1], d[:, 2]
    out = np.empty((len(d), 9))
    out[:, 0] = 0.28209479177387814
    out[:, 1] = 0.4886025119029199 * y
    out[:, 2] = 0.4886025119029199 * z
    out[:, 3] = 0.4886025119029199 * x
    out[:, 4] = 1.0925484305920792 * (x * y)
    out[:, 5] = 1.0925484305920792 * (y * z)
    out[:, 6] = 1.0925484305920792 * (x * z)
    out[:, 7] = 0.31539156525252005 * ((3.0 * (z * z)) - 1.0)
    out[:, 8] = 0.5462742152960396 * ((x * x) - (y * y))
    return out


def test_sh9_weights_are_the_headers_operations(built):
    lib = rt_host.load_library()
    dirs = rt_host.lighting_offsets(64, lib=lib)
    got = rt_host.sh9_weights(dirs, lib=lib)
    assert got.shape == (64, 9) and got.tobytes() == sh9_numpy(dirs).tobytes()
    # directions are taken as given: twice as long, other values
    assert rt_host.sh9_weights(2.0 * dirs, lib=lib).tobytes() == sh9_numpy(2.0 * dirs).tobytes() != got.tobytes()
    assert lib.rt_probe_sh9_weights(0, C.c_void_p(dirs.ctypes.data), C.c_void_p(got.ctypes.data)) == RT_ERR_INVALID
    assert lib.rt_probe_sh9_weights(4, None, C.c_void_p(got.ctypes.data)) == RT_ERR_INVALID


def test_the_host_form_refuses_a_mapping_it_does_not_know(built):
    scene = rt_host.load_scene("h8")
    hits = au.hand_built()
    with pytest.raises(ValueError, match="mapping"):
        rt_host.gather(scene, hits, 4, mapping="bogus")
    with pytest.raises(ValueError, match="weights need"):
        rt_host.gather(scene, hits, 4, mapping="receivers", weights=np.ones((4, 1)))
    with pytest.raises(ValueError, match="weights need"):
        rt_host.gather(scene, hits, 4, weights=np.ones((4, 1)))
    with pytest.raises(ValueError, match="needs weights"):
        rt_host.gather(scene, hits, 4, mapping="samples", want=("coef",))
    with pytest.raises(ValueError, match="one row per table entry"):
        rt_host.gather(scene, hits, 4, mapping="samples", weights=np.ones((5, 1)), want=("coef",))
