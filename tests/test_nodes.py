"""CPU tests of the wavefront surface (include/rt_hip.h: rt_node, rt_scene_shade_rays_device, rt_nodes_spawn_work_bytes,
rt_scene_spawn_rays_device, rt_scene_fold_nodes_device, rt_trace_rays_wavefront; rt_host.NODE_DTYPE, fold_nodes_host): the record's
layout against the header, exports and binding, argument checks before a device is touched, and - with the oracle alone - the fold
rule: node arrays built from the C restatement's own probe records, folded bottom-up by rt_host.fold_nodes_host, give the bytes of
the restatement's render, equal and not within 1 LSB."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import nodes_util as nu
import oracle_util as ou
import rays_util as ru
import rt_host

ROOT = ou.ROOT
RT_ERR_INVALID, RT_ERR_STATE = -1, -5
SYMBOLS = ("rt_scene_shade_rays_device", "rt_shade_rays", "rt_nodes_spawn_work_bytes", "rt_scene_spawn_rays_device", "rt_scene_fold_nodes_device",
           "rt_trace_rays_wavefront")
# include/rt_hip.h rt_node, by hand: what the kernels' 16-byte stores and the hosts' readers go by
LAYOUT = {"object": 0, "inside": 4, "t": 8, "point": 16, "normal": 40, "u": 64, "v": 72, "sample": 80, "diffuse": 104, "specular": 112,
          "ambient": 120, "reflect_weight": 128, "refract_weight": 136, "reflect_dir": 144, "refract_dir": 168, "children": 192, "reserved": 196}
C_FIELD = {"object": "hit.object", "inside": "hit.inside", "t": "hit.t", "point": "hit.point", "normal": "hit.normal", "u": "hit.u", "v": "hit.v"}


def test_both_libraries_export_the_symbols(built):
    for path in (rt_host.LIB_PATH, rt_host.TEST_LIB_PATH):
        lib = C.CDLL(path)
        for name in SYMBOLS:
            assert hasattr(lib, name), (path, name)


def test_node_layout_is_the_headers(built, tmp_path):
    cc = shutil.which("gcc") or shutil.which("cc")
    assert cc, "a C compiler is needed (the oracle is built with one)"
    names = list(LAYOUT)
    src = tmp_path / "layout.c"
    text = '#include <stddef.h>\n#include <stdio.h>\n#include "rt_hip.h"\nint main(void) {\n  printf("%zu %u\\n", sizeof(rt_node), RT_ABI_VERSION);\n'
    text += "".join('  printf("%%zu\\n", offsetof(rt_node, %s));\n' % C_FIELD.get(f, f) for f in names) + "  return 0;\n}\n"
    src.write_text(text)
    exe = tmp_path / "layout"
    subprocess.run([cc, "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)], check=True)
    got = [int(x) for x in subprocess.check_output([str(exe)], text=True).split()]
    d = rt_host.NODE_DTYPE
    assert got[0] == d.itemsize == 200 and got[0] % 8 == 0
    assert got[1] == 2 == rt_host.RT_ABI_VERSION          # an addition: the ABI version stays
    assert list(d.names) == names
    assert got[2:] == [d.fields[f][1] for f in names] == [LAYOUT[f] for f in names]
    assert d.fields["point"][0].shape == (3,) and d.fields["children"][0].base == np.dtype("<u4") and d.fields["object"][0] == np.dtype("<i4")
    # the prototypes: a C compiler takes the header and the assignments
    proto = tmp_path / "proto.c"
    proto.write_text('#include "rt_hip.h"\n'
                     'int (*a)(rt_scene_dev *, uint64_t, const double *, const uint32_t *, const uint32_t *, const uint32_t *, rt_node *, void *, rt_stats *) = rt_scene_shade_rays_device;\n'
                     'int (*a2)(const void *, size_t, uint64_t, const double *, const uint32_t *, const uint32_t *, int, rt_node *, rt_stats *) = rt_shade_rays;\n'
                     'size_t (*b)(uint64_t) = rt_nodes_spawn_work_bytes;\n'
                     'int (*c)(rt_scene_dev *, uint64_t, const rt_node *, const uint32_t *, const uint32_t *, double *, uint32_t *, uint32_t *, int32_t *, uint32_t *, void *, size_t, void *) = rt_scene_spawn_rays_device;\n'
                     'int (*d)(rt_scene_dev *, uint64_t, const rt_node *, const int32_t *, const double *, double *, uint8_t *, void *) = rt_scene_fold_nodes_device;\n'
                     'int (*e)(const void *, size_t, uint64_t, const double *, uint32_t, int, const rt_ray_outputs *, rt_stats *, uint64_t *) = rt_trace_rays_wavefront;\n')
    subprocess.run([cc, "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", "-o", str(tmp_path / "proto.o"), str(proto)], check=True)
    lib = rt_host.load_library()
    for name in SYMBOLS:
        assert getattr(lib, name).argtypes == rt_host.ABI[name][1]


def test_spawn_work_bytes(built):
    f = rt_host.nodes_spawn_work_bytes
    assert f(0) == 0 and f(2 ** 31) == 0 and f(2 ** 40) == 0
    sizes = [1, 2, 63, 64, 65, 255, 256, 257, 4096, 4097, 10 ** 6, 2 ** 31 - 1]
    got = [f(n) for n in sizes]
    assert got[0] > 0 and all(a <= b for a, b in zip(got, got[1:]))
    assert all(g >= 4 * ((n + 255) // 256) for g, n in zip(got, sizes))


def _aligned(nbytes, offset_bytes=0):
    """A zeroed uint8 array on a 16-byte boundary (+ offset_bytes)."""
    raw = np.zeros(nbytes + 32, np.uint8)
    start = (-raw.ctypes.data) % 16 + offset_bytes
    a = raw[start:start + nbytes]
    assert a.ctypes.data % 16 == offset_bytes
    return a


def test_bad_arguments_are_refused_before_a_device_is_touched(built):
    lib = rt_host.load_library()
    err = lambda: lib.rt_last_error().decode()
    rays, nodes, crays = _aligned(96), _aligned(400), _aligned(192)
    u32 = [_aligned(16) for _ in range(6)]                 # order, pix, path, child pix, child path, links
    count, work, rgb, crgb, rgba = _aligned(16), _aligned(16), _aligned(48), _aligned(96), _aligned(8)
    nodes[:] = 7
    P = lambda a, off=0: C.c_void_p(a.ctypes.data + off) if a is not None else None

    def shade(n=2, r=P(rays), o=P(u32[0]), px=P(u32[1]), pa=P(u32[2]), nd=P(nodes)):
        return lib.rt_scene_shade_rays_device(None, n, r, o, px, pa, nd, None, None)

    def spawn(n=2, nd=P(nodes), px=P(u32[1]), pa=P(u32[2]), cr=P(crays), cpx=P(u32[3]), cpa=P(u32[4]), lk=P(u32[5]), cnt=P(count), wk=P(work), wb=16):
        return lib.rt_scene_spawn_rays_device(None, n, nd, px, pa, cr, cpx, cpa, lk, cnt, wk, wb, None)

    def fold(n=2, nd=P(nodes), lk=P(u32[5]), cr=P(crgb), o=P(rgb), oa=P(rgba)):
        return lib.rt_scene_fold_nodes_device(None, n, nd, lk, cr, o, oa, None)

    for call in (shade, spawn, fold):
        assert call(n=0) == RT_ERR_INVALID and "n 0" in err()
        assert call(n=2 ** 31) == RT_ERR_INVALID and "n 2147483648" in err()
        assert call(nd=None) == RT_ERR_INVALID and "NULL" in err()
        assert call(nd=P(nodes, 4)) == RT_ERR_INVALID and "misaligned" in err()
    assert shade(r=None) == RT_ERR_INVALID and "NULL" in err()
    assert shade(r=P(rays, 8)) == RT_ERR_INVALID and "16-byte aligned" in err()
    for k in ("o", "px", "pa"):
        assert shade(**{k: P(u32[0], 2)}) == RT_ERR_INVALID and "misaligned" in err()
    for k in ("cr", "lk", "cnt", "wk"):
        assert spawn(**{k: None}) == RT_ERR_INVALID and "NULL" in err()
    assert spawn(cr=P(crays, 8)) == RT_ERR_INVALID and "16-byte aligned" in err()
    for k in ("px", "pa", "cpx", "cpa", "lk", "cnt", "wk"):
        assert spawn(**{k: P(u32[0], 2)}) == RT_ERR_INVALID and "misaligned" in err()
    assert spawn(n=257, wb=4) == RT_ERR_INVALID and "work_bytes" in err()
    assert fold(o=None, oa=None) == RT_ERR_INVALID and "every output is NULL" in err()
    assert fold(cr=None) == RT_ERR_INVALID and "links without" in err()
    for k, a, off in (("lk", u32[5], 2), ("cr", crgb, 4), ("o", rgb, 4), ("oa", rgba, 2)):
        assert fold(**{k: P(a, off)}) == RT_ERR_INVALID and "misaligned" in err()
    # with every argument in order: a NULL scene handle is a state error (the optional pointers NULL are in order)
    for call, kws in ((shade, ({}, {"o": None, "px": None, "pa": None})), (spawn, ({}, {"px": None, "pa": None, "cpx": None, "cpa": None})),
                      (fold, ({}, {"lk": None, "cr": None}, {"o": None}, {"oa": None}))):
        for kw in kws:
            assert call(**kw) == RT_ERR_STATE and "NULL scene" in err()
    assert (nodes == 7).all() and not rgb.any() and not count.any()
    # the host form: the ray-list checks of rt_trace_rays, and no hit records
    blob = rt_host.flatten_scene(rt_host.load_scene("h8"))
    buf = C.create_string_buffer(blob, len(blob))
    out = rt_host.RtRayOutputs(rgb.ctypes.data, None, None)

    def host(n=2, r=P(rays), segs=0, o=out, nb=len(blob)):
        return lib.rt_trace_rays_wavefront(buf, nb, n, r, segs, 0, C.byref(o), None, None)

    assert host(n=0) == RT_ERR_INVALID and host(n=2 ** 31) == RT_ERR_INVALID and host(r=None) == RT_ERR_INVALID
    assert host(r=P(rays, 8)) == RT_ERR_INVALID and host(segs=17) == RT_ERR_INVALID and host(nb=len(blob) - 8) == RT_ERR_INVALID
    assert host(o=rt_host.RtRayOutputs(None, None, None)) == RT_ERR_INVALID
    assert host(o=rt_host.RtRayOutputs(rgb.ctypes.data, None, nodes.ctypes.data)) == RT_ERR_INVALID and "hit records" in err()
    for bad in (dict(method="levels"), dict(method="wavefront", order="binned"), dict(method="wavefront", want=("hits",)),
                dict(method="wavefront", want=("level_counts",)), dict(want=("rgb", "level_counts"))):
        with pytest.raises(ValueError):
            rt_host.trace_rays(rt_host.load_scene("h8"), np.zeros((2, 6)), **bad)


def test_fold_host_nan_and_order_rules():
    """Math.min / Math.max with JavaScript's NaN rule, the four terms left to right, a miss keeps its sample."""
    nd = np.zeros(4, rt_host.NODE_DTYPE)
    nd["sample"] = [[0.5, 1.0, 0.25], [1.0, 0.0, 0.0], [np.nan, 1.0, 1.0], [1e308, 1.0, 0.1]]
    nd["object"] = [0, -1, 2, 3]
    nd["diffuse"], nd["specular"], nd["ambient"] = [0.5, 9.0, 0.5, 1.0], [0.25, 9.0, 0.0, 1.0], [0.1, 9.0, 0.2, 0.0]
    nd["reflect_weight"], nd["refract_weight"] = [0.5, 1.0, 0.5, 0.0], [0.25, 1.0, 0.0, 0.0]
    links = np.array([[1, 0], [-1, -1], [-1, -1], [-1, -1]], np.int32)
    child = np.array([[0.2, 0.4, 8.0], [0.1, 0.2, 0.3]])
    got = rt_host.fold_nodes_host(nd, links, child)
    s = nd["sample"][0]
    want0 = [max(s[c] * 0.1, min(1.0, s[c] * 0.5 + s[c] * 0.25 + child[1][c] * 0.5 + child[0][c] * 0.25)) for c in range(3)]
    assert got[0].tolist() == want0 and got[0][2] == 1.0
    assert got[1].tolist() == [1.0, 0.0, 0.0]                               # a miss: the sample, whatever the other fields hold
    assert np.isnan(got[2][0]) and got[2][1:].tolist() == [0.5, 0.5]          # NaN in, NaN out; the other channels are untouched
    assert got[3].tolist() == [1.0, 1.0, 0.2]                               # an overflowing sum is +Infinity, and min(1, .) of it 1
    leaf = rt_host.fold_nodes_host(nd, None, None)
    assert leaf[0].tolist() == [max(s[c] * 0.1, min(1.0, s[c] * 0.5 + s[c] * 0.25)) for c in range(3)]


def _cfg2_textured():
    import texture_util as tu
    return tu.textured(tu.with_textures(rt_host.load_scene("cfg2")), {0: 2, 1: 12, 3: 9})


FOLD_CASES = {"default14": (lambda: rt_host.load_scene("default14"), 6), "h8": (lambda: rt_host.load_scene("h8"), 3),
              "cfg2_textured": (_cfg2_textured, 4), "default14_d2": (lambda: rt_host.load_scene("default14"), 2)}


@pytest.mark.parametrize("case", sorted(FOLD_CASES))
def test_fold_rule_against_the_restatement(built, case):
    """Nodes from the restatement's probe, rt_host.fold_nodes_host bottom-up, the store rule: c_oracle_render's bytes, all of them."""
    make, segs = FOLD_CASES[case]
    scene = make()
    assert segs <= 6                                                     # 2^6 - 1 nodes at most: no probe can overflow its 64 records
    cams = ru.draw_cameras(scene, 48, 4000 + len(case), outside_radius=5000.0 if case.startswith("default14") else None)
    oracle = nu.TreeOracle(scene, segs)
    trees = oracle.trees(cams)
    assert len(trees) == 192 and oracle.overflowed == 0
    levels = oracle.levels(trees)
    sizes = [len(lv["nodes"]) for lv in levels]
    assert sizes[0] == 192 and sum(sizes) == sum(len(t) for t in trees) and len(levels) <= segs
    rgb = nu.fold_levels(levels)
    want = oracle.rgba(cams)
    got = ru.store_rule(rgb)
    both = sum(1 for lv in levels for l in lv["links"] if l[0] >= 0 and l[1] >= 0)
    print("NODES fold %s: %d rays, levels %s, %d two-child nodes, %d of %d bytes differ" % (case, len(trees), sizes, both, int((got != want).sum()), got.size))
    assert got.shape == want.shape == (192, 4) and np.array_equal(got, want)
    assert len({bytes(p) for p in want}) > 20                             # not all sky
    if case == "default14":
        assert len(levels) == 6 and both > 0                             # deep trees, and nodes with a reflection AND a refraction child
