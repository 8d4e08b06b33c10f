"""Wavefront tracing of ray lists on the GPU (include/rt_hip.h: rt_scene_shade_rays_device, rt_scene_spawn_rays_device,
rt_scene_fold_nodes_device, rt_trace_rays_wavefront).  Every node of every tree is held to the unchanged C restatement's probe
(oracle/rt_oracle.c oracle_probe_sample) bit for bit - hit, sample, diffuse, children, the spawned rays - and the folded result to the
recursive kernel (rt_host.trace_rays) bit for bit in rgb, which also pins `specular` (OCML's pow, where the probe has the host's)."""
import base64
import copy
import json
import math
import os
import subprocess

import numpy as np
import pytest

import nodes_util as nu
import oracle_util as ou
import rays_util as ru
import rt_host
from objects_util import tlib  # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu
ROOT = ou.ROOT
N_CAMERAS = 48


def _random_scene(seed, n, segs):
    from test_gpu_parity import random_scene
    return random_scene(seed, n, True, segs)


def _four_spheres():
    """Home, skybox and two bubbles (a reflection AND a refraction child per hit) next to each other: deep trees at segs = 16."""
    s = _random_scene(7, 4, 16)
    small = [o for o in s["objects"] if o["r2"] < ru.SMALL_R2]
    assert len(s["objects"]) == 4 and len(small) == 2
    for k, o in enumerate(small):
        o["origin"], o["r2"] = [-0.9 + 1.8 * k, 1.0, 0.0], 1.0
        o["mtl"]["albedo"] = [0.1, 0.5, 0.4, 0.3, 0.6]
        o["mtl"]["refract_index"] = 1.3
    return s


SCENES = {"default14": lambda: rt_host.load_scene("default14"), "h8": lambda: rt_host.load_scene("h8"), "random3": lambda: _random_scene(3, 10, 4)}
_scenes, _oracles = {}, {}


def scene_of(name):
    if name not in _scenes:
        s = SCENES[name]()
        cams = ru.draw_cameras(s, N_CAMERAS, 2000 + len(name), outside_radius=5000.0 if name == "default14" else None)
        _scenes[name] = (s, cams, ru.micro_rays(cams, float(s.get("fovDeg", 60))))
    return _scenes[name]


def oracle_of(name, segs):
    """The restatement's trees of the scene's micro rays at depth segs: computed once, shared, never changed."""
    if (name, segs) not in _oracles:
        s, cams, _ = scene_of(name)
        o = nu.TreeOracle(s, segs)
        trees = o.trees(cams)
        assert o.overflowed == 0
        _oracles[(name, segs)] = (o, trees)
    return _oracles[(name, segs)]


@pytest.fixture(scope="module")
def lib(built):
    lib = rt_host.load_library()
    assert lib.rt_init(1) == 0, lib.rt_last_error()
    return lib


@pytest.fixture(params=["product", "test"])
def anylib(request, lib, tlib):  # noqa: F811
    return lib if request.param == "product" else tlib


# ------------------------------------------------------------------ 5. every node is the restatement's
@pytest.mark.parametrize("segs", [1, 3, 6])
@pytest.mark.parametrize("name", list(SCENES))
def test_every_node_is_the_restatements(anylib, name, segs):
    scene, cams, rays = scene_of(name)
    oracle, trees = oracle_of(name, segs)
    objs = scene["objects"]
    r = rt_host.Renderer(scene, 0, anylib)
    try:
        levels = nu.walk(anylib, r, rays, segs)
    finally:
        r.close()
    assert len(rays) == 4 * N_CAMERAS == len(trees) and len(levels) <= segs
    # the inputs are what they claim to be: origins inside refracting spheres, and (default14) outside the skybox
    roots = np.array([t[1] for t in trees])
    codes = roots[:, 1].astype(int)
    inside = [c >> 1 for c in codes if c >= 0 and c & 1 and objs[c >> 1]["r2"] < ru.SMALL_R2]
    assert any(objs[i]["mtl"]["albedo"][4] > 0 for i in inside) or name == "h8"
    if name == "default14":
        assert (np.linalg.norm(rays[:, 0:3], axis=1) > 5000.0).sum() >= 12
    n_nodes, n_hits, n_children = nu.assert_nodes_are_the_restatements(levels, trees, oracle, objs, segs, name)
    print("NODES %s segs %d: %d nodes in %d levels, %d hits, %d two-child nodes" % (name, segs, n_nodes, len(levels), n_hits, n_children))
    if name != "h8" and segs > 1:
        assert n_children > 0


# ------------------------------------------------------------------ 6. wavefront equals the recursive trace
def _frame_and_micro(scene, name="default14"):
    return np.concatenate([rt_host.primary_rays(64, 36, scene), scene_of(name)[2]])


def _same_as_recursive(scene, rays, segs=0, order_levels=False):
    want = rt_host.trace_rays(scene, rays, segs=segs, want=("rgb", "rgba"))
    got = rt_host.trace_rays(scene, rays, segs=segs, want=("rgb", "rgba", "level_counts"), method="wavefront", order_levels=order_levels)
    counts = got["level_counts"]
    assert got["rgb"].tobytes() == want["rgb"].tobytes(), int((got["rgb"].view(np.uint64) != want["rgb"].view(np.uint64)).sum())
    assert got["rgba"].tobytes() == want["rgba"].tobytes()
    assert counts[0] == len(rays) and counts.dtype == np.uint64 and len(counts) == 16
    empty = np.flatnonzero(counts == 0)
    assert not counts[empty[0]:].any() if len(empty) else True                    # after the first empty level: nothing
    assert not counts[(segs or scene["segs"]):].any()
    return got, counts


def test_wavefront_is_the_recursive_trace_default14(lib):
    scene = rt_host.load_scene("default14")
    assert scene["segs"] == 8
    rays = _frame_and_micro(scene)
    assert len(rays) == 64 * 36 + 192
    got, counts = _same_as_recursive(scene, rays)
    print("NODES wavefront default14: level counts %s" % counts.tolist())
    assert counts[7] > 0 and len({bytes(p) for p in got["rgba"]}) > 100
    ordered, counts2 = _same_as_recursive(scene, rays, order_levels=True)
    assert counts2.tolist() == counts.tolist() and ordered["rgb"].tobytes() == got["rgb"].tobytes()


def test_wavefront_is_the_recursive_trace_h8_d8(lib):
    scene = rt_host.load_scene("h8_d8")
    _, counts = _same_as_recursive(scene, _frame_and_micro(scene, "h8"))
    print("NODES wavefront h8_d8: level counts %s" % counts.tolist())
    assert counts[1] > 0


def test_wavefront_draws_the_stars_of_the_recursive_trace(lib):
    """pix and path travel through the levels: the sky seen directly (level 1), in mirrors and through glass, for two seeds."""
    scene = rt_host.load_scene("default14_stars")
    rays = _frame_and_micro(scene)
    seen = []
    for seed in (0, 7):
        got, _ = _same_as_recursive(dict(scene, starsSeed=seed), rays)
        seen.append(got["rgb"].tobytes())
    assert seen[0] != seen[1]


def test_wavefront_is_the_recursive_trace_at_depth_16(lib):
    scene = _four_spheres()
    rays = rt_host.primary_rays(64, 36, scene)
    got, counts = _same_as_recursive(scene, rays, segs=16)
    print("NODES wavefront four spheres segs 16: level counts %s" % counts.tolist())
    assert counts[15] > 0 and counts[3] > counts[1]                                # the trees do branch
    short, _ = _same_as_recursive(scene, rays, segs=5)
    assert short["rgb"].tobytes() != got["rgb"].tobytes()


def test_wavefront_halves_a_chunk_whose_trees_exceed_the_node_budget(lib):
    """One chunk may hold 2^21 nodes (include/rt_hip.h: rt_trace_rays_wavefront): 90 000 rays of ~30 nodes each do not fit, so the host
    form halves the chunk and starts it again - the same bytes, every ray counted once."""
    scene = _four_spheres()
    rays = rt_host.primary_rays(400, 225, scene)
    _, counts = _same_as_recursive(scene, rays, segs=16)
    print("NODES wavefront four spheres 400x225 segs 16: %d nodes, level counts %s" % (int(counts.sum()), counts.tolist()))
    assert counts[0] == 90000 and counts.sum() > 2 ** 21


# ------------------------------------------------------------------ 7. spawn
@pytest.mark.parametrize("n", [1, 63, 64, 65, 257, 4097, 65536, 65537, 65536 + 257, 2 ** 18])
def test_spawn(lib, n):
    rng = np.random.default_rng(n)
    nodes = np.zeros(n, rt_host.NODE_DTYPE)
    nodes["children"] = rng.integers(0, 4, n)
    if n > 300:
        nodes["children"][256:512] = 0                                               # a workgroup without children, then a full one
        nodes["children"][512:768] = 3
    if n > 65536:                                                                    # above 256 workgroups the scan carries: the same pair astride the carry
        nodes["children"][65536:65792] = 0
        nodes["children"][65792:66048] = 3
    nodes["point"], nodes["reflect_dir"], nodes["refract_dir"] = rng.normal(size=(n, 3)), rng.normal(size=(n, 3)), rng.normal(size=(n, 3))
    pix, path = rng.integers(0, 2 ** 32, n, dtype=np.uint64).astype(np.uint32), rng.integers(1, 2 ** 30, n).astype(np.uint32)
    r = rt_host.Renderer(rt_host.load_scene("h8"), 0, lib)
    try:
        a = nu.spawn(lib, r, nodes, pix, path)
        b = nu.spawn(lib, r, nodes, pix, path)
        bare = nu.spawn(lib, r, nodes)
    finally:
        r.close()
    ch = nodes["children"]
    has = np.stack([(ch & 1) != 0, (ch & 2) != 0], axis=1)
    assert a["count"] == int(has.sum()) == int(np.array([0, 1, 1, 2])[ch].sum())
    print("NODES spawn n %d: %d tiles, %d children" % (n, (n + 255) // 256, a["count"]))
    links = a["links"]
    assert ((links >= 0) == has).all() and (links[~has] == -1).all()
    flat = links.reshape(-1)
    assert (flat[flat >= 0] == np.arange(a["count"])).all()                         # strictly increasing in (parent, reflect-then-refract) order
    for k, field in enumerate(("reflect_dir", "refract_dir")):
        m = has[:, k]
        at = links[m, k]
        assert (a["path"][at] == 2 * path[m] + k).all() and (a["pix"][at] == pix[m]).all()
        assert nu.same_bits(a["rays"][at, 0:3], nodes["point"][m]) and nu.same_bits(a["rays"][at, 3:6], nodes[field][m])
        assert (bare["path"][at] == 2 + k).all() and (bare["pix"][at] == np.flatnonzero(m)).all()
    assert a["raw"] == b["raw"]                                                      # a second run: identical bytes, the unused tails included
    assert bare["raw"][0] == a["raw"][0] and bare["raw"][3] == a["raw"][3]


# ------------------------------------------------------------------ 8. orders and odd rays
def test_orders_give_the_plain_calls_bytes(lib):
    scene, _, rays = scene_of("default14")
    n = len(rays)
    r = rt_host.Renderer(scene, 0, lib)
    try:
        plain = nu.shade(lib, r, rays)
        perm = np.random.default_rng(5).permutation(n).astype(np.uint32)
        assert nu.shade(lib, r, rays, order=perm).tobytes() == plain.tobytes()
        holes = perm.copy()
        skipped = holes[::7].copy()
        holes[::7] = n + np.arange(len(skipped))                                     # entries that name no ray
        got = nu.shade(lib, r, rays, order=holes, fill=0xA5)
        keep = np.ones(n, bool)
        keep[skipped] = False
        assert got[keep].tobytes() == plain[keep].tobytes()
        assert (got[~keep].view(np.uint8) == 0xA5).all() and (~keep).sum() == len(skipped) > 20   # untouched: the sentinel
    finally:
        r.close()
    assert rt_host.shade_rays(scene, rays, order="binned", lib=lib).tobytes() == plain.tobytes()   # the library's own order
    assert rt_host.shade_rays(scene, rays, lib=lib).tobytes() == plain.tobytes()


def test_non_finite_rays_give_the_nan_miss_node(lib):
    scene, _, rays = scene_of("default14")
    rays = rays[:100].copy()
    bad = {}
    j = 2
    for slot in range(6):
        for v in (math.nan, math.inf, -math.inf):
            rays[j, slot] = v
            bad[j] = (slot, v)
            j += 5
    r = rt_host.Renderer(scene, 0, lib)
    try:
        nodes = nu.shade(lib, r, rays)
        clean = nu.shade(lib, r, scene_of("default14")[2][:100])
        rgb, rgba = nu.fold(lib, r, nodes)
    finally:
        r.close()
    keep = np.array([k not in bad for k in range(len(rays))])
    assert nodes[keep].tobytes() == clean[keep].tobytes()
    want = np.zeros(1, rt_host.NODE_DTYPE)
    want["object"], want["t"], want["sample"] = -1, math.inf, math.nan
    for k in bad:
        nd = nodes[k:k + 1]
        assert np.isnan(nd["sample"]).all() and nd["object"][0] == -1 and nd["children"][0] == 0 and nd["t"][0] == math.inf, (k, bad[k])
        rest = nd.copy()
        rest["sample"] = 0
        blank = want.copy()
        blank["sample"] = 0
        assert rest.tobytes() == blank.tobytes(), (k, bad[k])                      # every other double 0
        assert np.isnan(rgb[k]).all() and rgba[k].tolist() == [0, 0, 0, 255]
    assert np.isfinite(rgb[keep]).all()


# ------------------------------------------------------------------ 9. resident edits
def test_resident_edits_reach_the_nodes(tlib):  # noqa: F811
    base = rt_host.load_scene("default14_stars")
    scene = json.loads(json.dumps({k: v for k, v in base.items() if k != "textures"}))
    scene["textures"] = base["textures"]
    for o in scene["objects"]:                                                       # half the sky lit: a few hundred rays show a seed
        if o["mtl"]["sampler"]["kind"] == rt_host.SAMPLER_STARS:
            o["mtl"]["sampler"].update(threshold=0.5, scale=1.0)
    rays = np.concatenate([rt_host.primary_rays(32, 18, scene), scene_of("default14")[2]])

    def fresh(sc):
        f = rt_host.Renderer(sc, 0, tlib)
        try:
            return nu.shade(tlib, f, rays)
        finally:
            f.close()

    r = rt_host.Renderer(scene, 0, tlib)
    try:
        uploads = tlib.rt_test_upload_count()
        first = nu.shade(tlib, r, rays)
        assert first.tobytes() == fresh(scene).tobytes()
        uploads += 1
        r.set_camera(dict(scene["camera"], origin=[1.0, 2.0, 9.0]))                 # a camera move changes nothing
        assert nu.shade(tlib, r, rays).tobytes() == first.tobytes()
        seen = [first.tobytes()]
        i = next(i for i, o in enumerate(scene["objects"]) if o["r2"] < 1e4 and o["mtl"]["albedo"][4] > 0)
        c0 = list(scene["objects"][i]["origin"])
        scene["objects"][i]["origin"] = [c0[0] + 0.5 * math.cos(0.4), c0[1], c0[2] + 0.5 * math.sin(0.4)]
        scene["objects"][i]["mtl"]["albedo"][1] = 0.35
        r.set_objects(scene["objects"][i:i + 1], i)
        scene["lights"] = [[c + 0.75 for c in l] for l in scene["lights"]]
        steps = [("objects", lambda: None), ("lights", lambda: r.set_lights(scene["lights"])),
                 ("intensity", lambda: r.set_light_intensity(31.0)), ("seed", lambda: r.set_stars_seed(7))]
        edited = copy.deepcopy(scene)
        edited["lights"] = base["lights"]
        for what, apply in steps:
            apply()
            if what == "lights":
                edited["lights"] = scene["lights"]
            if what == "intensity":
                edited["light_intensity"] = 31.0
            if what == "seed":
                edited["starsSeed"] = 7
            got = nu.shade(tlib, r, rays)
            assert tlib.rt_test_upload_count() == uploads, what                      # the resident scene took the edit
            want = fresh(edited)
            uploads += 1
            assert got.tobytes() == want.tobytes(), (what, int((got.view(np.uint8).reshape(len(rays), 200) != want.view(np.uint8).reshape(len(rays), 200)).any(axis=1).sum()))
            assert got.tobytes() not in seen, what                                   # ... and the edit shows
            seen.append(got.tobytes())
    finally:
        r.close()


# ------------------------------------------------------------------ 10. Node and Python agree
@pytest.mark.skipif(ou.node_path() is None, reason="node not installed")
def test_node_agrees_with_python(lib):
    name = "default14_stars"
    scene = rt_host.load_scene(name)
    rays = scene_of("default14")[2][:64]
    rng = np.random.default_rng(10)
    pix, path = rng.integers(0, 2 ** 20, 64).astype(np.uint32), rng.integers(1, 2 ** 8, 64).astype(np.uint32)
    pkg = os.path.join(ROOT, "html5-canvas-raytracer_amd")
    b64 = lambda a: base64.b64encode(np.ascontiguousarray(a).tobytes()).decode()
    out = subprocess.check_output([ou.node_path(), os.path.join(ROOT, "tests", "js_nodes_check.js"), pkg, name, b64(rays), b64(pix), b64(path)],
                                  text=True, timeout=300)
    res = json.loads(out.strip().splitlines()[-1])
    want = rt_host.shade_rays(scene, rays, lib=lib)
    assert res["count"] == 64 and base64.b64decode(res["nodes"]) == want.tobytes() and res["binned"] is True
    assert base64.b64decode(res["tagged"]) == rt_host.shade_rays(scene, rays, pix=pix, path=path, lib=lib).tobytes()
    for nd, w in zip(res["accessor"], want):
        if w["object"] < 0:
            assert nd["hit"] is None
        else:
            h = nd["hit"]
            assert (h["index"], h["inside"], h["t"], h["point"], h["normal"], h["u"], h["v"]) == \
                (int(w["object"]), bool(w["inside"]), float(w["t"]), w["point"].tolist(), w["normal"].tolist(), float(w["u"]), float(w["v"]))
        assert nd["sample"] == w["sample"].tolist() and nd["diffuse"] == w["diffuse"] and nd["specular"] == w["specular"]
        assert (nd["ambient"], nd["reflectWeight"], nd["refractWeight"]) == (w["ambient"], w["reflect_weight"], w["refract_weight"])
        assert nd["reflectDir"] == w["reflect_dir"].tolist() and nd["refractDir"] == w["refract_dir"].tolist() and nd["children"] == int(w["children"])
    py = rt_host.trace_rays(scene, rays, want=("rgb", "level_counts"), method="wavefront", lib=lib)
    assert res["sameRgb"] is True and res["sameRgba"] is True and base64.b64decode(res["rgb"]) == py["rgb"].tobytes()
    assert res["levelCounts"] == py["level_counts"].tolist()
    assert res["bad"] == [True, True, True, True]
