"""The wavefront form (csrc/rt_nodes.hip: shade, spawn, fold; csrc/rt_frame.hip: rt_trace_rays_wavefront) at the edges the older copies of
its code are held to (tests/test_gpu_parity.py) and at the edges of its own host loop.  Two references, no tolerance of this file's own:
R1  rt_host.trace_rays(..., method="recursive") on the same list: rgb and rgba byte for byte;
R2  the unchanged C restatement (oracle/rt_oracle.c): its probe records bit for bit (nodes_util.assert_nodes_are_the_restatements), its
    frame under the project's rule of at most 1 LSB per channel - and byte for byte for the soak's exact-coincidence seeds, where
    test_soak_seeds_on_exact_coincidences demands that of the strict kernel.
A condition that says an input reaches the edge it is there for is asserted on the reference's side alone."""
import copy
import math
import time

import numpy as np
import pytest

import hits_util as hu
import nodes_util as nu
import oracle_util as ou
import rays_util as ru
import rt_host
import texture_util as tu

pytestmark = pytest.mark.gpu
N_CAMERAS = 48
SOAK = [(1153727, False), (1189883, False), (1021, True), (1183, True), (1616, True), (2532, True), (3581, True), (3979, True)]   # test_soak_seeds_on_exact_coincidences'
TOINT32 = [(3.0e9, 7.0e9), (1e308, -1e308), (-5000.0, 2500.0)]                                                                   # test_checker_toint32_beyond_32_bits'


@pytest.fixture(scope="module")
def lib(built):
    lib = rt_host.load_library()
    assert lib.rt_init(1) == 0, lib.rt_last_error()
    return lib


# ------------------------------------------------------------------ the scenes
def _max_scene(lights=16):
    from test_gpu_parity import random_scene
    s = random_scene(11, 256, True, 3)
    s["lights"] = [[math.cos(k) * 6, 9.0, math.sin(k) * 6] for k in range(lights)]      # test_max_objects_and_lights'
    return s


def _h8(**changes):
    s = rt_host.load_scene("h8")
    s.update(changes)
    return s


def _toint32_scene(k):
    s = rt_host.load_scene("h8")
    home = next(o for o in s["objects"] if o["mtl"]["sampler"]["kind"] == 2)
    home["mtl"]["sampler"]["freqU"], home["mtl"]["sampler"]["freqV"] = TOINT32[k]
    return s


def _soak(k):
    import soak_gpu_parity as soak
    return soak.draw_scene(SOAK[k][0], SOAK[k][1], False)


ROWS = list(range(120, 170, 3))                                                          # test_camera_inside_a_sphere_and_transparent_occluders'
# name -> () -> (scene, w, h, rows of the frame or None = all)
CASES = {"max256x16": lambda: (_max_scene(), 48, 32, None), "no_lights": lambda: (_h8(lights=[]), 64, 40, None)}
CASES.update({name: (lambda name=name: tu.oracle_scene(name) + (None,)) for name, _, _, _ in tu.ORACLE_SCENES})
CASES.update({"toint32_%d" % k: (lambda k=k: (_toint32_scene(k), 160, 90, None)) for k in range(len(TOINT32))})
CASES.update({"soak_%d" % SOAK[k][0]: (lambda k=k: _soak(k) + (None,)) for k in range(len(SOAK))})
CASES.update({"cfg1": lambda: (rt_host.load_scene("cfg1"), 64, 64, None), "default14_rows": lambda: (rt_host.load_scene("default14"), 320, 180, ROWS)})
_cases, _oracles = {}, {}


def case(name):
    """The scene, its primary rays (every sample of the frame, or of `rows`) followed by 192 micro rays: built once, shared, never changed."""
    if name not in _cases:
        scene, w, h, rows = CASES[name]()
        k = scene.get("supersample", 1)
        primary = rt_host.primary_rays(w, h, scene)
        if rows is not None:
            assert k == 1
            primary = primary.reshape(h, w, 6)[rows].reshape(-1, 6)
        cams = ru.draw_cameras(scene, N_CAMERAS, 3000 + sorted(CASES).index(name))
        micro = ru.micro_rays(cams, float(scene.get("fovDeg", 60)))
        _cases[name] = {"scene": scene, "w": w, "h": h, "rows": rows, "ss": k, "cams": cams, "micro": micro, "n_primary": len(primary),
                        "rays": np.concatenate([primary, micro]), "node_segs": min(max(scene["segs"], 3), 6)}
    return _cases[name]


def oracle_of(name, scene=None, tag=""):
    """The restatement's trees of the case's micro rays at its node depth (scene: a variant of the case's scene, under `tag`)."""
    if (name, tag) not in _oracles:
        c = case(name)
        o = nu.TreeOracle(scene or c["scene"], c["node_segs"])
        trees = o.trees(c["cams"])
        assert o.overflowed == 0
        _oracles[(name, tag)] = (o, trees)
    return _oracles[(name, tag)]


def _records(trees):
    return np.array([q for t in trees for q in t.values()])


# ------------------------------------------------------------------ A (i) wavefront == R1 (and R2's frame)
def _wavefront(scene, rays, segs=0, want=("rgb", "rgba"), order_levels=False):
    got = rt_host.trace_rays(scene, rays, segs=segs, want=tuple(want) + ("level_counts",), method="wavefront", order_levels=order_levels)
    assert set(got) == set(want) | {"level_counts"}
    counts = got["level_counts"]
    assert counts.dtype == np.uint64 and len(counts) == 16
    empty = np.flatnonzero(counts == 0)
    assert not counts[empty[0]:].any() if len(empty) else True                          # after the first empty level: nothing
    return got


def _same(got, ref, what):
    for k in ref:
        assert got[k].dtype == ref[k].dtype and got[k].shape == ref[k].shape
        assert got[k].tobytes() == ref[k].tobytes(), (what, k, int((got[k].reshape(len(ref[k]), -1).view(np.uint8) != ref[k].reshape(len(ref[k]), -1).view(np.uint8)).any(axis=1).sum()))


@pytest.mark.parametrize("name", list(CASES))
def test_edge_scene_wavefront_is_the_recursive_trace(lib, name):
    c = case(name)
    scene, rays = c["scene"], c["rays"]
    t0 = time.perf_counter()
    ref = rt_host.trace_rays(scene, rays, want=("rgb", "rgba"))
    got = _wavefront(scene, rays)
    _same(got, ref, name)
    counts = got["level_counts"]
    assert counts[0] == (len(rays) if scene["segs"] else 0) and not counts[scene["segs"]:].any()
    ordered = _wavefront(scene, rays, order_levels=True)
    _same(ordered, ref, name + " ordered")
    assert ordered["level_counts"].tolist() == counts.tolist()
    print("NODES edges %s: %d rays, level counts %s, %.2f s" % (name, len(rays), counts.tolist(), time.perf_counter() - t0))
    # R2: the frame's primary rays at supersample 1
    if c["ss"] == 1:
        blob = rt_host.flatten_scene(scene)
        w, h = c["w"], c["h"]
        want = ou.c_oracle_render(blob, w, h) if c["rows"] is None else ou.c_oracle_rows(blob, w, h, c["rows"])
        frame = got["rgba"][:c["n_primary"]].tobytes()
        if name.startswith("soak_"):
            assert frame == want                                                          # as the strict frame there: exactly
        else:
            assert ou.max_lsb(frame, want)[0] <= 1


# ------------------------------------------------------------------ A (ii) the walked nodes == R2
_texture_indices = {}


def _sampled_textures(name):
    """The texture indices that are the sampler of a hit node of the case's trees (the restatement's side alone)."""
    if name not in _texture_indices:
        objs = case(name)["scene"]["objects"]
        codes = _records(oracle_of(name)[1])[:, 1].astype(int)
        hit = {int(c) >> 1 for c in codes if c >= 0}
        _texture_indices[name] = {objs[i]["mtl"]["sampler"]["texture"] for i in hit if objs[i]["mtl"]["sampler"]["kind"] == rt_host.SAMPLER_TEXTURE}
    return _texture_indices[name]


def _conditions_on_the_restatement(name):
    """What makes the case the edge it is named for, from R2 alone (no GPU result enters)."""
    c = case(name)
    scene = c["scene"]
    Q = _records(oracle_of(name)[1])
    if name == "max256x16":
        assert len(scene["objects"]) == 256 and len(scene["lights"]) == 16
        assert (Q[:, 1].astype(int) >> 1).max() >= 250                                   # a sphere at the end of the table is hit ...
        fewer = _records(oracle_of(name, _max_scene(15), "15 lights")[1])
        assert fewer.shape == Q.shape and (fewer[:, 0:12] == Q[:, 0:12]).all()
        assert (fewer[:, 15] != Q[:, 15]).sum() > 20                                     # ... and light 15 lights nodes
    if name.startswith("h8_tex"):
        seen = set().union(*[_sampled_textures(n) for n, _, _, _ in tu.ORACLE_SCENES])
        assert seen == set(range(tu.MAX_TEXTURES)), sorted(set(range(tu.MAX_TEXTURES)) - seen)
    if name == "default14_rows":
        # a transparent occluder divides the intensity (quirk q2): a primary hit that is lit brighter than it is with the glass taken away
        w, h = c["w"], c["h"]
        bare = copy.deepcopy(scene)
        bare["objects"] = [o for o in bare["objects"] if o["mtl"]["albedo"][4] == 0]
        assert len(bare["objects"]) == len(scene["objects"]) - 2
        pa, pb = hu.Probe(scene, w, h), hu.Probe(bare, w, h)
        ra = np.array([pa.root(x, y) for y in c["rows"] for x in range(w)])
        rb = np.array([pb.root(x, y) for y in c["rows"] for x in range(w)])
        same_point = (ra[:, 2] == rb[:, 2]) & (ra[:, 1] >= 0)                             # the same surface point in both
        brighter = same_point & (ra[:, 15] > rb[:, 15]) & (rb[:, 15] > 0)
        assert brighter.sum() > 20, int(brighter.sum())
        return ra
    return None


@pytest.mark.parametrize("name", list(CASES))
def test_edge_scene_nodes_are_the_restatements(lib, name):
    c = case(name)
    scene, segs = c["scene"], c["node_segs"]
    roots = _conditions_on_the_restatement(name)
    oracle, trees = oracle_of(name)
    t0 = time.perf_counter()
    r = rt_host.Renderer(scene, 0, lib)
    try:
        levels = nu.walk(lib, r, c["micro"], segs)
        first = nu.shade(lib, r, c["rays"][:c["n_primary"]]) if roots is not None else None
    finally:
        r.close()
    assert len(trees) == 4 * N_CAMERAS and len(levels) <= segs
    n_nodes, n_hits, n_children = nu.assert_nodes_are_the_restatements(levels, trees, oracle, scene["objects"], segs, name)
    print("NODES edges %s segs %d: %d nodes in %d levels, %d hits, %d two-child nodes, %.2f s"
          % (name, segs, n_nodes, len(levels), n_hits, n_children, time.perf_counter() - t0))
    assert n_hits > 0
    if name == "no_lights":
        for lv in levels:
            assert not lv["nodes"]["diffuse"].view(np.uint64).any() and not lv["nodes"]["specular"].view(np.uint64).any()   # +0.0, every node
    if roots is not None:                                                                 # the rows' primary hits, whose shadows the condition is about
        hit = roots[:, 1] >= 0
        assert (first["object"] == np.where(hit, roots[:, 1].astype(int) >> 1, -1)).all()
        assert nu.same_bits(first["diffuse"], roots[:, 15]) and nu.same_bits(first["t"], roots[:, 2])


# ------------------------------------------------------------------ A (iii) level 1's hit record == rt_trace_rays' hits
@pytest.mark.parametrize("name", list(CASES))
def test_edge_scene_level_one_is_the_hit_record_of_trace_rays(lib, name):
    c = case(name)
    t0 = time.perf_counter()
    hits = rt_host.trace_rays(c["scene"], c["rays"], want=("hits",))["hits"]
    nodes = rt_host.shade_rays(c["scene"], c["rays"], lib=lib)
    miss = np.array([h is None for h in hits])
    assert len(hits) == len(nodes) and ((nodes["object"] < 0) == miss).all()
    nd, H = nodes[~miss], [h for h in hits if h is not None]
    assert (nd["object"] == np.array([h["object"] for h in H], np.int64)).all() and (nd["inside"] == np.array([h["inside"] for h in H], np.int64)).all()
    want = np.array([[h["t"], *h["point"], *h["normal"], h["u"], h["v"]] for h in H], np.float64).reshape(len(H), 9)
    got = np.column_stack([nd["t"], nd["point"], nd["normal"], nd["u"], nd["v"]])
    assert nu.same_bits(got, want), int((got.view(np.uint64) != want.view(np.uint64)).any(axis=1).sum())
    print("NODES edges %s level 1: %d rays, %d hits, %d inside, %.2f s" % (name, len(hits), len(H), int(nd["inside"].sum()), time.perf_counter() - t0))
    assert len(H) > 0


# ------------------------------------------------------------------ a list in which every ray misses
def _all_miss_rays(n=1000):
    """cfg1 has no skybox, and nothing above y = 3: rays that start above it and point upwards meet no sphere."""
    rng = np.random.default_rng(31)
    rays = np.empty((n, 6), np.float64)
    rays[:, 0:3] = rng.uniform(-50.0, 50.0, (n, 3)) + np.array([0.0, 100.0, 0.0])
    d = rng.normal(size=(n, 3))
    d[:, 1] = np.abs(d[:, 1]) + 0.1
    rays[:, 3:6] = rt_host.normal3d(d)
    return rays


def test_a_list_of_misses_is_one_level_of_the_miss_colour(lib):
    scene = rt_host.load_scene("cfg1")
    assert all(o["origin"][1] + math.sqrt(o["r2"]) < 3.0 for o in scene["objects"])
    rays = _all_miss_rays()
    t0 = time.perf_counter()
    ref = rt_host.trace_rays(scene, rays, segs=8, want=("rgb", "rgba"))
    got = _wavefront(scene, rays, segs=8)
    _same(got, ref, "all miss")
    assert got["level_counts"].tolist() == [len(rays)] + [0] * 15
    assert (got["rgba"] == np.array([255, 0, 0, 255], np.uint8)).all() and (got["rgb"] == np.array([1.0, 0.0, 0.0])).all()   # main.js:231: red
    print("NODES edges all-miss cfg1: level counts %s, %.2f s" % (got["level_counts"].tolist(), time.perf_counter() - t0))


# ------------------------------------------------------------------ B. the host loop
def _default14_list():
    scene = rt_host.load_scene("default14")
    cams = ru.draw_cameras(scene, N_CAMERAS, 2009, outside_radius=5000.0)
    return scene, np.concatenate([rt_host.primary_rays(64, 36, scene), ru.micro_rays(cams, float(scene.get("fovDeg", 60)))])


@pytest.mark.parametrize("want", [("rgb", "rgba"), ("rgb",), ("rgba",)], ids=["both", "rgb", "rgba"])
def test_depth_zero_is_black_without_a_level(lib, want):
    """A scene of depth 0 traced at "the scene's depth": no level is shaded, so no fold writes the outputs - the loop itself has to
    (main.js:221).  The ray with a NaN in it is whatever rt_trace_rays makes of it."""
    scene = _h8(segs=0)
    rays = np.concatenate([rt_host.primary_rays(40, 24, scene), ru.micro_rays(ru.draw_cameras(scene, 8, 77), 60.0)])
    bad = 501
    rays[bad, 4] = math.nan
    ref = rt_host.trace_rays(scene, rays, segs=0, want=want)
    got = _wavefront(scene, rays, segs=0, want=want)
    _same(got, ref, "depth 0")
    assert not got["level_counts"].any()
    keep = np.arange(len(rays)) != bad
    if "rgb" in want:
        assert not got["rgb"][keep].view(np.uint64).any()                              # [0, 0, 0], +0.0
    if "rgba" in want:
        assert (got["rgba"][keep] == np.array([0, 0, 0, 255], np.uint8)).all()
    print("NODES edges depth 0 (%s): %d rays, level counts %s" % ("+".join(want), len(rays), got["level_counts"].tolist()))


@pytest.mark.parametrize("segs", [1, 2])
def test_depths_one_and_two(lib, segs):
    scene, rays = _default14_list()
    ref = rt_host.trace_rays(scene, rays, segs=segs, want=("rgb", "rgba"))
    got = _wavefront(scene, rays, segs=segs)
    _same(got, ref, segs)
    counts = got["level_counts"]
    assert counts[0] == len(rays) and (counts[1] > 0) == (segs == 2) and not counts[segs:].any()   # 1: no spawn at all; 2: one, and its level the deepest
    print("NODES edges default14 segs %d: level counts %s" % (segs, counts.tolist()))


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_small_lists(lib, n):
    scene, rays = _default14_list()
    rays = rays[np.random.default_rng(n).choice(len(rays), n, replace=False)] if n > 1 else rays[2304:2305]   # (the one ray: from inside a glass sphere)
    ref = rt_host.trace_rays(scene, rays, segs=8, want=("rgb", "rgba"))
    got = _wavefront(scene, rays, segs=8)
    _same(got, ref, n)
    counts = got["level_counts"]
    assert counts[0] == n and counts[1] > 0
    print("NODES edges default14 n %d: level counts %s" % (n, counts.tolist()))


@pytest.mark.parametrize("want", [("rgb",), ("rgba",)], ids=["rgb", "rgba"])
@pytest.mark.parametrize("which", ["default14", "all_miss"])
def test_one_output(lib, which, want):
    scene, rays = _default14_list() if which == "default14" else (rt_host.load_scene("cfg1"), _all_miss_rays())
    ref = rt_host.trace_rays(scene, rays, segs=8, want=want)
    got = _wavefront(scene, rays, segs=8, want=want)
    _same(got, ref, (which, want))
    counts = got["level_counts"]
    assert counts[0] == len(rays) and ((counts[7] > 0) if which == "default14" else not counts[1:].any())   # deep trees / a tree of one level
    print("NODES edges %s %s alone: level counts %s" % (which, want[0], counts.tolist()))


# ---- stars: ray i keeps pix = i across chunks
_stars = {}


def stars_list():
    if not _stars:
        scene = rt_host.load_scene("default14_stars")
        _stars.update(scene=scene, rays=rt_host.primary_rays(640, 412, scene))
        assert len(_stars["rays"]) == 263680 == (1 << 18) + 1536                          # one full chunk, and a second with base 262 144
    return _stars


def stars_result(seed):
    """rt_host.trace_rays' wavefront result of the two-chunk stars list (no stats): computed once, shared, never changed."""
    s = stars_list()
    if ("got", seed) not in s:
        s[("got", seed)] = _wavefront(dict(s["scene"], starsSeed=seed), s["rays"])
    return s[("got", seed)]


def _dense_stars(scene):
    """A copy with half the sky lit (threshold 0.5, scale 1.0): every other sky ray shows its pix."""
    s = copy.deepcopy({k: v for k, v in scene.items() if k != "textures"})
    s["textures"] = scene["textures"]
    for o in s["objects"]:
        if o["mtl"]["sampler"]["kind"] == rt_host.SAMPLER_STARS:
            o["mtl"]["sampler"].update(threshold=0.5, scale=1.0)
    return s


def test_stars_keep_their_pixel_across_chunks(lib):
    """The frame's list in row order, seeds 0 and 7: its second chunk (rows 409.6 to 411) is floor, which mirrors nothing, so there the
    two seeds agree in the recursive trace itself.  The same rays in reverse order, with half the sky lit, put 1 536 sky rays into the
    second chunk: there the seeds must differ, and every lit one is decided by pix = 262 144 + i."""
    s = stars_list()
    t0 = time.perf_counter()
    seen = []
    for seed in (0, 7):
        ref = rt_host.trace_rays(dict(s["scene"], starsSeed=seed), s["rays"], want=("rgb", "rgba"))
        got = stars_result(seed)
        _same(got, ref, seed)
        assert got["level_counts"][0] == len(s["rays"])
        seen.append(ref["rgb"])
    assert seen[0].tobytes() != seen[1].tobytes()
    dense, back = _dense_stars(s["scene"]), s["rays"][::-1]
    second = slice(1 << 18, None)
    seen = []
    for seed in (0, 7):
        ref = rt_host.trace_rays(dict(dense, starsSeed=seed), back, want=("rgb", "rgba"))
        got = _wavefront(dict(dense, starsSeed=seed), back)
        _same(got, ref, ("reversed", seed))
        seen.append(ref["rgb"][second])
    lit = [(x[:, 0] > 0).sum() for x in seen]
    assert min(lit) > 500 and (seen[0] != seen[1]).any(axis=1).sum() > 500, lit          # the seed shows inside the second chunk
    print("NODES edges default14_stars 640x412: level counts %s; reversed, half the sky lit: %d and %d stars among the second chunk's 1536 rays, %.2f s"
          % (stars_result(0)["level_counts"].tolist(), lit[0], lit[1], time.perf_counter() - t0))


def test_stars_keep_their_pixel_across_a_halved_chunk(lib):
    from test_gpu_nodes import _four_spheres
    scene = _four_spheres()
    sky = max(scene["objects"], key=lambda o: o["r2"])
    sky["mtl"]["sampler"] = {"kind": rt_host.SAMPLER_STARS, "threshold": 0.5, "scale": 1.0}
    rays = rt_host.primary_rays(400, 225, scene)
    t0 = time.perf_counter()
    ref = rt_host.trace_rays(scene, rays, segs=16, want=("rgb", "rgba"))
    got = _wavefront(scene, rays, segs=16)
    _same(got, ref, "halved")
    counts = got["level_counts"]
    assert counts[0] == 90000 and counts.sum() > 2 ** 21                                 # more nodes than one chunk may hold: it was halved
    assert len({bytes(p) for p in ref["rgba"]}) > 100 and ref["rgb"].tobytes() != rt_host.trace_rays(dict(scene, starsSeed=7), rays, segs=16)["rgb"].tobytes()
    print("NODES edges four spheres with stars 400x225 segs 16: %d nodes, level counts %s, %.2f s" % (int(counts.sum()), counts.tolist(), time.perf_counter() - t0))


@pytest.mark.parametrize("n", [263680, 65])
def test_stats_from_python(lib, n):
    s = stars_list()
    rays = s["rays"] if n == len(s["rays"]) else s["rays"][300 * 640 + 200:][:n]       # (the short list: floor and spheres, deep trees)
    plain = stars_result(0) if n == len(s["rays"]) else _wavefront(s["scene"], rays)
    t0 = time.perf_counter()
    got = nu.trace_wavefront_abi(lib, s["scene"], rays, with_stats=True)
    st = got["stats"]
    assert st.pixels == n and st.kernel_ms > 0 and st.total_ms >= st.kernel_ms
    assert got["rgb"].tobytes() == plain["rgb"].tobytes() and got["rgba"].tobytes() == plain["rgba"].tobytes()
    assert got["level_counts"].tolist() == plain["level_counts"].tolist()
    print("NODES edges stats n %d: kernel %.3f ms of %.3f ms, level counts %s, %.2f s"
          % (n, st.kernel_ms, st.total_ms, got["level_counts"].tolist(), time.perf_counter() - t0))


# ------------------------------------------------------------------ D. fold alone, against fold_nodes_host
ORDINARY = [0.125, 0.3, 0.5, 0.7, 0.9]
SPECIAL = [0.0, -0.0, 1.0, float(np.nextafter(1.0, 0.0)), float(np.nextafter(1.0, 2.0)), -0.25, -2.0, 1.5, 1e308, math.inf, -math.inf, math.nan]
FOLD_SEED = 4


def _draw(rng, shape):
    v = np.where(rng.random(shape) < 0.7, rng.choice(ORDINARY, shape), rng.choice(SPECIAL, shape))
    return v.astype(np.float64)


def fold_case(n):
    """-> nodes, links, child_rgb: crafted values, every combination of missing links, shared children, a third of the nodes a miss."""
    rng = np.random.default_rng(FOLD_SEED * 1000 + n)
    m = max(1, n // 2 + 3)                                                               # fewer children than links: two parents may share one
    nodes = np.zeros(n, rt_host.NODE_DTYPE)
    nodes["object"] = np.where(np.arange(n) % 3 == 2, -1, rng.integers(0, 256, n))
    nodes["t"], nodes["point"], nodes["normal"] = rng.normal(size=n), rng.normal(size=(n, 3)), rng.normal(size=(n, 3))
    nodes["sample"] = _draw(rng, (n, 3))
    for f in ("diffuse", "specular", "ambient", "reflect_weight", "refract_weight"):
        nodes[f] = _draw(rng, n)
    links = rng.integers(0, m, (n, 2)).astype(np.int32)
    none = rng.integers(0, 4, n)                                                         # neither, the first, the second, both slots without a child
    links[(none & 1) != 0, 0] = -1
    links[(none & 2) != 0, 1] = -1
    nodes["children"] = (links[:, 0] >= 0) + 2 * (links[:, 1] >= 0)
    return nodes, links, _draw(rng, (m, 3))


def _fold_census(nodes, links, child_rgb, want):
    """(NaN channels, channels clamped to 1, channels decided by sample * ambient) among the hits of an expected result."""
    n = len(nodes)
    s, hit = nodes["sample"], (nodes["object"] >= 0)[:, None]
    re, rf = np.zeros((n, 3)), np.zeros((n, 3))
    with np.errstate(all="ignore"):
        if links is not None:
            for k, (dst, w) in enumerate(((re, nodes["reflect_weight"]), (rf, nodes["refract_weight"]))):
                sel = links[:, k] >= 0
                dst[sel] = child_rgb[links[sel, k]] * w[sel, None]
        shade = s * nodes["diffuse"][:, None] + s * nodes["specular"][:, None] + re + rf
        amb = s * nodes["ambient"][:, None]
        inner = np.where(np.isnan(shade), np.nan, np.where(1.0 < shade, 1.0, shade))
        ambient = hit & ~np.isnan(amb) & ~np.isnan(inner) & (amb > inner)
        clamped = hit & (shade > 1.0) & ~(amb > 1.0) & ~np.isnan(amb)
    assert (want[ambient] == amb[ambient]).all() and (want[clamped] == 1.0).all()
    return np.array([int((hit & np.isnan(want)).sum()), int(clamped.sum()), int(ambient.sum())])


def test_fold_of_crafted_nodes_is_fold_nodes_host(lib):
    t0 = time.perf_counter()
    census = np.zeros(3, np.int64)
    r = rt_host.Renderer(rt_host.load_scene("h8"), 0, lib)
    try:
        for n in (1, 255, 257):
            nodes, links, child = fold_case(n)
            assert (nodes["object"] < 0).sum() == n // 3
            with np.errstate(all="ignore"):
                want = rt_host.fold_nodes_host(nodes, links, child)
                bare = rt_host.fold_nodes_host(nodes, None, None)
                want_bytes, bare_bytes = ru.store_rule(want), ru.store_rule(bare)
            census += _fold_census(nodes, links, child, want) + _fold_census(nodes, None, None, bare)
            rgb, rgba = nu.fold(lib, r, nodes, links, child)
            assert rgb.tobytes() == want.tobytes(), (n, int((rgb.view(np.uint64) != want.view(np.uint64)).sum()))
            assert rgba.tobytes() == want_bytes.tobytes(), n
            rgb0, rgba0 = nu.fold(lib, r, nodes)                                         # links=None: every child counts as [0, 0, 0]
            assert rgb0.tobytes() == bare.tobytes() and rgba0.tobytes() == bare_bytes.tobytes(), n
            only, none = nu.fold(lib, r, nodes, links, child, want_rgba=False)           # (the other buffer's canaries: nodes_util.fold)
            assert none is None and only.tobytes() == want.tobytes(), n
            none, only = nu.fold(lib, r, nodes, links, child, want_rgb=False)
            assert none is None and only.tobytes() == want_bytes.tobytes(), n
    finally:
        r.close()
    assert (census >= 20).all(), census.tolist()                                         # asserted on the reference alone
    print("NODES edges fold n 1, 255, 257: %d NaN channels, %d clamped to 1, %d decided by sample * ambient, %.2f s"
          % (census[0], census[1], census[2], time.perf_counter() - t0))


# ------------------------------------------------------------------ E. shade with an order and tags together
def test_an_order_with_tags_gives_the_plain_calls_bytes(lib):
    """pix and path are indexed by ray, not by work-item: under a shuffled order every node keeps the star its own tags draw."""
    scene = _dense_stars(rt_host.load_scene("default14_stars"))                          # half the sky lit: a few hundred rays show their tags
    cams = ru.draw_cameras(scene, N_CAMERAS, 2015)
    rays = np.concatenate([ru.micro_rays(cams, float(scene.get("fovDeg", 60))), rt_host.primary_rays(32, 18, scene)])
    n = len(rays)
    rng = np.random.default_rng(15)
    pix, path = rng.integers(0, 2 ** 32, n, dtype=np.uint64).astype(np.uint32), rng.integers(1, 2 ** 30, n).astype(np.uint32)
    perm = rng.permutation(n).astype(np.uint32)
    r = rt_host.Renderer(scene, 0, lib)
    try:
        plain = nu.shade(lib, r, rays, pix, path)
        assert nu.shade(lib, r, rays, pix, path, order=perm).tobytes() == plain.tobytes()
        untagged = nu.shade(lib, r, rays)
        moved = nu.shade(lib, r, rays, pix[perm], path[perm])
    finally:
        r.close()
    assert rt_host.shade_rays(scene, rays, pix=pix, path=path, order="binned", lib=lib).tobytes() == plain.tobytes()   # the library's own order
    sky = plain["sample"][:, 0] != untagged["sample"][:, 0]
    assert sky.sum() > 50 and moved.tobytes() != plain.tobytes()                         # the tags show
    rest = plain.copy()
    rest["sample"] = untagged["sample"]
    assert rest.tobytes() == untagged.tobytes()                                          # ... in the sample, and nowhere else
    print("NODES edges default14_stars order with tags: %d rays, %d whose star the tags decide" % (n, int(sky.sum())))
