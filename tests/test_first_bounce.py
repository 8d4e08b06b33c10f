"""First-bounce sets of the launch table (csrc/rt_block.h: rt_first_bounce_set; CPU only, the host build of the table).

With RT_TABLE_FIRST_BOUNCE (bit 7 of rt_scene_launch_table's `ranked`) word 3 of a block that shows a mirror also names, with bit 31 and
bits 18..30, the loop-order spheres a ray reflected at a primary hit of the block can meet.  The trace kernel then tests only those at
the node after the primary, so the set has to be conservative: for every stating entry and every sample of its block whose ray tree has
a second node, that node's ray (origin and direction from the C restatement's per-sample probe, oracle/rt_oracle.c) is held against
EVERY loop sphere with the reference's own discriminant and epsilon rule (main.js:420-439) - no sphere outside the entry's set may be
met at t >= epsilon, and the sphere the node actually hit is in the set.

The probe keeps 64 nodes and records a node after its children; it reads the scene at depth 2, where the tree is the primary node and
its reflection child (neither the primary hit, nor the reflected ray, nor the table's statement depends on the depth beyond "at least 2")."""
import copy
import ctypes as C
import math

import numpy as np
import pytest

import oracle_util as ou
import rt_host
from soak_gpu_parity import draw_scene, look_at

PLAIN, CELLS = 1 | 2 | 4, 1 | 2 | 4 | 32
FIRST_BOUNCE = CELLS | 128
PROBE_WORDS, PROBE_NODES = 24, 64
H8_4K_SAVED = 60000             # the threshold the change was decided on (docs/EVIDENCE.md, first-bounce sets, step 0): sphere tests saved per headline launch
SEEDS = range(910000, 910070)


@pytest.fixture(scope="module")
def lib(built):
    return rt_host.load_library()


def table(lib, blob, w, h, flags, tiles=None):
    t = rt_host.RtTiles(*(tiles or (h, 0, 1, 1)))
    buf = C.create_string_buffer(blob, len(blob))
    n, nb = C.c_uint32(), C.c_uint32()
    assert lib.rt_scene_launch_table(buf, len(blob), w, h, C.byref(t), flags, None, C.byref(n), C.byref(nb)) == 0, lib.rt_last_error()
    out = (C.c_uint32 * (4 * 8 * ((nb.value + 7) // 8)))()
    assert lib.rt_scene_launch_table(buf, len(blob), w, h, C.byref(t), flags, out, C.byref(n), C.byref(nb)) == 0, lib.rt_last_error()
    return np.frombuffer(out, dtype=np.uint32).reshape(-1, 4).copy()


def stating(tab):
    """The entries that state a set: rows of the table with bit 31 of word 3 (never a sky run, never an empty slot, never beside a cell)."""
    rows = tab[tab[:, 3] >> 31 == 1]
    for w0, w1, _, w3 in rows:
        assert (int(w0) >> 11) & 15 and not int(w1) >> 31 and (int(w3) >> 16) & 3 in (1, 2), (w0, w1, w3)
    return rows


def enclosing(scene):
    """Scene index of the sphere the library takes out of the loops (rt_tables.cpp: enclosing_sphere), or None."""
    ob, cam = scene["objects"], scene["camera"]["origin"]
    for e, s in enumerate(ob):
        re = math.sqrt(s["r2"])
        lim = re * (1.0 - 1e-6)
        ok = re > 0.0 and math.dist(cam, s["origin"]) < lim and all(math.dist(li, s["origin"]) < lim for li in scene["lights"])
        ok = ok and all(math.dist(o["origin"], s["origin"]) + math.sqrt(o["r2"]) < lim for j, o in enumerate(ob) if j != e)
        if ok and len(ob) > 1:
            return e
    return None


def loop_order(scene):
    """Scene indices in the product kernel's loop order: the enclosing sphere, if any, is outside the loops."""
    sky = enclosing(scene)
    return [i for i in range(len(scene["objects"])) if i != sky]


def check(lib, scene, w, h, tiles=None):
    """Every stating entry of the frame's table, every sample of its block: returns (stating entries, second nodes held, sphere tests saved -
    counted per wave: a wave with at least one bouncing sample walks its entry's set instead of every loop sphere)."""
    blob = rt_host.flatten_scene(scene)
    ss = scene.get("supersample", 1)
    assert ss in (1, 2)
    rows = stating(table(lib, blob, w, h, FIRST_BOUNCE, tiles))
    order = loop_order(scene)
    sky = enclosing(scene)
    if (scene["segs"] < 2 or len(order) > 13 or any(o["mtl"]["albedo"][4] > 0 for o in scene["objects"])
            or (sky is not None and not scene["objects"][sky]["mtl"]["albedo"][3] <= 0)):
        assert len(rows) == 0
    if len(rows) == 0:
        return 0, 0, 0
    c = ou.c_oracle()
    c.oracle_probe_sample.restype = C.c_int
    c.oracle_probe_sample.argtypes = [C.c_void_p, C.c_size_t, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p]
    blob2 = rt_host.flatten_scene(dict(scene, segs=2))
    buf = C.create_string_buffer(blob2, len(blob2))
    rec = np.zeros(PROBE_NODES * PROBE_WORDS)
    nodes = rec.reshape(PROBE_NODES, PROBE_WORDS)
    rays, sets, hits = [], [], []
    saved = 0
    for w0, _, _, w3 in rows:
        bouncing = set()                                       # the block's columns (waves) with a sample that bounces
        tile_x, rows_valid, frow0 = int(w0) & 2047, (int(w0) >> 11) & 15, int(w0) >> 15
        fb = (int(w3) >> 18) & 0x1fff
        cands = [int(w3) & 255] + ([(int(w3) >> 8) & 255] if (int(w3) >> 16) & 3 == 2 else [])
        assert fb and fb >> len(order) == 0, (w0, w3)
        # a mirror among the candidates, and every mirror among them in the set (its own rays may meet it again: kept in, not argued away)
        mirrors = [k for k in cands if scene["objects"][order[k]]["mtl"]["albedo"][3] > 0]
        assert mirrors and all(fb >> k & 1 for k in mirrors), (w0, w3)
        for sy in range(frow0 * ss, (frow0 + rows_valid) * ss):
            for sx in range(tile_x * 32 * ss, min((tile_x + 1) * 32 * ss, w * ss)):
                rec[:] = 0.0
                assert c.oracle_probe_sample(buf, len(blob2), w, h, sx, sy, rec.ctypes.data) == 0
                second = nodes[(nodes[:, 23] == 1.0) & (nodes[:, 0] == 2.0)]
                if len(second):
                    assert len(second) == 1
                    rays.append(np.concatenate((second[0, 19:22], second[0, 9:12])))
                    sets.append(fb)
                    hits.append(int(second[0, 1]))
                    bouncing.add((sx // (8 * ss)) % 4)
        saved += len(bouncing) * (len(order) - bin(fb).count("1"))
    if not rays:
        return len(rows), 0, 0
    rays, sets, hits = np.array(rays), np.array(sets, dtype=np.int64), np.array(hits, dtype=np.int64)
    p, d = rays[:, 0:3], rays[:, 3:6]
    eps = 0.001                                                 # (main.js:429-436: the literal, whatever the scene's own epsilon)
    for k, si in enumerate(order):
        o = scene["objects"][si]
        L = np.array(o["origin"], dtype=np.float64) - p         # main.js:422-425
        tca = (d * L).sum(axis=1)
        d2 = (L * L).sum(axis=1) - tca * tca
        met = ~(d2 > o["r2"])
        thc = np.sqrt(np.where(met, o["r2"] - d2, 0.0))
        t0, t1 = tca - thc, tca + thc
        lo, hi = np.minimum(t0, t1), np.maximum(t0, t1)
        met &= ~((lo < eps) & (hi < eps))                       # main.js:428-438: the nearer root, or the farther one, or nothing
        outside = (sets >> k) & 1 == 0
        bad = met & outside
        assert not bad.any(), (scene.get("name"), w, h, "loop sphere", k, "met by", int(bad.sum()), "rays of entries that leave it out", rays[bad][0].tolist())
        hit_here = (hits >> 1) == si
        assert not (hit_here & outside).any(), (scene.get("name"), w, h, k)
    return len(rows), len(rays), saved


def h8(**kw):
    s = rt_host.load_scene("h8")
    s.update(kw)
    return s


def two_mirrors():
    """Two mirrors facing each other over a checker floor, the camera close: some blocks graze a silhouette (no statement, or a wide set),
    and each mirror shows the other - and itself in the other - so the sets hold two and three spheres."""
    s = h8()
    floor = next(o for o in s["objects"] if o["r2"] == 250000.0)
    sky = next(o for o in s["objects"] if o["r2"] == 25000000)
    mirror = next(o for o in s["objects"] if o["mtl"]["albedo"][3] > 0 and o["r2"] == 1)
    a, b = copy.deepcopy(mirror), copy.deepcopy(mirror)
    a["origin"], a["r2"] = [-1.3, 1.2, 0.0], 1.44
    b["origin"], b["r2"] = [1.3, 1.2, 0.0], 1.44
    s["objects"] = [a, b, floor, sky]
    s["camera"] = look_at([0.2, 1.4, 3.6], [0.0, 1.1, 0.0], [0.0, 1.0, 0.0])
    s["name"] = "two_mirrors"
    return s


def bench_moving_camera(scene, k, n):
    """bench.py's moving_camera, restated: camera k of n on a slow orbit around the scene's own camera position."""
    o = scene["camera"]["origin"]
    r = math.hypot(o[0], o[2]) or 10.0
    a0 = math.atan2(o[0], o[2])
    a = a0 + 0.35 * math.sin(2.0 * math.pi * (k + 0.37) / n) + 0.02
    return look_at([r * math.sin(a), o[1] + 0.3 * math.cos(2.0 * math.pi * k / n) + 0.05, r * math.cos(a)], [0.1, 1.5, 0.0], [0.0, 1.0, 0.0])


def test_h8_headline_frame(lib):
    """3840x2160: every stating entry, every sample; and not vacuously - at least the saving the change was decided on."""
    entries, held, saved = check(lib, h8(), 3840, 2160)
    print("h8 3840x2160: %d stating entries, %d second nodes held, %d tests saved" % (entries, held, saved))
    assert saved >= H8_4K_SAVED and held > 0, (entries, held, saved)


def test_h8_ragged_size(lib):
    """1001x563: blocks only partly inside the frame."""
    entries, held, _ = check(lib, h8(), 1001, 563)
    assert entries > 0 and held > 0


def test_h8_interleaved_tiles(lib):
    """One rank's tiles of two interleaved ranks (16-row tiles, every second one)."""
    entries, held, _ = check(lib, h8(), 1001, 563, tiles=(16, 1, 2, (563 // 16) // 2))
    assert entries > 0 and held > 0


def test_h8_supersample_2(lib):
    entries, held, _ = check(lib, h8(supersample=2), 1001, 563)
    assert entries > 0 and held > 0


def test_h8_moving_camera(lib):
    """The 64 cameras of bench.py's moving-camera leg."""
    total = 0
    for k in range(64):
        s = h8()
        s["camera"] = bench_moving_camera(s, k, 64)
        total += check(lib, s, 1280, 720)[1]
    assert total > 0


def test_h8_depth_8(lib):
    entries, held, _ = check(lib, rt_host.load_scene("h8_d8"), 1920, 1080)
    assert entries > 0 and held > 0


def test_two_mirrors_facing_each_other(lib):
    """Blocks that graze a silhouette state nothing or a wide set; whatever is stated must hold."""
    s = two_mirrors()
    entries, held, _ = check(lib, s, 1280, 720)
    assert entries > 0 and held > 0
    tab = table(lib, rt_host.flatten_scene(s), 1280, 720, FIRST_BOUNCE)
    live = tab[((tab[:, 0] >> 11) & 15 != 0) & (tab[:, 1] >> 31 == 0)]
    order = loop_order(s)
    shows_mirror = np.array([any(s["objects"][order[k]]["mtl"]["albedo"][3] > 0 for k in ([int(w3) & 255] + ([(int(w3) >> 8) & 255] if (int(w3) >> 16) & 3 == 2 else [])))
                             if (int(w3) >> 16) & 3 else True for w3 in live[:, 3]])
    silent = live[shows_mirror & (live[:, 3] >> 31 == 0)]
    sizes = [bin((int(w3) >> 18) & 0x1fff).count("1") for w3 in stating(tab)[:, 3]]
    print("two mirrors 1280x720: %d stating entries (set sizes %s), %d mirror blocks without a statement" % (entries, sorted(set(sizes)), len(silent)))
    assert max(sizes) == 3                                     # the silhouettes are on screen: their blocks name every sphere (or nothing)


def test_no_statement_at_depth_1(lib):
    assert len(stating(table(lib, rt_host.flatten_scene(h8(segs=1)), 1920, 1080, FIRST_BOUNCE))) == 0


def test_no_statement_when_the_only_mirror_also_refracts(lib):
    s = h8()
    for o in s["objects"]:
        if o["mtl"]["albedo"][3] > 0:
            if o["r2"] == 0.25:
                o["mtl"]["albedo"][4] = 0.5
            else:
                o["mtl"]["albedo"][3] = 0.0
    assert len(stating(table(lib, rt_host.flatten_scene(s), 1920, 1080, FIRST_BOUNCE))) == 0


def reflecting_sky():
    """h8 with a skybox that reflects: it is outside the loops and the candidates, and a lane of a mirror's silhouette block that misses the
    mirror meets it - its reflected ray, thousands of units away, is at its first bounce too and no mirror's set bounds it."""
    s = h8()
    sky = next(o for o in s["objects"] if o["r2"] == 25000000)
    sky["mtl"]["albedo"][3] = 0.5
    return s


def test_no_statement_when_the_enclosing_sphere_reflects(lib):
    s = reflecting_sky()
    assert enclosing(s) is not None
    for wh in ((3840, 2160), (640, 360)):
        assert len(stating(table(lib, rt_host.flatten_scene(s), *wh, FIRST_BOUNCE))) == 0
    # (an enclosing sphere that does not reflect - h8's own - and no enclosing sphere at all both state)
    s = h8()
    s["objects"] = [o for o in s["objects"] if o["r2"] != 25000000]
    assert enclosing(s) is None and check(lib, s, 1001, 563)[1] > 0


def test_no_statement_with_14_loop_spheres(lib):
    for extra, expect in ((6, True), (7, False)):              # 13 loop spheres state, 14 do not
        s = h8()
        small = next(o for o in s["objects"] if o["r2"] == 0.25)
        for i in range(extra):
            o = copy.deepcopy(small)
            o["origin"] = [-3.0 + i, 3.5, -3.0]
            s["objects"].insert(0, o)
        assert len(loop_order(s)) == 7 + extra
        assert (len(stating(table(lib, rt_host.flatten_scene(s), 1920, 1080, FIRST_BOUNCE))) > 0) == expect


@pytest.mark.parametrize("scene,wh", [("h8", (3840, 2160)), ("h8", (1001, 563)), ("h8_ss2", (1001, 563)), ("h8_d8", (1280, 720)), ("two_mirrors", (1280, 720)),
                                      ("default14", (1280, 720)), ("lcg64_ss1", (1280, 720))])
def test_a_table_without_the_flag_is_todays_table(lib, scene, wh):
    """Word for word: the table built without RT_TABLE_FIRST_BOUNCE is the table built with it, bits 18..31 of the stating entries' word 3
    masked off - and an entry that states a set had no bit there before (no checker cell beside a set)."""
    s = h8(supersample=2) if scene == "h8_ss2" else (two_mirrors() if scene == "two_mirrors" else rt_host.load_scene(scene))
    if s.get("supersample", 1) > 2:
        s["supersample"] = 1
    blob = rt_host.flatten_scene(s)
    for tiles in (None, (16, 1, 2, (wh[1] // 16) // 2)):
        for base in (PLAIN, CELLS, CELLS | 64):
            plain, fb = table(lib, blob, *wh, base, tiles), table(lib, blob, *wh, base | 128, tiles)
            assert (plain[:, 3] >> 31 == 0).all()
            says = fb[:, 3] >> 31 == 1
            assert (plain[says, 3] >> 18 == 0).all()
            masked = fb.copy()
            masked[says, 3] &= 0x3ffff
            assert (masked == plain).all()
            if scene in ("default14", "lcg64_ss1"):              # a refracting scene, a scene of 64 spheres: nothing is stated
                assert not says.any()


def test_random_scenes(lib):
    """The GPU soaks' generator (tests/soak_gpu_parity.py: draw_scene), at the size drawn and at four times that size.  Not vacuous:
    the draws must yield statements (the counts are printed)."""
    entries = held = 0
    for seed in SEEDS:
        scene, w, h = draw_scene(seed, False, False)
        scene["name"] = "seed %d" % seed
        for k in (1, 4):
            a, b, _ = check(lib, scene, k * w, k * h)
            entries, held = entries + a, held + b
    print("random scenes: %d stating entries, %d second nodes held" % (entries, held))
    assert entries > 0 and held > 0, (entries, held)
