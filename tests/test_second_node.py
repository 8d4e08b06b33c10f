"""Second-node bits of the launch table (csrc/rt_block.h: rt_second_node_bits, rt_self_clear; CPU only, the host build of the table).

With RT_TABLE_SECOND_NODE (bit 8 of rt_scene_launch_table's `ranked`, beside bit 7) word 1 of an entry that states a first-bounce set says,
in bits 24..26, what the node after the primary may skip: SELF0 / SELF1 - the walk of the set may leave out candidate 0 / 1 (a mirror
whose own reflected rays cannot be accepted at it again, and which no other candidate's reflected rays can reach), SKY - nothing is left
of the set then, every reflected ray of the block meets no loop sphere.  The trace kernels read SELF0 / SELF1 and drop those tests; no
kernel reads SKY.  Every statement is held here against the reference's own rules: for every stating entry and every sample of its block
with a second node, that node's ray (the C restatement's per-sample probe at depth 2, as tests/test_first_bounce.py reads it) meets no
dropped candidate at t >= epsilon (main.js:420-439), and in a SKY entry no loop sphere at all.

Bits 27 and 28 - DARK0 / DARK1: no loop sphere can stand between light k and any second-node hit of the block (rt_cand_second_dark) - are
stated by the HOST build alone, with bit 9 of `ranked` beside bit 8: the device build does not know them and no kernel reads them (counted
below what pays: docs/EVIDENCE.md);
they are held the same way: a lit second-node hit of such an entry that faces light k has no loop sphere on its segment to the light
by the shadow rule (main.js:293-304).  tests/host/second_node_check.cpp runs the statement's arithmetic under ASan and UBSan.
"""
import copy
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import oracle_util as ou
import rt_host
from soak_gpu_parity import draw_scene
from test_first_bounce import CELLS, FIRST_BOUNCE, PLAIN, PROBE_NODES, PROBE_WORDS, SEEDS, bench_moving_camera, h8, loop_order, reflecting_sky, stating, table, two_mirrors

SECOND_NODE = FIRST_BOUNCE | 256
DARK = SECOND_NODE | 512
SELF0, SELF1, SKY = 1, 2, 4
# what profiles/count_second_node.py recorded for the headline frame before the kernel read a bit (profiles/second_node_counts.txt, per wave)
H8_4K_SKY_ENTRIES = 1389                        # the parent's one-sphere sets: all of them come out SKY
H8_4K_SKY_WAVES = 5375
H8_4K_SELF_DROPPED = 15178
H8_4K_DARK_ENTRIES = (659, 468)                 # entries that state DARK0 / DARK1 and are not SKY, and the waves whose shadow scan they would skip
H8_4K_DARK_WAVES = (2636, 1860)                 # (31 472 tests at 7 each: below the 40 000 the statement was to be built for)


@pytest.fixture(scope="module")
def lib(built):
    return rt_host.load_library()


def met(scene, order, k, p, d, eps=0.001):
    """Rays (p, d) against loop sphere k by the reference's discriminant and epsilon rule (main.js:420-439; the literal epsilon)."""
    o = scene["objects"][order[k]]
    L = np.array(o["origin"], dtype=np.float64) - p
    tca = (d * L).sum(axis=1)
    d2 = (L * L).sum(axis=1) - tca * tca
    ok = ~(d2 > o["r2"])
    thc = np.sqrt(np.where(ok, o["r2"] - d2, 0.0))
    t0, t1 = tca - thc, tca + thc
    return ok & ~((np.minimum(t0, t1) < eps) & (np.maximum(t0, t1) < eps))


def check(lib, scene, w, h, tiles=None):
    """Every stating entry of the frame's table, every sample of its block.  Returns counts: entries with a bit, SKY entries, second nodes
    held, and per wave (a column of the block with a bouncing sample) the SKY waves and the tests the SELF bits drop."""
    blob = rt_host.flatten_scene(scene)
    ss = scene.get("supersample", 1)
    assert ss in (1, 2)
    rows = stating(table(lib, blob, w, h, DARK, tiles))
    out = {"entries": 0, "sky_entries": 0, "held": 0, "sky_waves": 0, "self_dropped": 0, "dark_entries": [0, 0], "dark_waves": [0, 0], "dark_held": 0}
    if len(rows) == 0:
        return out
    order = loop_order(scene)
    c = ou.c_oracle()
    c.oracle_probe_sample.restype = C.c_int
    c.oracle_probe_sample.argtypes = [C.c_void_p, C.c_size_t, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p]
    blob2 = rt_host.flatten_scene(dict(scene, segs=2))
    buf = C.create_string_buffer(blob2, len(blob2))
    rec = np.zeros(PROBE_NODES * PROBE_WORDS)
    nodes = rec.reshape(PROBE_NODES, PROBE_WORDS)
    rays, drops, skies, hits, darks, hps, hns, wave_ids = [], [], [], [], [], [], [], []
    for e_i, (w0, w1, _, w3) in enumerate(rows):
        sn = (int(w1) >> 24) & 127
        assert sn >> 5 == 0, (w0, w1, w3)                      # bits 29, 30: nothing states them
        assert len(scene["lights"]) > 1 or not sn & 16, (w0, w1, w3)
        n_cand = (int(w3) >> 16) & 3
        cands = [int(w3) & 255] + ([(int(w3) >> 8) & 255] if n_cand == 2 else [])
        fb = (int(w3) >> 18) & 0x1fff
        assert not (sn & SELF1) or n_cand == 2, (w0, w1, w3)
        drop = sum(1 << cands[i] for i in range(len(cands)) if sn >> i & 1)
        # a dropped candidate is a mirror of the set; SKY says exactly "nothing is left of the set"
        assert drop & ~fb == 0 and all(scene["objects"][order[k]]["mtl"]["albedo"][3] > 0 for k in cands if drop >> k & 1), (w0, w1, w3)
        assert bool(sn & SKY) == (fb & ~drop == 0), (w0, w1, w3)
        if not sn:
            continue
        out["entries"] += 1
        out["sky_entries"] += 1 if sn & SKY else 0
        for kl in range(2):
            out["dark_entries"][kl] += 1 if sn >> (3 + kl) & 1 and not sn & SKY else 0
        bouncing = set()
        tile_x, rows_valid, frow0 = int(w0) & 2047, (int(w0) >> 11) & 15, int(w0) >> 15
        for sy in range(frow0 * ss, (frow0 + rows_valid) * ss):
            for sx in range(tile_x * 32 * ss, min((tile_x + 1) * 32 * ss, w * ss)):
                rec[:] = 0.0
                assert c.oracle_probe_sample(buf, len(blob2), w, h, sx, sy, rec.ctypes.data) == 0
                second = nodes[(nodes[:, 23] == 1.0) & (nodes[:, 0] == 2.0)]
                if len(second):
                    assert len(second) == 1
                    rays.append(np.concatenate((second[0, 19:22], second[0, 9:12])))
                    drops.append(drop)
                    skies.append(1 if sn & SKY else 0)
                    hits.append(int(second[0, 1]))
                    darks.append(sn >> 3)
                    hps.append(second[0, 3:6].copy())
                    hns.append(second[0, 6:9].copy())
                    wave_ids.append(4 * e_i + (sx // (8 * ss)) % 4)
                    bouncing.add((sx // (8 * ss)) % 4)
        out["sky_waves"] += len(bouncing) if sn & SKY else 0
        out["self_dropped"] += len(bouncing) * bin(sn & 3).count("1")
    if not rays:
        return out
    rays, drops, skies, hits = np.array(rays), np.array(drops, dtype=np.int64), np.array(skies, dtype=bool), np.array(hits, dtype=np.int64)
    p, d = rays[:, 0:3], rays[:, 3:6]
    out["held"] = len(rays)
    for k, si in enumerate(order):
        m = met(scene, order, k, p, d)
        bad = m & ((drops >> k) & 1 == 1)
        assert not bad.any(), (scene.get("name"), w, h, "dropped candidate", k, "met by", int(bad.sum()), "rays", rays[bad][0].tolist())
        bad = m & skies
        assert not bad.any(), (scene.get("name"), w, h, "loop sphere", k, "met by", int(bad.sum()), "rays of SKY entries", rays[bad][0].tolist())
        hit_here = (hits >= 0) & ((hits >> 1) == si)
        assert not (hit_here & (((drops >> k) & 1 == 1) | skies)).any(), (scene.get("name"), w, h, k)
    # DARK k: the second-node hits on lit loop spheres that face light k (an outside hit: the probe's normal points outwards)
    darks, hps, hns = np.array(darks, dtype=np.int64), np.array(hps), np.array(hns)
    on_loop = np.array([hc >= 0 and (hc >> 1) in order for hc in hits])
    lit = np.array([bool(on_loop[i]) and (scene["objects"][hits[i] >> 1]["mtl"]["albedo"][1] > 0 or scene["objects"][hits[i] >> 1]["mtl"]["albedo"][2] > 0)
                    for i in range(len(hits))])
    for kl, li in enumerate(scene["lights"][:2]):
        sraw = np.array(li, dtype=np.float64) - hps
        llen = np.sqrt((sraw * sraw).sum(axis=1))
        sv = sraw / llen[:, None]
        scans = lit & ((sv * hns).sum(axis=1) > 0.0) & ((darks >> kl) & 1 == 1)
        out["dark_held"] += int(scans.sum())
        out["dark_waves"][kl] = len(np.unique(np.array(wave_ids)[scans]))
        for k, si in enumerate(order):
            o = scene["objects"][si]
            L = np.array(o["origin"], dtype=np.float64) - hps          # main.js:293-304: the scan from the hit point towards the light
            tca = (sv * L).sum(axis=1)
            d2 = (L * L).sum(axis=1) - tca * tca
            ok = ~(d2 > o["r2"])
            thc = np.sqrt(np.where(ok, o["r2"] - d2, 0.0))
            t0, t1 = tca - thc, tca + thc
            t = np.where(t0 < 0.001, t1, t0)
            bad = scans & ok & ((hits >> 1) != si) & (t < llen) & ~(t < 0.001)
            assert not bad.any(), (scene.get("name"), w, h, "light", kl, "loop sphere", k, "shadows", int(bad.sum()), "second-node hits of DARK entries", hps[bad][0].tolist())
    return out


def bits(lib, scene, w, h):
    rows = stating(table(lib, rt_host.flatten_scene(scene), w, h, SECOND_NODE))
    return (rows[:, 1] >> 24) & 127 if len(rows) else np.zeros(0, dtype=np.uint32)


def test_h8_headline_frame(lib):
    """3840x2160: every entry with a bit, every sample; not vacuously - the parent's one-sphere sets all come out SKY, and the per-wave
    counts are at least what the change was decided on."""
    s = h8()
    r = check(lib, s, 3840, 2160)
    print("h8 3840x2160:", r)
    rows = stating(table(lib, rt_host.flatten_scene(s), 3840, 2160, SECOND_NODE))
    one = np.array([bin((int(w3) >> 18) & 0x1fff).count("1") == 1 for w3 in rows[:, 3]])
    assert one.sum() >= H8_4K_SKY_ENTRIES and ((rows[one, 1] >> 26) & 1 == 1).all()
    assert r["sky_entries"] >= H8_4K_SKY_ENTRIES and r["sky_waves"] >= H8_4K_SKY_WAVES and r["self_dropped"] >= H8_4K_SELF_DROPPED, r
    assert r["held"] > 0 and r["dark_held"] > 0, r
    assert all(r["dark_entries"][k] >= H8_4K_DARK_ENTRIES[k] and r["dark_waves"][k] >= H8_4K_DARK_WAVES[k] for k in range(2)), r


def test_h8_ragged_size(lib):
    r = check(lib, h8(), 1001, 563)
    assert r["entries"] > 0 and r["sky_entries"] > 0 and r["held"] > 0, r


def test_h8_interleaved_tiles(lib):
    r = check(lib, h8(), 1001, 563, tiles=(16, 1, 2, (563 // 16) // 2))
    assert r["entries"] > 0 and r["held"] > 0, r


def test_h8_supersample_2(lib):
    r = check(lib, h8(supersample=2), 1001, 563)
    assert r["entries"] > 0 and r["sky_entries"] > 0 and r["held"] > 0, r


def test_h8_moving_camera(lib):
    """The 64 cameras of bench.py's moving-camera leg."""
    total = sky = 0
    for k in range(64):
        s = h8()
        s["camera"] = bench_moving_camera(s, k, 64)
        r = check(lib, s, 1280, 720)
        total, sky = total + r["held"], sky + r["sky_entries"]
    assert total > 0 and sky > 0


def test_h8_depth_8(lib):
    r = check(lib, rt_host.load_scene("h8_d8"), 1920, 1080)
    assert r["entries"] > 0 and r["sky_entries"] > 0 and r["held"] > 0, r


def test_two_mirrors_facing_each_other(lib):
    """Each mirror shows the other: its blocks' sets hold two and three spheres, of which only the block's own mirror is left out."""
    s = two_mirrors()
    r = check(lib, s, 1280, 720)
    b = bits(lib, s, 1280, 720)
    print("two mirrors 1280x720:", r, "entries by bits", {int(k): int((b == k).sum()) for k in np.unique(b)})
    assert r["entries"] > 0 and r["held"] > 0, r
    # a mirror block in whose reflection the other mirror (or the floor) shows leaves its own mirror out and walks the rest; one that reflects the sky alone walks nothing
    assert (b == SELF0).any() and (b == SELF0 | SKY).any()


def test_random_scenes(lib):
    """The GPU soaks' generator (tests/soak_gpu_parity.py: draw_scene), at the size drawn and at four times that size."""
    tot = {"entries": 0, "sky_entries": 0, "held": 0}
    for seed in SEEDS:
        scene, w, h = draw_scene(seed, False, False)
        scene["name"] = "seed %d" % seed
        for k in (1, 4):
            r = check(lib, scene, k * w, k * h)
            for key in tot:
                tot[key] += r[key]
    print("random scenes:", tot)
    assert tot["entries"] > 0 and tot["held"] > 0, tot


@pytest.mark.parametrize("scene,wh", [("h8", (3840, 2160)), ("h8", (1001, 563)), ("h8_ss2", (1001, 563)), ("h8_d8", (1280, 720)), ("two_mirrors", (1280, 720)),
                                      ("default14", (1280, 720)), ("lcg64_ss1", (1280, 720))])
def test_only_word_1_of_stating_entries_changes(lib, scene, wh):
    """Without the flag the table is word for word the one built with flags 1|2|4|32|128 (and the flag alone, without the sets, states
    nothing); with it words 0, 2 and 3, bit 31 and the low 24 bits of word 1 are unchanged, and only stating entries carry a bit."""
    s = h8(supersample=2) if scene == "h8_ss2" else (two_mirrors() if scene == "two_mirrors" else rt_host.load_scene(scene))
    if s.get("supersample", 1) > 2:
        s["supersample"] = 1
    blob = rt_host.flatten_scene(s)
    for tiles in (None, (16, 1, 2, (wh[1] // 16) // 2)):
        for base in (FIRST_BOUNCE, PLAIN | 128, FIRST_BOUNCE | 64):
            before, after = table(lib, blob, *wh, base, tiles), table(lib, blob, *wh, base | 256, tiles)
            assert (before[:, [0, 2, 3]] == after[:, [0, 2, 3]]).all()
            assert ((before[:, 1] ^ after[:, 1]) & 0x80ffffff == 0).all()
            changed = before[:, 1] != after[:, 1]
            assert (after[changed, 3] >> 31 == 1).all() and (after[changed, 1] >> 31 == 0).all()
            assert ((before[before[:, 1] >> 31 == 0, 1] >> 24) == 0).all()
            if scene in ("default14", "lcg64_ss1"):
                assert not changed.any()
        for base in (PLAIN, CELLS):                            # the bits ride on the sets: nothing without them
            assert (table(lib, blob, *wh, base, tiles) == table(lib, blob, *wh, base | 256, tiles)).all()


def test_the_dark_bits_ride_on_a_flag_of_their_own(lib):
    """Bit 9 of `ranked` adds bits 27 and 28 to entries that state a set and changes nothing else; without bit 8, or without the shadow
    masks, it adds nothing."""
    for s, wh in ((h8(), (3840, 2160)), (two_mirrors(), (1280, 720)), (h8(supersample=2), (1001, 563))):
        blob = rt_host.flatten_scene(s)
        a, b = table(lib, blob, *wh, SECOND_NODE), table(lib, blob, *wh, DARK)
        assert (a[:, [0, 2, 3]] == b[:, [0, 2, 3]]).all() and ((a[:, 1] ^ b[:, 1]) & ~np.uint32(0x18000000) == 0).all()
        changed = a[:, 1] != b[:, 1]
        assert changed.any() and (b[changed, 3] >> 31 == 1).all()
        assert (table(lib, blob, *wh, FIRST_BOUNCE | 512) == table(lib, blob, *wh, FIRST_BOUNCE)).all()
        assert (table(lib, blob, *wh, (1 | 2 | 128 | 256 | 512)) == table(lib, blob, *wh, (1 | 2 | 128 | 256))).all()


def test_the_statement_under_asan_and_ubsan(tmp_path):
    """tests/host/second_node_check.cpp: every block of a few hand-made frames, ordinary and at the edges of the arithmetic, through
    rt_block_statement with the host compiler's address and undefined-behaviour sanitizers; a stand-alone program."""
    here = os.path.dirname(os.path.abspath(__file__))
    cxx = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("c++") or shutil.which("clang++")
    exe = str(tmp_path / "second_node_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-I" + os.path.join(here, "..", "html5-canvas-raytracer_amd", "csrc"), os.path.join(here, "host", "second_node_check.cpp"), "-o", exe], check=True)
    run = subprocess.run([exe], capture_output=True, text=True)
    print(run.stdout, run.stderr)
    assert run.returncode == 0, run.stderr[-2000:]


def test_nothing_is_stated_with_a_tiny_epsilon(lib):
    """rt_self_clear sets the far root's rounding against epsilon: 1e-12 is below it for every sphere (the sets themselves stay)."""
    s = h8(epsilon=1e-12)
    assert len(stating(table(lib, rt_host.flatten_scene(s), 1920, 1080, SECOND_NODE))) > 0
    assert not bits(lib, s, 1920, 1080).any()
    assert bits(lib, h8(), 1920, 1080).any()


def test_nothing_is_stated_for_a_huge_mirror(lib):
    """The bound grows with the size of the coordinates: a mirror 1000 units across and away drops nothing."""
    s = h8()
    big = copy.deepcopy(next(o for o in s["objects"] if o["mtl"]["albedo"][3] > 0 and o["r2"] == 1))
    big["origin"], big["r2"] = [0.0, 300.0, -1500.0], 250000.0
    s["objects"] = [big] + [o for o in s["objects"] if not (o["mtl"]["albedo"][3] > 0)]
    rows = stating(table(lib, rt_host.flatten_scene(s), 1920, 1080, SECOND_NODE))
    assert len(rows) > 0 and not ((rows[:, 1] >> 24) & 127).any()


def test_nothing_is_stated_at_depth_1(lib):
    assert not bits(lib, h8(segs=1), 1920, 1080).any()
    t = table(lib, rt_host.flatten_scene(h8(segs=1)), 1920, 1080, SECOND_NODE)
    assert ((t[t[:, 1] >> 31 == 0, 1] >> 24) == 0).all()


def test_nothing_is_stated_when_the_only_mirror_also_refracts(lib):
    s = h8()
    for o in s["objects"]:
        if o["mtl"]["albedo"][3] > 0:
            if o["r2"] == 0.25:
                o["mtl"]["albedo"][4] = 0.5
            else:
                o["mtl"]["albedo"][3] = 0.0
    t = table(lib, rt_host.flatten_scene(s), 1920, 1080, SECOND_NODE)
    assert ((t[t[:, 1] >> 31 == 0, 1] >> 24) == 0).all()


def test_nothing_is_stated_when_the_enclosing_sphere_reflects(lib):
    t = table(lib, rt_host.flatten_scene(reflecting_sky()), 1920, 1080, SECOND_NODE)
    assert ((t[t[:, 1] >> 31 == 0, 1] >> 24) == 0).all()


def test_nothing_is_stated_with_14_loop_spheres(lib):
    for extra, expect in ((6, True), (7, False)):              # 13 loop spheres state, 14 do not
        s = h8()
        small = next(o for o in s["objects"] if o["r2"] == 0.25)
        for i in range(extra):
            o = copy.deepcopy(small)
            o["origin"] = [-3.0 + i, 3.5, -3.0]
            s["objects"].insert(0, o)
        t = table(lib, rt_host.flatten_scene(s), 1920, 1080, SECOND_NODE)
        assert ((t[t[:, 1] >> 31 == 0, 1] >> 24) != 0).any() == expect
