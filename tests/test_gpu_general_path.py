"""The general path of the few-sphere reflection-only product kernels (rt_kernel_trace.h: WAVE_NODE, RT_CHAIN_END): the node a wave is at
is a count of the node loop's turns in a scalar register - and with it the shadow scan's pair mask, the fold's "map so far" and the
first-bounce walk's condition are scalar values -, and a lane whose chain ends folds its colour in the branch that ended it.  The change moves
bookkeeping and no arithmetic, so the first yardstick is byte equality with the PARENT commit's product library: the sha256 of both frames of
a fresh upload (four-wave form, then one-wave workgroups), recorded once on the GPU with that library in place of the tree's
(docs/EVIDENCE.md, "Diet for the general path").  The test library's frames are held to the same bytes, with and without
RT_NO_UNIFORM_BLOCKS and with as many samples marked for the exact launch, and the frame stays within 1 LSB of the C restatement
(oracle/rt_oracle.c) - except the two cases with an infinite material constant, which are held to the parent's bytes alone
(tests/test_gpu_vector_paths.py says why: the product fold swallows a NaN child).

What can go wrong is a wave whose lanes are NOT at the same node after all, a pair of the scan skipped at a node whose mask does not
speak of it, a map applied at the primary or not applied below it, and a colour that a lane which left the loop early loses while the
wave's other lanes go on.  No case passes vacuously: the restatement's per-sample probe (oracle_probe_sample) must show the events a
case is there for, at the case's own size - bouncing samples, a node below the primary whose light is blocked, chains that end at a
childless primary hit, behind a fold, and on the miss colour - and the cameras and lights below were moved on the CPU until it did.
(The spheres that h8_12_spheres and h8_13_spheres add lie outside the 64 x 16 frame and shadow nothing in it: they lengthen every scan.)"""
import collections
import copy
import ctypes as C
import hashlib
import os

import numpy as np
import pytest

import hits_util as hu
import oracle_util as ou
import rt_host
import test_gpu_prologue_loads as pl          # h8, with_loop_spheres, restatement, SWITCH
import test_gpu_vector_paths as vp            # h8_mirror, inside_mirror
from objects_util import tlib  # noqa: F401  (fixture: the test library)
from test_first_bounce import two_mirrors
from test_gpu_prologue_loads import plib  # noqa: F401  (fixture: the product library)

pytestmark = pytest.mark.gpu

INF = float("inf")
# needs: the events the restatement must show for the case (events(), below)
Case = collections.namedtuple("Case", "make w h tiles moved needs exact", defaults=(None, False, ("bounce", "end_leaf", "end_fold"), True))


def _h8(**kw):
    s = pl.h8()
    s.update(kw)
    return s


def no_sky():
    """h8 without its enclosing sphere: a ray that meets nothing takes the miss colour - at the primary and behind a mirror's fold."""
    s = pl.h8()
    s["objects"] = [o for o in s["objects"] if o["r2"] != 25000000]
    return s


def light_behind_an_occluder():
    """h8 with its first light moved low behind the row of spheres: the floor a mirror shows lies in the spheres' shadows, so the scan at the
    node below the primary has blocked lanes (the light was lowered on the CPU until the restatement's probe showed them at 64 x 16)."""
    s = pl.h8()
    s["lights"][0] = [0.0, 1.5, -8.0]
    return s


CASES = {
    # h8 at depth 3: mirror hits, mirror to mirror, a mirror's reflection of the shadowed floor; blocks with one, two and no named candidate
    "h8_96x24": Case(pl.h8, 96, 24, needs=("bounce", "blocked_below", "end_leaf", "end_fold")),
    "h8_33x9": Case(pl.h8, 33, 9),                                                   # odd both ways: partly valid blocks
    "h8_32x8": Case(pl.h8, 32, 8),                                                   # one block: four waves
    "h8_d1_64x16": Case(lambda: _h8(segs=1), 64, 16, needs=("end_leaf",)),           # no wave descends: every chain ends at the primary
    "h8_d8_64x16": Case(lambda: rt_host.load_scene("h8_d8"), 64, 16, needs=("bounce", "deep", "end_leaf", "end_fold")),
    "h8_ss2_48x16": Case(lambda: _h8(supersample=2), 48, 16),                        # rt_trace<0,0,1,0,1>
    "h8_rank0_64x32": Case(pl.h8, 64, 32, tiles=(8, 0, 2, 2)),                       # the interleaved tiles of two ranks
    "h8_rank1_64x32": Case(pl.h8, 64, 32, tiles=(8, 1, 2, 2)),
    "h8_moved_camera": Case(pl.h8, 64, 16, moved=True),                              # the first frame after set_camera: the four-wave form
    "two_mirrors_64x16": Case(two_mirrors, 64, 16, needs=("bounce", "deep", "end_fold")),   # two mirrors facing each other
    "inside_mirror_32x8": Case(vp.inside_mirror, 32, 8, needs=("bounce", "deep", "inside", "end_fold")),   # the camera inside a mirror sphere
    "h8_13_spheres": Case(lambda: pl.with_loop_spheres(12), 64, 16),                 # the largest few-sphere scene: the pair loop's later masks
    "h8_12_spheres": Case(lambda: pl.with_loop_spheres(11), 64, 16),                 # ... and an odd count of loop spheres: the scan's single tail
    "light_behind_64x16": Case(light_behind_an_occluder, 64, 16, needs=("bounce", "blocked_below", "end_fold")),
    "no_sky_64x16": Case(no_sky, 64, 16, needs=("bounce", "end_miss", "miss_below", "end_leaf", "end_fold")),
    # NaN and infinity through the chain end and the fold: the parent's bytes only
    "colour_inf_64x16": Case(lambda: vp.h8_mirror(color=[INF, 0.5, 0.5], sampler={"kind": 0}), 64, 16, needs=("bounce", "end_fold"), exact=False),
    "a2_inf_64x16": Case(lambda: vp.h8_mirror(a2=INF), 64, 16, needs=("bounce", "end_fold"), exact=False),
}

# sha256 of the frame by the parent commit's product library - its first frame (the four-wave form) and its second (one-wave workgroups)
# are the same bytes in every case - recorded with it on the GPU, never from the tree under test
PARENT_SHA256 = {
    "a2_inf_64x16": "da42b3f09fc01fc0b3cd3b40b1f7c4b6a49a373bee50d3caf6508ce9d7c946ad",
    "colour_inf_64x16": "fab2324851c60b6be11c6448f319cf036b6231d84d2fc4abdc2cb78bb205e06a",
    "h8_12_spheres": "a772789f4d86ab6bdc58a1b06315f04482903edd9a8a524ec76bafd8f9f90a49",
    "h8_13_spheres": "a772789f4d86ab6bdc58a1b06315f04482903edd9a8a524ec76bafd8f9f90a49",
    "h8_32x8": "5b0efafe364422b3d14d5ef4518591ce2bb330919ba3b2bafe28fe32fedd92c0",
    "h8_33x9": "1f405c2d667504d4468b50f885372d6f8ec045ab67fda3c4f033c5e0194c2915",
    "h8_96x24": "388768b7e32acc4b0d659b9d08335b577e265d851e5fdac59fa9cb0de24591f3",
    "h8_d1_64x16": "6a567095e646723128175fae7d4f1a8b02223c4af1a679fa3e7025f7bba18640",
    "h8_d8_64x16": "cbcc1ba9cb16720e4b6ef03610f69157050083b303e367cf5539411364697b41",
    "h8_moved_camera": "a28e8179fc603c379ff7cb1bb55d87636a0842465aac15f082aeed4655d13fa6",
    "h8_rank0_64x32": "7323b1708a90a9770854e57c070502dcc48d354097096c4c69a69c003d8d0ed0",
    "h8_rank1_64x32": "6c5467b8a60856f04d008f7f85977044c01b42366701fb1872508305f7dab34a",
    "h8_ss2_48x16": "0dbc83c5ce3020de243693d59ce52b101b7e2ddf5038b0f7dd5b2ee309313b0e",
    "inside_mirror_32x8": "68d3fb1462d742e6e5da98dc0594440355d7ff011601de6b742ab8e78a727175",
    "light_behind_64x16": "efc72abae434be7468843e27f59763ef653c53b12141ae8e9c71390b5dea39a0",
    "no_sky_64x16": "7444061929de20b48cc7f05a5daa3390cd71631bd2a65c18946694cf5c1a0f6a",
    "two_mirrors_64x16": "3e92b90625fd5a2c67f27d03738fcfd6f71f1126b37f37fd0c4a8e0f0e77e7ff",
}


def camera_of(name):
    c = CASES[name]
    if not c.moved:
        return None
    import bench
    return bench.moving_camera(c.make(), 3, 16)


def shown(name):
    """The scene as the frames show it (the moved camera in place)."""
    s = copy.deepcopy(CASES[name].make())
    cam = camera_of(name)
    if cam is not None:
        s["camera"] = cam
    return s


def band_rows(h, tiles):
    tile_rows, first, stride, n_tiles = tiles or (h, 0, 1, 1)
    return [y for k in range(n_tiles) for y in range((first + k * stride) * tile_rows, min(h, (first + k * stride + 1) * tile_rows))]


def events(scene, w, h, tiles=None):
    """What the restatement's probe shows in the band's samples: how many samples bounce (a node below the primary), go deeper than the second
    node, end at a childless primary hit / behind a fold / on the miss colour (at the primary, below it), have a lit node below the primary
    whose light intensity ended at 0 (a blocked shadow ray), hit a sphere from the inside."""
    lib = hu.oracle_lib()
    blob = rt_host.flatten_scene(scene)
    buf = C.create_string_buffer(blob, len(blob))
    ss = max(1, scene.get("supersample", 1))
    rec = np.zeros((hu.PROBE_NODES, hu.PROBE_WORDS), np.float64)
    lit = [o["mtl"]["albedo"][1] > 0 or o["mtl"]["albedo"][2] > 0 for o in scene["objects"]]
    ev = collections.Counter(bounce=0, deep=0, end_leaf=0, end_fold=0, end_miss=0, miss_below=0, blocked_below=0, inside=0)
    for y in band_rows(h, tiles):
        for sy in range(y * ss, (y + 1) * ss):
            for sx in range(w * ss):
                assert lib.oracle_probe_sample(buf, len(blob), w, h, sx, sy, rec.ctypes.data) == 0
                nodes = {int(q[0]): q for q in rec if q[23] == 1}
                last = nodes[max(nodes)]                               # reflection-only: a chain, path 1, 2, 4, ...
                ev["bounce"] += 2 in nodes
                ev["deep"] += 4 in nodes
                ev["end_miss"] += len(nodes) == 1 and last[1] < 0
                ev["miss_below"] += len(nodes) > 1 and last[1] < 0
                ev["end_leaf"] += len(nodes) == 1 and last[1] >= 0
                ev["end_fold"] += len(nodes) > 1 and last[1] >= 0
                ev["blocked_below"] += any(p > 1 and q[1] >= 0 and lit[int(q[1]) >> 1] and q[18] == 0 for p, q in nodes.items())
                ev["inside"] += any(q[1] >= 0 and (int(q[1]) & 1) and scene["objects"][int(q[1]) >> 1]["r2"] < 1000 for q in nodes.values())
    return dict(ev)


def two_frames(lib, name, general=False):
    """[(frame, exact_samples)] x 2 of a fresh upload (after one set_camera if the case moves the camera): the four-wave form, then one-wave
    workgroups.  general: with RT_NO_UNIFORM_BLOCKS (the test library reads it)."""
    c = CASES[name]
    t = rt_host.RtTiles(*(c.tiles or (c.h, 0, 1, 1)))
    n = t.n_tiles * t.tile_rows * c.w * 4
    if general:
        os.environ[pl.SWITCH] = "1"
    try:
        r = rt_host.Renderer(rt_host.flatten_scene(c.make()), 0, lib)
        try:
            cam = camera_of(name)
            if cam is not None:
                r.set_camera(cam)
            out = []
            for _ in range(2):
                d = lib.rt_alloc_device(0, n)
                assert d, lib.rt_last_error()
                try:
                    st = r.render_tiles(c.w, c.h, d, t, want_stats=True)
                    host = C.create_string_buffer(n)
                    assert lib.rt_copy_to_host(0, host, d, n) == 0, lib.rt_last_error()
                    out.append((host.raw, int(st.exact_samples)))
                finally:
                    lib.rt_free_device(0, d)
            return out
        finally:
            r.close()
    finally:
        if general:
            os.environ.pop(pl.SWITCH, None)


@pytest.mark.parametrize("name", sorted(CASES))
def test_frames_are_the_parents(tlib, plib, name):  # noqa: F811
    c = CASES[name]
    ev = events(shown(name), c.w, c.h, c.tiles)
    print(name, "events by the restatement:", ev)
    assert all(ev[k] > 0 for k in c.needs), (c.needs, ev)
    product = two_frames(plib, name)
    sha = [hashlib.sha256(f).hexdigest() for f, _ in product]
    print(name, "sha256", sha)
    assert len(set(product[1][0][i:i + 4] for i in range(0, len(product[1][0]) - 3, 4))) > 8, "a flat frame: the case does not test what it is meant to"
    assert sha == [PARENT_SHA256[name]] * 2
    test, general = two_frames(tlib, name), two_frames(tlib, name, general=True)
    assert test == product, "the test library's frames or marked samples differ from the product library's"
    assert general == product, "the general path's frames or marked samples differ (RT_NO_UNIFORM_BLOCKS)"
    if c.exact:
        ora = pl.restatement(shown(name), c.w, c.h, c.tiles or (c.h, 0, 1, 1))
        lsb, frac = ou.max_lsb(product[1][0], ora)
        print(name, "|gpu - restatement| <= %d LSB in %.2e of the channels" % (lsb, frac))
        assert lsb <= 1, (lsb, frac)
