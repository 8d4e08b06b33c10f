"""The scalar forms of the few-sphere one-wave trace kernels (docs/EVIDENCE.md, "Scalar forms"): the specular power's walk as a ladder on the
condition code (rt_spec_walk.h, rt_kernel_math.h: rt_pow_spec), a wave's decisions about its entry as bits of one scalar word (rt_kernel.hip:
WAVE_FLAGS), a light's occluder set by one 64-bit shift, and the occluder's transparency tested on its bit pattern (rt_uniform_pred.h).  The
change moves control flow and no arithmetic, so the first yardstick is byte equality with the PARENT commit's product library: the sha256 of
both frames of a fresh upload (four-wave form, then one-wave workgroups), recorded once on the GPU with that library in place of the tree's.
The test library's frames are held to the same bytes, with and without RT_NO_UNIFORM_BLOCKS and with as many samples marked for the exact
launch, and every frame stays within 1 LSB of the C restatement (oracle/rt_oracle.c).

What can go wrong is a ladder that multiplies in another order or once too often - exponents with no bit (0), the lowest bit alone (1), one
ladder step (2, 3), several (10, 50, 500), all nine steps and not one more (1023), none at all behind ten squarings of the trailing-zero loop
(1024), the nine steps and then the loop behind them (1025: its top bit, 2047: its top bit with every step's product), and the generic call
(12.5) -, a wave that takes the path it should have been turned away from or the reverse (a mirror at depth 1 and 3, stars), a sky wave that
traces or a traced wave that stores the sky constant, and a light whose occluder set is read at the wrong shift (a sphere over the floor; a
light behind the surface).  No case passes vacuously: the restatement's per-sample probe (oracle_probe_sample) must show the event a case is
there for at the case's own size, and the test library's counters must show the waves on the uniform-material path - or off it - and the waves
that took their checker cell from the table - or none - as the case says."""
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
import test_gpu_general_path as gp            # events, band_rows
import test_gpu_prologue_loads as pl          # h8, restatement, SWITCH
import test_gpu_scalar_paths as sp            # floor_alone, waves
from objects_util import tlib  # noqa: F401  (fixture: the test library)
from test_first_bounce import two_mirrors
from test_gpu_prologue_loads import plib  # noqa: F401  (fixture: the product library)
from test_gpu_scalar_paths import lib  # noqa: F401  (fixture: the test library with its wave counters)

pytestmark = pytest.mark.gpu

W, H = 64, 16
BAND = (H, 3, 1, 1)                  # tile 3 of four 16-row tiles of a 64 x 64 frame: under h8's camera it shows the floor alone
# needs: events the restatement must show (probe_events, below); path: what the test library's counter must say of the second frame's waves -
# "some" complete the uniform-material path, "none" does (the case is there for the turn-away), None - not looked at; cells: of those waves,
# the ones that took their checker cell from the table - "some", "none", None - not looked at
Case = collections.namedtuple("Case", "make w h tiles needs path cells", defaults=(W, H, BAND, ("floor_only",), "some", None))

CHECKER = {"kind": 2, "colors": [[1, 1, 0], [1, 0, 1]]}


def floor_n(e, highlight=False, a2=0.9):
    """h8's floor alone with specular exponent e.  highlight: the second light at the camera's mirror image in the floor about the band's centre
    hit, so that the band holds the highlight's peak - under h8's own lights the powers of 500 and more are below a byte's resolution
    everywhere in the band and the three largest exponents give one and the same frame (checked with the C restatement: with this light
    the frames of 500, 1023 and 1024 all differ).  a2: the specular albedo - exponent 0 makes every light's power 1, and with 0.9 the sum
    saturates every channel: two flat colours; with 0.2 the diffuse term shows."""
    def make():
        s = sp.floor_alone(specular_exponent=e, albedo=[0, 0.3, a2, 0, 0])
        if highlight:
            s["lights"][1] = [-0.0629547715612, 1.5, 3.02138477293]
        return s
    return make


def light_behind():
    """The second light under the floor's surface (the sphere's top lies at y = -0.1 + ...: h8's floor is centred 500 below): it faces no hit."""
    s = sp.floor_alone(specular_exponent=10, albedo=[0, 0.3, 0.9, 0, 0])
    s["lights"][1] = [5.0, -3.0, 0.0]
    return s


def ball_over_floor():
    """tests/test_gpu_scalar_paths.py's shadow scene: a small sphere on the way from light 0 to the floor the band shows - one-candidate blocks
    whose shadow masks name it."""
    s = sp.floor_alone(specular_exponent=10)
    ball = copy.deepcopy(next(o for o in pl.h8()["objects"] if o["r2"] == 1))
    ball["origin"], ball["r2"] = [3.0, 6.0, 5.4], 0.09
    s["objects"].insert(0, ball)
    return s


def mirror_floor(segs):
    def make():
        s = sp.floor_alone(albedo=[0.1, 0.5, 0.3, 0.4, 0], sampler={"kind": 0}, color=[0.9, 0.6, 0.3])
        s["segs"] = segs
        return s
    return make


CASES = {
    # a floor-only view under two lights: the ladder's entry (no bit, bit 0), its first step, two adjacent bits, the record's exponents, its top
    # step (1023: exactly its nine), a single bit above it (1024: ten squarings, no step), past its range (1025, 2047: the loop behind the ladder;
    # from 500 on with the highlight in the band: floor_n), the generic call
    "floor_n0": Case(floor_n(0, a2=0.2)), "floor_n1": Case(floor_n(1), needs=("floor_only", "specular")), "floor_n2": Case(floor_n(2), needs=("floor_only", "specular")),
    "floor_n3": Case(floor_n(3), needs=("floor_only", "specular")), "floor_n10": Case(floor_n(10), needs=("floor_only", "specular")),
    "floor_n50": Case(floor_n(50), needs=("floor_only", "specular")), "floor_n500": Case(floor_n(500, True), needs=("floor_only", "specular")),
    "floor_n1023": Case(floor_n(1023, True), needs=("floor_only", "specular")), "floor_n1024": Case(floor_n(1024, True), needs=("floor_only", "specular")),
    "floor_n1025": Case(floor_n(1025, True), needs=("floor_only", "specular")), "floor_n2047": Case(floor_n(2047, True), needs=("floor_only", "specular")),
    "floor_n12_5": Case(floor_n(12.5), needs=("floor_only", "specular")),
    "light_behind": Case(light_behind, needs=("floor_only", "light1_behind", "specular")),
    "ball_over_floor": Case(ball_over_floor, needs=("floor_only", "blocked")),
    "mirror_depth1": Case(mirror_floor(1), needs=("floor_only", "no_bounce")),
    "mirror_depth3": Case(mirror_floor(3), needs=("floor_only", "bounce"), path="none"),
    "texture": Case(lambda: sp.floor_alone(sampler={"kind": 1, "texture": 0}, color=[0.9, 0.6, 0.3]), needs=("floor_only", "texels")),
    "checker_cell": Case(lambda: sp.floor_alone(sampler=dict(CHECKER, freqU=6, freqV=3)), needs=("floor_only", "one_colour"), cells="some"),
    "checker_no_cell": Case(lambda: sp.floor_alone(sampler=dict(CHECKER, freqU=100000, freqV=50000)), needs=("floor_only", "both_colours"), cells="none"),
    "stars": Case(lambda: sp.floor_alone(sampler={"kind": 3, "threshold": 0.5, "scale": 1.5}), path="none"),
    # a bouncing block three nodes deep, and a frame with sky runs, spheres and floor at a ragged size
    "two_mirrors_64x16": Case(two_mirrors, 64, 16, None, ("bounce", "deep"), None),
    "h8_128x64": Case(pl.h8, 128, 64, None, ("bounce",), None),
}

# sha256 of the frame by the parent commit's product library - its first frame (the four-wave form) and its second (one-wave workgroups)
# are the same bytes in every case - recorded with it on the GPU, never from the tree under test
PARENT_SHA256 = {
    "ball_over_floor": "8a5bbaf1e9c1e9a6777f6437b18f5e90fcd0366f3022106deb50d36167f12146",
    "checker_cell": "0e9dbd339235acae6218764f823aa0fe511b705757597c38e71e01a2fd1b18d6",
    "checker_no_cell": "891a3cd282e74c615764469dcdfeffd73af58638d6b5ed0f19a6f1fcb46d8437",
    "floor_n0": "4dca5aefcd8fd52cb149aa50248f846330f649b1a23ab97b5a5a9d75a1fb1262",
    "floor_n1": "7add4d801cb276ce16ce423fbba11f6c6b6ff082122cb52f736a57ce9de3d753",
    "floor_n10": "c09e17d6e30b77b4464de117d27d7f3f2825048b34c0198453bb6a42128fbaad",
    "floor_n1025": "c67267346ffcd8f7919bae11acc26fcc366e54a1e59e08fcfcd7a96dc89031e7",
    "floor_n2047": "0aaf1e49644c0bfc0d9609dd74c2679ef732c401b71494ee1b75832e7770818f",
    "floor_n1023": "99169c0bb884e91401eb6955ce3fb939804896927e37e06c77e9cd3fdb09213f",
    "floor_n1024": "c67267346ffcd8f7919bae11acc26fcc366e54a1e59e08fcfcd7a96dc89031e7",
    "floor_n12_5": "480f0d62d7fbec7fcfbbeb843e022709ff007039eb0326d9dcec81df45bbddfc",
    "floor_n2": "1cee64137d92cee74e671ef43ddd68bae5e17f992b6205577ebe305912752af2",
    "floor_n3": "1de1e7c47bbf4b531b0c0b251e2e05d2f7581ebf6989edea7389144d56b1826b",
    "floor_n50": "ae9514260f37daf476b4158a17ae1717cdf2536d493752ef76b100cf280b48ee",
    "floor_n500": "519cd00af160917d6c0c2c223d238b05fd1260136c7db39ac4df29ee1a1a9fbb",
    "h8_128x64": "03c7fb97cd51ab683333add66920dfe9cb635a27a50d72b2d2d88ec02e907bbc",
    "light_behind": "7bd7c733d1d56c8e64b2aecbd9a579671e6998cbe8882eed35d31adf1487243d",
    "mirror_depth1": "f032a157b2c471d46e2430c0b348f52defdfe2846b2be12c1c15c35150c451b8",
    "mirror_depth3": "fa8469a7fc9afbf77fd5ad4659525fe60847f3924f95eedac75256a56f839eaf",
    "stars": "a4df70626147b41d2f7c765a5e57983aff911000430a40c210d319f5c6690a47",
    "texture": "f996fb8c56c64df4d37e8355d31b86b74b71de4c45031ec00cb22cc1055a5228",
    "two_mirrors_64x16": "3e92b90625fd5a2c67f27d03738fcfd6f71f1126b37f37fd0c4a8e0f0e77e7ff",
}


def probe_events(scene, w, h, tiles):
    """What the restatement's probe shows in the band's samples: gp.events' counts, and floor_only - EVERY sample's primary hit is the scene's
    floor from outside; specular - samples with a specular term > 0 (the power is evaluated); blocked - lit primary hits whose light intensity
    ended at 0; light1_behind - light 1 faces NO primary hit (l . n <= 0 at every one); no_bounce - no sample has a node below the primary;
    texels / one_colour / both_colours - the primary hits' sampled colours are more than 8 / exactly one (the band inside ONE checker cell) /
    exactly two (cells finer than a block)."""
    ev = gp.events(scene, w, h, tiles)
    lib = hu.oracle_lib()
    blob = rt_host.flatten_scene(scene)
    buf = C.create_string_buffer(blob, len(blob))
    rec = np.zeros((hu.PROBE_NODES, hu.PROBE_WORDS), np.float64)
    floor_i = next((i for i, o in enumerate(scene["objects"]) if o["r2"] == pl.FLOOR_R2), -1)
    n = on_floor = spec = blocked = facing1 = 0
    colours = set()
    for y in gp.band_rows(h, tiles):
        for sx in range(w):
            assert lib.oracle_probe_sample(buf, len(blob), w, h, sx, y, rec.ctypes.data) == 0
            q = next(q for q in rec if q[23] == 1 and int(q[0]) == 1)
            n += 1
            on_floor += int(q[1]) == 2 * floor_i
            spec += q[16] > 0
            colours.add(tuple(q[12:15]))
            blocked += q[1] >= 0 and q[18] == 0
            if len(scene["lights"]) > 1:
                facing1 += float(np.dot(np.array(scene["lights"][1]) - q[3:6], q[6:9])) > 0
    ev.update(floor_only=int(on_floor == n), specular=spec, blocked=blocked, light1_behind=int(facing1 == 0), no_bounce=int(ev["bounce"] == 0),
              texels=int(len(colours) > 8), one_colour=int(len(colours) == 1), both_colours=int(len(colours) == 2))
    return ev


def two_frames(lib, name, general=False, count=False):  # noqa: F811
    """[(frame, exact_samples)] x 2 of a fresh upload: the four-wave form, then one-wave workgroups; general: with RT_NO_UNIFORM_BLOCKS (the test
    library reads it); count: also (the waves of the second frame that completed the uniform-material path, those of them that took their checker cell from the
    table) (test library)."""
    c = CASES[name]
    t = rt_host.RtTiles(*(c.tiles or (c.h, 0, 1, 1)))
    h = c.h if c.tiles is None else 4 * c.h
    n = t.n_tiles * t.tile_rows * c.w * 4
    if general:
        os.environ[pl.SWITCH] = "1"
    try:
        r = rt_host.Renderer(rt_host.flatten_scene(c.make()), 0, lib)
        try:
            out, took = [], None
            for _ in range(2):
                d = lib.rt_alloc_device(0, n)
                assert d, lib.rt_last_error()
                try:
                    if count:
                        sp.waves(lib, lib.rt_test_uniform_waves), sp.waves(lib, lib.rt_test_cell_waves)
                    st = r.render_tiles(c.w, h, d, t, want_stats=True)
                    if count:
                        took = (sp.waves(lib, lib.rt_test_uniform_waves), sp.waves(lib, lib.rt_test_cell_waves))
                    host = C.create_string_buffer(n)
                    assert lib.rt_copy_to_host(0, host, d, n) == 0, lib.rt_last_error()
                    out.append((host.raw, int(st.exact_samples)))
                finally:
                    lib.rt_free_device(0, d)
            return (out, took) if count else out
        finally:
            r.close()
    finally:
        if general:
            os.environ.pop(pl.SWITCH, None)


@pytest.mark.parametrize("name", sorted(CASES))
def test_frames_are_the_parents(lib, plib, name):  # noqa: F811
    c = CASES[name]
    h = c.h if c.tiles is None else 4 * c.h
    tiles = c.tiles or (c.h, 0, 1, 1)
    ev = probe_events(c.make(), c.w, h, tiles)
    print(name, "events by the restatement:", ev)
    assert all(ev[k] > 0 for k in c.needs), (c.needs, ev)
    product = two_frames(plib, name)
    sha = [hashlib.sha256(f).hexdigest() for f, _ in product]
    print(name, "sha256", sha)
    assert len(set(product[1][0][i:i + 4] for i in range(0, len(product[1][0]) - 3, 4))) > 8, "a flat frame: the case does not test what it is meant to"
    assert sha == [PARENT_SHA256[name]] * 2
    test, (took, cells) = two_frames(lib, name, count=True)
    general, (none, _) = two_frames(lib, name, general=True, count=True)
    print(name, "uniform-material waves %d of %d, %d with a stated cell" % (took, len(gp.band_rows(h, tiles)) // 8 * (c.w // 8), cells))
    if c.cells == "some":
        assert cells > 0
    elif c.cells == "none":
        assert cells == 0, cells
    assert none == 0, none                                       # the switch really kept every wave off the path
    if c.path == "none":
        assert took == 0, took
    elif c.path == "some":
        assert took > 0
    assert test == product, "the test library's frames or marked samples differ from the product library's"
    assert general == product, "the general path's frames or marked samples differ (RT_NO_UNIFORM_BLOCKS)"
    ora = pl.restatement(c.make(), c.w, h, tiles)
    lsb, frac = ou.max_lsb(product[1][0], ora)
    print(name, "|gpu - restatement| <= %d LSB in %.2e of the channels" % (lsb, frac))
    assert lsb <= 1, (lsb, frac)
