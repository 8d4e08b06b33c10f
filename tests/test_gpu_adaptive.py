"""Adaptive supersampling on the GPU (include/rt_hip.h: rt_render_adaptive_device, rt_render_adaptive).  The yardsticks are existing
paths only: `base` is render_tiles of the supersample-1 scene, `fine` render_tiles(..., RT_FLAG_STRICT_FP) of the same scene with
supersample = k on a Renderer of its own, `mask` rt_host.adaptive_mask(base) in numpy and `want` adaptive_compose(base, fine, mask);
frame, mask and count each equal their yardstick byte for byte.  Every case first asserts that the base frame rendered before and
after the adaptive call on the same Renderer is the same bytes, so that a mismatch is not blamed on the new code; and every case with
0 < T < 256 on a frame of at least 60 x 45 refines between 1 % and 60 % of its pixels, so that none is vacuous."""
import base64
import ctypes as C
import functools
import json
import os
import subprocess

import numpy as np
import pytest

import nodes_util as nu
import oracle_util as ou
import rt_host
from lights_util import move_lights
from objects_util import FAST, STRICT, Frames, fresh, tlib  # noqa: F401
from texels_util import with_texels
from texture_util import texels

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID = -1


@pytest.fixture(scope="module")
def lib(tlib):
    return tlib


def drain():
    assert nu.hip().hipDeviceSynchronize() == 0


def adaptive(lib, r, w, h, k, t, flags=0, want_mask=True, stats=False):
    """One rt_render_adaptive_device call into canary-framed device buffers: (frame bytes, mask (h, w) or None, refined count)."""
    wb = rt_host.adaptive_work_bytes(w, h, lib)
    assert wb == 16 + 4 * w * h
    out, work = nu.Dev(lib, w * h * 4), nu.Dev(lib, wb)
    mask = nu.Dev(lib, w * h) if want_mask else None
    try:
        st = r.render_adaptive(w, h, out.ptr, k, t, work.ptr, wb, mask.ptr if mask else 0, flags=flags, want_stats=stats)
        drain()
        frame, words = out.read().tobytes(), work.read(np.uint32)
        m = mask.read().reshape(h, w) if mask else None
        count = int(words[0])
        assert count <= w * h
        listed = words[4:4 + count]                               # every refined pixel once, in whatever order
        assert len(set(listed.tolist())) == count and ((listed & 0xffff) < w).all() and ((listed >> 16) < h).all()
        if m is not None:
            seen = np.zeros((h, w), np.uint8)
            seen[listed >> 16, listed & 0xffff] = 1
            assert (seen == m).all()
        if stats:
            assert st.pixels == w * h and st.kernel_ms > 0
        return frame, m, count
    finally:
        for d in (out, work, mask):
            if d:
                d.close()


@functools.lru_cache(maxsize=None)
def scene_of(name):
    return rt_host.load_scene(name)


def refine_grid(lib, w, h, k):
    """The workgroups of the refine launch for a w x h frame (csrc/rt_adaptive.h: rt_adaptive_refine_grid, exported by the test build)."""
    lib.rt_test_adaptive_refine_grid.restype = C.c_uint32
    lib.rt_test_adaptive_refine_grid.argtypes = [C.c_uint32, C.c_uint32, C.c_uint32]
    return int(lib.rt_test_adaptive_refine_grid(w, h, k))


def one_turn(lib, w, h, k):
    """The listed pixels one turn of the refine kernel's grid-stride loop covers: workgroups x 4 waves x 64 // k^2 pixels."""
    return refine_grid(lib, w, h, k) * 4 * (64 // (k * k))


def check(lib, scene, w, h, k, t, flags=FAST, r=None, tag=None, fine=None):
    """The adaptive frame of `scene` (on `r`, a Renderer that holds it - or is said to, after edits - else a fresh one) against its
    yardsticks; returns (frame, base, fine, mask)."""
    own = r is None
    r = r or rt_host.Renderer(rt_host.flatten_scene(scene), 0, lib)
    try:
        fr = Frames(lib, w, h, (h, 0, 1, 1))
        fr.render(r, flags)
        got, mask, count = adaptive(lib, r, w, h, k, t, flags)
        fr.render(r, flags)
        drain()
        before, after = fr.read()
    finally:
        if own:
            r.close()
    assert before == after, tag                                    # the precondition: the base path itself is stable here
    assert before == fresh(lib, scene, w, h, flags=flags), tag     # ... and is the frame of a fresh upload of this scene
    fine = fine or fresh(lib, dict(scene, supersample=k), w, h, flags=STRICT)
    m = rt_host.adaptive_mask(before, w, h, t)
    want = rt_host.adaptive_compose(before, fine, m).tobytes()
    share = float(m.mean())
    print("ADAPTIVE %s %dx%d k=%d T=%d: refined %d of %d pixels (%.1f %%)" % (tag, w, h, k, t, count, w * h, 100 * share))
    assert count == int(m.sum()), tag
    assert (mask == m).all(), (tag, np.argwhere(mask != m)[:8])
    if got != want:
        d = (np.frombuffer(got, np.uint8).reshape(h, w, 4) != np.frombuffer(want, np.uint8).reshape(h, w, 4)).any(axis=2)
        raise AssertionError((tag, "pixels that differ", int(d.sum()), "of them refined", int((d & (m != 0)).sum()), np.argwhere(d)[:8].tolist()))
    if 0 < t < 256 and w >= 60 and h >= 45:
        assert 0.01 <= share <= 0.60, (tag, share)
    return got, before, fine, m


# ------------------------------------------------------------------ ordinary frames
ORDINARY = [("h8", 131, 60, 4), ("default14", 67, 45, 3), ("lcg64_ss1", 96, 64, 2), ("lcg64_ss1", 96, 64, 3), ("lcg64_ss1", 96, 64, 4), ("cfg2", 240, 135, 2)]


@pytest.mark.parametrize("name,w,h,k", ORDINARY, ids=["%s_%dx%d_k%d" % c for c in ORDINARY])
def test_ordinary_frames(lib, name, w, h, k):
    check(lib, scene_of(name), w, h, k, 32, tag=name)


# ------------------------------------------------------------------ T = 0: the supersampled strict frame, and the reference's own
GOLDENS = [("h8", "h8_ss4_131x60", 4), ("default14", "default14_ss3_67x45", 3), ("lcg64_ss1", "lcg64_ss2_128x128", 2), ("lcg64_ss1", "lcg64_ss3_96x64", 3),
           ("lcg64_ss1", "lcg64_ss4_96x64", 4)]


@pytest.mark.parametrize("name,golden,k", GOLDENS, ids=[g[1] for g in GOLDENS])
def test_threshold_0_is_the_supersampled_frame(lib, name, golden, k):
    entry = next(f for f in ou.manifest()["frames"] if f["name"] == golden)
    w, h = entry["w"], entry["h"]
    got, _, fine, m = check(lib, scene_of(name), w, h, k, 0, tag=golden)
    assert m.all() and got == fine
    worst, frac = ou.max_lsb(got, ou.golden_frame(entry))          # the tolerance tests/test_gpu_parity.py holds these frames to
    assert worst <= 1 and frac < 0.01, (golden, worst, frac)


def test_threshold_256_is_the_base_frame(lib):
    got, base, _, m = check(lib, scene_of("h8"), 131, 60, 4, 256, tag="h8 T=256")
    assert not m.any() and got == base


# ------------------------------------------------------------------ lists longer than one turn of the refine kernel's loop
# The refine grid is capped (csrc/rt_adaptive.h), so a list longer than grid x 4 waves x 64 // k^2 pixels is finished by the loop's
# further turns.  (k, w, h): the smallest frames whose w h pixels exceed one turn of the capped grid by a count that is no multiple
# of 64 // k^2, so that the second turn ends in a partly filled wave - 3 pixels past the stride for k = 4, 384 = 54 x 7 + 6 for k = 3,
# 511 = 31 x 16 + 15 for k = 2.  tests/test_adaptive.py holds both properties against the library's own grid, without a GPU.
BEYOND_ONE_TURN = [(4, 749, 175), (3, 640, 359), (2, 1023, 513)]
# (scene, w, h, k, T): 0 < T < 256, a list with holes that is still longer than one turn
HOLES = ("h8", 1920, 1080, 4, 4)
# (w, h, k): the largest extents the call admits - k w or k h = 65536 in the launch record, py up to 32767 in a list entry
LARGEST_EXTENTS = [(16384, 2, 4), (2, 16384, 4), (32768, 1, 2), (1, 32768, 2)]


@pytest.mark.parametrize("name", ["h8", "default14"])
@pytest.mark.parametrize("k,w,h", BEYOND_ONE_TURN, ids=["k%d_%dx%d" % c for c in BEYOND_ONE_TURN])
def test_threshold_0_beyond_one_turn_of_the_refine_loop(lib, name, k, w, h):
    """Every pixel is listed and the list outruns one turn: the frame is the strict supersample-k frame, whose kernel has no such loop.
    h8 runs the <false, k> kernels, default14 (depth 8, refraction) the <true, k> ones."""
    assert w * h > one_turn(lib, w, h, k)
    got, _, fine, m = check(lib, scene_of(name), w, h, k, 0, tag=name)
    assert m.all() and got == fine


def noise_scene(refract):
    """A frame in which no pixel is flat: the camera of h8 inside one sphere that shines with the stars sampler's hash of the sample
    index, every sample a grey drawn uniformly from [0, 1) (threshold 1, scale 1).  A base pixel is one draw of the w x h grid, a
    refined one the box of k k draws of the k w x k h grid: the two bytes agree by chance alone, for about 1 pixel in 256, so a listed
    pixel that is not refined, or refined into another pixel's place, shows whichever pixel it is.  refract: a glass bead behind the
    camera, which no ray meets, makes the scene one of the <true, k> kernels'."""
    s = dict(scene_of("h8"))
    sky = next(o for o in s["objects"] if o["r2"] > 1e6)
    s["objects"] = [dict(sky, mtl=dict(sky["mtl"], sampler={"kind": rt_host.SAMPLER_STARS, "threshold": 1.0, "scale": 1.0}))]
    if refract:
        bead = {"origin": [0.0, 1.5, 40.0], "r2": 0.01, "mtl": {"color": [1, 1, 1], "albedo": [0, 0, 0.5, 0.1, 0.8], "specular_exponent": 125,
                                                                   "refract_index": 1.5, "sampler": {"kind": rt_host.SAMPLER_COLOR}}}
        s["objects"] = [bead] + s["objects"]
    return s


@pytest.mark.parametrize("refract", [False, True], ids=["opaque", "refracting"])
@pytest.mark.parametrize("k,w,h", BEYOND_ONE_TURN, ids=["k%d_%dx%d" % c for c in BEYOND_ONE_TURN])
def test_every_entry_beyond_one_turn_is_refined_into_its_own_pixel(lib, refract, k, w, h):
    """The frames above at T = 0 on noise_scene: in h8 and default14 most pixels are flat - the supersampled pixel is the base pixel - and
    which entries the list's second turn holds is up to the atomics of rt_adaptive_mark, so a loop that skips a few entries can go
    unseen there.  Here at least 99 % of the pixels differ between the base and the strict supersample-k frame (expected: 255 in 256)."""
    assert w * h > one_turn(lib, w, h, k)
    got, base, fine, m = check(lib, noise_scene(refract), w, h, k, 0, tag="noise, %s" % ("refracting" if refract else "opaque"))
    assert m.all() and got == fine
    differ = (np.frombuffer(base, np.uint8).reshape(h, w, 4) != np.frombuffer(fine, np.uint8).reshape(h, w, 4)).any(axis=2)
    assert differ.mean() >= 0.99, differ.mean()


def test_a_list_with_holes_beyond_one_turn_of_the_refine_loop(lib):
    """0 < T < 256: the list names some pixels only, and still more than one turn of the k = 4 loop covers.  Both inequalities are
    conditions on the input, read back from the call.  Observed on an MI355X: 178 717 of 2 073 600 pixels
    refined (8.6 %), against 131 072 in one turn."""
    name, w, h, k, t = HOLES
    _, _, _, m = check(lib, scene_of(name), w, h, k, t, tag=name)
    count = int(m.sum())                                           # (check() held the call's own count and mask to it)
    assert one_turn(lib, w, h, k) < count < w * h, (count, one_turn(lib, w, h, k))


@pytest.mark.parametrize("w,h,k", LARGEST_EXTENTS, ids=["%dx%d_k%d" % c for c in LARGEST_EXTENTS])
def test_largest_extents(lib, w, h, k):
    assert 65536 in (k * w, k * h)
    check(lib, scene_of("h8"), w, h, k, 16, tag="h8")


def test_largest_extents_threshold_0(lib):
    w, h, k = LARGEST_EXTENTS[1]                                   # the tall one: py up to 16383 in every list entry's upper half
    got, _, fine, m = check(lib, scene_of("h8"), w, h, k, 0, tag="h8")
    assert m.all() and got == fine


# ------------------------------------------------------------------ sizes that cross the row ends, the 64-lane pieces and the 7-pixel waves
@pytest.mark.parametrize("w,h", [(1, 1), (1, 70), (70, 1), (63, 9), (65, 9), (257, 3)])
def test_awkward_sizes(lib, w, h):
    check(lib, scene_of("h8"), w, h, 3, 16, tag="h8 %dx%d" % (w, h))


def test_without_a_mask_and_with_stats(lib):
    s, (w, h, k) = scene_of("h8"), (131, 60, 2)
    r = rt_host.Renderer(rt_host.flatten_scene(s), 0, lib)
    try:
        a = adaptive(lib, r, w, h, k, 32)
        b = adaptive(lib, r, w, h, k, 32, want_mask=False, stats=True)
    finally:
        r.close()
    assert a[0] == b[0] and a[2] == b[2] and b[1] is None


# ------------------------------------------------------------------ stars: the refined pixels draw the k-grid's sky
def test_stars_come_from_the_supersampled_grid(lib):
    s, (w, h, k) = scene_of("default14_stars"), (160, 90, 2)
    s7 = dict(s, starsSeed=7)
    r = rt_host.Renderer(rt_host.flatten_scene(s), 0, lib)
    try:
        r.set_stars_seed(7)
        got, base, fine, m = check(lib, s7, w, h, k, 32, r=r, tag="default14_stars seed 7")
    finally:
        r.close()
    assert fresh(lib, s7, w, h) != fresh(lib, s, w, h)             # (the seed shows in this frame at all)
    sky = m.astype(bool) & (np.frombuffer(base, np.uint8).reshape(h, w, 4) != np.frombuffer(fine, np.uint8).reshape(h, w, 4)).any(axis=2)
    assert sky.any()


# ------------------------------------------------------------------ edits of the resident scene
def test_after_camera_object_and_light_edits(lib):
    s, (w, h, k) = scene_of("h8"), (131, 60, 4)
    r = rt_host.Renderer(rt_host.flatten_scene(s), 0, lib)
    try:
        adaptive(lib, r, w, h, k, 32)                              # (a frame with the first camera: tables and mark counts exist)
        e = move_lights(s, 3)
        e["camera"] = dict(s["camera"], origin=[0.4, 1.7, 9.5])
        e["objects"][3] = dict(e["objects"][3], origin=[-1.2, 1.3, 0.5])
        r.set_camera(e["camera"])
        r.set_objects(e["objects"][3:4], 3)
        r.set_lights(e["lights"])
        check(lib, e, w, h, k, 32, r=r, tag="h8 edited")
    finally:
        r.close()


def test_right_after_set_texels(lib):
    s, (w, h, k) = scene_of("cfg2"), (240, 135, 2)
    t0 = s["textures"][0]
    e = with_texels(s, 0, texels(t0["width"], t0["height"], 9))
    r = rt_host.Renderer(rt_host.flatten_scene(s), 0, lib)
    try:
        old = adaptive(lib, r, w, h, k, 32)[0]
        r.set_texels(0, e["textures"][0]["texels"])
        got = check(lib, e, w, h, k, 32, r=r, tag="cfg2 new texels")[0]
    finally:
        r.close()
    assert got != old


def test_strict_base(lib):
    check(lib, scene_of("h8"), 131, 60, 2, 32, flags=STRICT, tag="h8 strict base")


# ------------------------------------------------------------------ the host forms
def test_host_form_equals_the_device_form_and_takes_camera_edits(lib):
    s, (w, h, k, t) = scene_of("h8"), (131, 60, 4, 32)
    r = rt_host.Renderer(rt_host.flatten_scene(s), 0, lib)
    try:
        dev = adaptive(lib, r, w, h, k, t)
    finally:
        r.close()
    frame, st, refined, mask = rt_host.render_adaptive(w, h, s, k, t, want_mask=True, lib=lib)
    assert frame == dev[0] and refined == dev[2] and (np.frombuffer(mask, np.uint8).reshape(h, w) == dev[1]).all()
    assert st.pixels == w * h and st.kernel_ms > 0
    assert rt_host.render_adaptive(w, h, s, k, t, lib=lib)[:3:2] == (frame, refined)
    e = dict(s, camera=dict(s["camera"], origin=[0.4, 1.7, 9.5]))
    uploads = lib.rt_test_upload_count()
    moved = rt_host.render_adaptive(w, h, e, k, t, lib=lib)
    assert lib.rt_test_upload_count() == uploads                   # the resident scene took the camera as an edit
    r = rt_host.Renderer(rt_host.flatten_scene(e), 0, lib)
    try:
        dev = adaptive(lib, r, w, h, k, t)
    finally:
        r.close()
    assert moved[0] == dev[0] and moved[2] == dev[2] and moved[0] != frame


def test_node_agrees_with_python(lib):
    name, w, h, k, t = "h8", 131, 60, 4, 32
    pkg = os.path.join(ROOT, "html5-canvas-raytracer_amd")
    out = subprocess.check_output([ou.node_path(), os.path.join(ROOT, "tests", "js_adaptive_check.js"), pkg, name, str(w), str(h), str(k), str(t)],
                                  text=True, timeout=300)
    res = json.loads(out.strip().splitlines()[-1])
    frame, _, refined = rt_host.render_adaptive(w, h, scene_of(name), k, t, lib=lib)
    assert base64.b64decode(res["frame"]) == frame and res["refined"] == refined and res["pixels"] == w * h
    assert base64.b64decode(res["plain"]) == fresh(lib, scene_of(name), w, h) and res["plainRefined"] is True
    assert res["into"] is True and res["later"] is True and res["bad"] == [True, True]


def test_a_supersampled_scene_is_refused(lib):
    r = rt_host.Renderer(rt_host.flatten_scene(dict(scene_of("h8"), supersample=2)), 0, lib)
    out, work = nu.Dev(lib, 64 * 48 * 4), nu.Dev(lib, 16 + 4 * 64 * 48)
    try:
        rc = lib.rt_render_adaptive_device(r.handle, 64, 48, 2, 32, C.c_void_p(out.ptr), None, C.c_void_p(work.ptr), work.nbytes, None, 0, None)
        assert rc == INVALID and b"supersample" in lib.rt_last_error()
        assert (out.read() == nu.CANARY).all() and (work.read() == nu.CANARY).all()
    finally:
        out.close(); work.close(); r.close()
