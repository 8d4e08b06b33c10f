"""Moving the lights of a resident scene on the GPU (include/rt_hip.h: rt_scene_set_lights, rt_scene_set_light_intensity).  The
yardstick is a fresh upload of the edited blob: every region of the scene (the test build's rt_test_scene_state) and the launch table
must be its words, every frame its bytes (and within 1 LSB of the C restatement), every ray and pick its record - whatever the order
of camera moves, seeds, object moves and light moves in between, and with nothing waited for on the host between a move and its
frame.  The light edits are seeded (lights_util.move_lights: every light by a uniform offset in +-2 per axis, once with two lights
exchanged)."""
import copy
import ctypes as C
import math

import numpy as np
import pytest

import rt_host
from lights_util import move_lights, set_lights
from objects_util import FAST, PARTS, STRICT, Frames, fresh, gpu_table, host_table, load, near_oracle, set_objects, state, tlib  # noqa: F401
from test_gpu_objects import edit

pytestmark = pytest.mark.gpu

INVALID, UNSUPPORTED = -1, -2
GEOMETRY, GRIDS, BOUNCE = 1, 4, 5


def assert_state_of_a_fresh_upload(lib, r, scene, what):
    f = rt_host.Renderer(rt_host.flatten_scene(scene), 0, lib)
    try:
        got, want = state(lib, r), state(lib, f)
        for part in PARTS:
            assert got[part] == want[part], (what, part)
    finally:
        f.close()
    return got


# ------------------------------------------------------------------ 1. words
@pytest.mark.parametrize("name", ["h8", "default14", "default14_stars", "lcg64", "many:3"])
def test_a_light_move_leaves_the_words_of_a_fresh_upload(tlib, name):
    s0 = load(name)
    w, h = 160, 96
    r = rt_host.Renderer(rt_host.flatten_scene(s0), 0, tlib)
    try:
        first = Frames(tlib, w, h, (h, 0, 1, 1))
        first.render(r)                                      # a launch table in use: the move rebuilds it on the side stream
        before = state(tlib, r)
        cur = s0
        for seed, swap in ((1, False), (2, True)):
            cur = move_lights(cur, seed, swap)
            set_lights(r, cur)
            got = assert_state_of_a_fresh_upload(tlib, r, cur, (name, seed))
            assert got[GEOMETRY] != before[GEOMETRY], (name, seed)          # (the comparison cannot pass on a move that did nothing)
            assert got[BOUNCE] == before[BOUNCE], (name, seed)              # the bounce table does not depend on the lights
            if name in ("lcg64", "many:3"):
                assert len(got[GRIDS]) > 0 and got[GRIDS] != before[GRIDS], (name, seed)
            before = got
            blob = rt_host.flatten_scene(cur)
            for ranked in (7, 3):
                assert gpu_table(tlib, r, w, h, (h, 0, 1, 1), ranked, s0.get("supersample", 1)) == host_table(tlib, blob, w, h, (h, 0, 1, 1), ranked), (name, seed, ranked)
        first.read()
    finally:
        r.close()


def test_one_light_of_several_moves_alone(tlib):
    """`first` and `count`: the second light alone, then the first alone - each time the state of a fresh upload."""
    s0 = load("lcg64")
    r = rt_host.Renderer(rt_host.flatten_scene(s0), 0, tlib)
    try:
        s1 = copy.deepcopy(s0)
        s1["lights"][1] = [-3.0, 7.5, 2.0]
        r.set_lights([s1["lights"][1]], first=1)
        assert_state_of_a_fresh_upload(tlib, r, s1, "second")
        s2 = copy.deepcopy(s1)
        s2["lights"][0] = [4.0, 12.0, 6.5]
        r.set_lights(s2["lights"][:1])
        assert_state_of_a_fresh_upload(tlib, r, s2, "first")
        r.set_lights([], first=2)                           # an empty range at the end is no move
        assert_state_of_a_fresh_upload(tlib, r, s2, "empty")
    finally:
        r.close()


# ------------------------------------------------------------------ 2. frames without a host wait
@pytest.mark.parametrize("name,w,h,tiles,n_frames", [
    ("default14", 96, 64, None, 1),          # the refraction kernel
    ("lcg64", 64, 48, None, 1),              # 2x2 supersampling, the many-sphere kernel
    ("h8", 64, 100, (16, 1, 2, 3), 1),       # a tiled band
    ("default14", 64, 40, None, 2)])         # a batch
@pytest.mark.parametrize("flags", [FAST, STRICT])
def test_frames_follow_the_light_moves_without_a_host_wait(tlib, name, w, h, tiles, n_frames, flags):
    s0 = load(name)
    s1 = move_lights(s0, 11)
    s2 = move_lights(s1, 12, swap=True)
    tiles = tiles or (h, 0, 1, 1)
    r = rt_host.Renderer(rt_host.flatten_scene(s0), 0, tlib)
    try:
        fr = Frames(tlib, w, h, tiles, n_frames)
        fr.render(r, flags)
        set_lights(r, s1)
        fr.render(r, flags)
        set_lights(r, s2)
        fr.render(r, flags)
        got = fr.read()
    finally:
        r.close()
    assert got[0] != got[1] and got[1] != got[2] and got[0] != got[2], name
    for k, sc in enumerate((s0, s1, s2)):
        assert got[k] == fresh(tlib, sc, w, h, tiles, flags, n_frames), (name, k)      # (enqueued frames kept their lights)
        if tiles == (h, 0, 1, 1) and n_frames == 1:
            assert near_oracle(got[k], sc, w, h), (name, k)


def test_enqueued_frames_keep_their_intensity(tlib):
    w, h = 96, 64
    s0 = load("default14")
    scenes = [s0, dict(s0, light_intensity=20.0), dict(s0, light_intensity=75.5)]
    r = rt_host.Renderer(rt_host.flatten_scene(s0), 0, tlib)
    try:
        fr = Frames(tlib, w, h, (h, 0, 1, 1))
        fr.render(r)
        for sc in scenes[1:]:
            r.set_light_intensity(sc["light_intensity"])
            fr.render(r)
        got = fr.read()
        assert_state_of_a_fresh_upload(tlib, r, scenes[-1], "intensity")
    finally:
        r.close()
    assert got[0] != got[1] and got[1] != got[2] and got[0] != got[2]
    for k, sc in enumerate(scenes):
        assert got[k] == fresh(tlib, sc, w, h), k
        assert near_oracle(got[k], sc, w, h), k


# ------------------------------------------------------------------ 3. interleaving
def test_camera_seed_object_and_light_moves_interleave(tlib):
    import soak_gpu_parity as soak
    w, h = 96, 64
    s0 = load("default14_stars")
    cam = soak.look_at([0.7, 0.3, -0.4], [0.0, 1.0, 0.0], [0.0, 1.0, 0.0])
    r = rt_host.Renderer(rt_host.flatten_scene(s0), 0, tlib)
    try:
        fr = Frames(tlib, w, h, (h, 0, 1, 1))
        want = []
        s1 = dict(move_lights(s0, 21), camera=cam)
        r.set_camera(cam); set_lights(r, s1)                         # camera, then lights
        fr.render(r); want.append(s1)
        s2 = dict(move_lights(s1, 22), starsSeed=77)
        set_lights(r, s2); r.set_stars_seed(77)                      # lights, then the seed
        fr.render(r); want.append(s2)
        s3, a, b = edit(move_lights(s2, 23, swap=True), 23)
        set_lights(r, s3); set_objects(r, s3, a, b)                  # lights, then objects
        fr.render(r); want.append(s3)
        s4, a, b = edit(s3, 24)
        s4 = move_lights(s4, 24)
        set_objects(r, s4, a, b); set_lights(r, s4)                  # objects, then lights
        fr.render(r); want.append(s4)
        s5 = dict(move_lights(s4, 25), light_intensity=33.0)
        r.set_light_intensity(33.0); set_lights(r, s5)               # the intensity, then lights
        fr.render(r); want.append(s5)
        got = fr.read()
    finally:
        r.close()
    for k, sc in enumerate(want):
        assert got[k] == fresh(tlib, sc, w, h), k


@pytest.mark.parametrize("name", ["lcg64", "many:3"])
def test_an_object_move_after_a_light_move_builds_its_grids_from_the_new_lights(tlib, name):
    """Scenes with shadow grids: the object move rebuilds every light's grid on the GPU - from the lights of the move before it, not
    from the ones the scene was uploaded with.  Then a camera move (a copy of the other block) and one more light move."""
    import soak_gpu_parity as soak
    w, h = 64, 48
    s0 = load(name)
    r = rt_host.Renderer(rt_host.flatten_scene(s0), 0, tlib)
    try:
        fr = Frames(tlib, w, h, (h, 0, 1, 1))
        fr.render(r)
        s1 = move_lights(s0, 31)
        set_lights(r, s1)
        s2, a, b = edit(s1, 32)
        set_objects(r, s2, a, b)
        got = assert_state_of_a_fresh_upload(tlib, r, s2, (name, "lights, objects"))
        assert len(got[GRIDS]) > 0
        fr.render(r)
        c = s0["camera"]["origin"]
        cam = soak.look_at([c[0] + 0.25, c[1] + 0.125, c[2] - 0.25], [c[0] + s0["camera"]["axisZ"][0], c[1] + s0["camera"]["axisZ"][1], c[2] + s0["camera"]["axisZ"][2]], [0.0, 1.0, 0.0])
        s3 = dict(move_lights(s2, 33, swap=True), camera=cam)
        set_lights(r, s3); r.set_camera(cam)
        assert_state_of_a_fresh_upload(tlib, r, s3, (name, "lights, camera"))
        fr.render(r)
        s4 = move_lights(s3, 34)
        set_lights(r, s4)
        assert_state_of_a_fresh_upload(tlib, r, s4, (name, "lights again"))
        fr.render(r)
        frames = fr.read()
    finally:
        r.close()
    for k, sc in enumerate((s0, s2, s3, s4)):
        assert frames[k] == fresh(tlib, sc, w, h), (name, k)


# ------------------------------------------------------------------ 4. the strict switch
def test_a_light_moved_onto_a_surface_switches_to_the_strict_kernel(tlib):
    w, h = 97, 61                                                    # odd: centre row and column are traced again
    s0 = load("default14")
    i = next(i for i, o in enumerate(s0["objects"]) if o["r2"] == 1.0)          # r2 a perfect square: the coincidence is exact
    o = s0["objects"][i]
    s1 = copy.deepcopy(s0)
    s1["lights"][0] = [o["origin"][0] + math.sqrt(o["r2"]), o["origin"][1], o["origin"][2]]
    x = s1["lights"][0][0] - o["origin"][0]
    assert x * x + 0.0 + 0.0 == o["r2"]
    r = rt_host.Renderer(rt_host.flatten_scene(s0), 0, tlib)
    f = rt_host.Renderer(rt_host.flatten_scene(s1), 0, tlib)
    try:
        d = tlib.rt_alloc_device(0, w * h * 4)

        def frame_of(x):
            st = x.render_tiles(w, h, d, None, want_stats=True)
            host = C.create_string_buffer(w * h * 4)
            assert tlib.rt_copy_to_host(0, host, d, w * h * 4) == 0
            return host.raw, st.exact_samples
        first, n0 = frame_of(r)
        set_lights(r, s1)
        got, n1 = frame_of(r)
        want, nf = frame_of(f)
        assert got == want
        assert n1 == nf, (n0, n1, nf)
        assert n1 != n0, (n0, n1)                                    # (every sample is the strict kernel's now)
        set_lights(r, s0)                                            # ... and away again
        back, n2 = frame_of(r)
        tlib.rt_free_device(0, d)
        assert back == first and n2 == n0, (n0, n2)
    finally:
        r.close()
        f.close()


# ------------------------------------------------------------------ 5. other consumers
def test_rays_hits_and_pick_follow_a_light_move(tlib):
    from test_gpu_rays import DeviceRays
    w, h = 64, 40
    s0 = load("default14")
    s1 = move_lights(s0, 41, swap=True)
    rays = rt_host.primary_rays(w, h, s1)
    n = w * h
    r = rt_host.Renderer(rt_host.flatten_scene(s0), 0, tlib)
    f = rt_host.Renderer(rt_host.flatten_scene(s1), 0, tlib)
    try:
        dr = DeviceRays(tlib, rays)
        dr.run(r)
        old = dr.read("rgba").tobytes()
        set_lights(r, s1)
        out = []
        for x in (r, f):
            dr.run(x)
            rec = [dr.read(k).tobytes() for k in ("rgb", "rgba", "hits")]
            di, dd = tlib.rt_alloc_device(0, n * 4), tlib.rt_alloc_device(0, n * 8)
            x.render_hits(w, h, di, dd, None)
            hi, hd = C.create_string_buffer(n * 4), C.create_string_buffer(n * 8)
            assert tlib.rt_copy_to_host(0, hi, di, n * 4) == 0 and tlib.rt_copy_to_host(0, hd, dd, n * 8) == 0
            tlib.rt_free_device(0, di); tlib.rt_free_device(0, dd)
            out.append(rec + [hi.raw, hd.raw, x.pick(w, h, [(w // 2, h // 2), (5, h - 3), (w - 2, 1)])])
        dr.close()
        for k, what in enumerate(("rgb", "rgba", "ray hits", "ids", "depths", "picks")):
            assert out[0][k] == out[1][k], what
        assert out[0][1] != old                                      # the rays saw the move
        assert out[0][1] == fresh(tlib, s1, w, h, flags=STRICT)      # (the list of a frame's primary rays is its strict frame)
    finally:
        r.close()
        f.close()


# ------------------------------------------------------------------ 6. refusals
def test_bad_light_moves_are_refused_and_change_nothing(tlib):
    w, h = 96, 64
    s0 = load("default14")
    r = rt_host.Renderer(rt_host.flatten_scene(s0), 0, tlib)
    try:
        before = Frames(tlib, w, h, (h, 0, 1, 1)); before.render(r)
        state0 = state(tlib, r)
        n = len(s0["lights"])
        xyz = (C.c_double * 6)(1.0, 2.0, 3.0, 4.0, 5.0, 6.0)
        assert tlib.rt_scene_set_lights(r.handle, n, 1, xyz, None) == INVALID               # outside [0, n_lights)
        assert tlib.rt_scene_set_lights(r.handle, n - 1, 2, xyz, None) == INVALID
        assert tlib.rt_scene_set_lights(r.handle, 1, 0xFFFFFFFF, xyz, None) == INVALID
        assert tlib.rt_scene_set_lights(r.handle, 0, 1, None, None) == INVALID               # NULL positions with a count
        outside = copy.deepcopy(s0)
        outside["lights"][1] = [0.0, 6000.0, 0.0]                                            # beyond the skybox (radius 5000)
        far = (C.c_double * 3)(*outside["lights"][1])
        assert tlib.rt_scene_set_lights(r.handle, 1, 1, far, None) == UNSUPPORTED
        assert state(tlib, r) == state0
        after = Frames(tlib, w, h, (h, 0, 1, 1)); after.render(r)
        assert before.read() == after.read()
        # the host form uploads such a scene and still draws it right
        rt_host.render(w, h, s0, lib=tlib)
        uploads = tlib.rt_test_upload_count()
        got, _ = rt_host.render(w, h, outside, lib=tlib)
        assert tlib.rt_test_upload_count() == uploads + 1
        assert got == fresh(tlib, outside, w, h)
    finally:
        r.close()


# ------------------------------------------------------------------ 7. no uploads
def test_host_form_renders_an_orbiting_fading_light_without_uploads(tlib):
    w, h = 96, 64
    s = load("default14")
    c0 = list(s["lights"][0])
    rt_host.render(w, h, s, lib=tlib)
    uploads = tlib.rt_test_upload_count()
    seen = set()
    for k in range(4):
        a = 0.4 * (k + 1)
        s["lights"][0] = [c0[0] + 3.0 * math.cos(a), c0[1], c0[2] + 3.0 * math.sin(a)]
        s["light_intensity"] = 50.0 - 6.0 * (k + 1)
        got, _ = rt_host.render(w, h, s, lib=tlib)
        assert tlib.rt_test_upload_count() == uploads, k
        assert got == fresh(tlib, s, w, h), k
        seen.add(got)
        uploads = tlib.rt_test_upload_count()              # (the fresh upload of the yardstick)
    assert len(seen) == 4
    # hits, picks and ray lists of the host form share that resident scene
    s["lights"][1] = [c0[0] - 1.0, c0[1] + 2.0, c0[2]]
    rays = rt_host.primary_rays(w, h, s)
    rgba = rt_host.trace_rays(s, rays, want=("rgba",), lib=tlib)["rgba"]
    assert tlib.rt_test_upload_count() == uploads
    assert rgba.tobytes() == fresh(tlib, s, w, h, flags=STRICT)


# ------------------------------------------------------------------ 8. equal positions
def test_setting_the_current_lights_again_changes_nothing(tlib):
    w, h = 96, 64
    s0 = load("lcg64")
    r = rt_host.Renderer(rt_host.flatten_scene(s0), 0, tlib)
    try:
        fr = Frames(tlib, w, h, (h, 0, 1, 1))
        fr.render(r)
        state0 = state(tlib, r)
        set_lights(r, s0)
        r.set_lights(s0["lights"][1:], first=1)
        assert state(tlib, r) == state0
        fr.render(r)
        a, b = fr.read()
        assert a == b
    finally:
        r.close()
