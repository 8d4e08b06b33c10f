"""Moving and restyling the spheres of a resident scene on the GPU (include/rt_hip.h: rt_scene_set_objects).  The yardstick is a fresh
upload of the edited blob: every sphere-dependent region of the scene (the test build's rt_test_scene_state) and the launch table must
be its words, every frame its bytes (and within 1 LSB of the C restatement), every pick its record - whatever the order of camera
moves, seeds and object moves in between, and with nothing waited for on the host between a move and its frame."""
import copy
import ctypes as C
import random

import numpy as np
import pytest

import rt_host
from objects_util import FAST, PARTS, SKYBOX_R2, STRICT, Frames, fresh, gpu_table, host_table, load, near_oracle, set_objects, state, tlib  # noqa: F401

pytestmark = pytest.mark.gpu


def edit(scene, seed, k=4):
    """A copy of `scene` with a seeded random subset of its spheres moved and recoloured, and one mirror made refractive; returns
    (scene, first, last + 1) - the range that covers the changes."""
    s = copy.deepcopy(scene)
    rng = random.Random(seed)
    objs = s["objects"]
    movable = [i for i, o in enumerate(objs) if o["r2"] < 1e4]       # (not the skybox, not the ground)
    changed = sorted(rng.sample(movable, min(k, len(movable))))
    for i in changed:
        o = objs[i]
        o["origin"] = [c + rng.uniform(-0.3, 0.3) for c in o["origin"]]
        o["mtl"]["color"] = [min(1.0, max(0.0, c + rng.uniform(-0.2, 0.2))) for c in o["mtl"]["color"]]
    mirror = next((i for i in movable if objs[i]["mtl"]["albedo"][3] > 0 and objs[i]["mtl"]["albedo"][4] == 0), None)
    if mirror is not None:
        objs[mirror]["mtl"]["albedo"][4] = 0.6
        objs[mirror]["mtl"]["refract_index"] = 1.33
        changed.append(mirror)
    return s, min(changed), max(changed) + 1


@pytest.mark.parametrize("name", ["h8", "default14", "default14_stars", "lcg64", "many:3"])
def test_a_move_leaves_the_words_of_a_fresh_upload(tlib, name):
    s0 = load(name)
    w, h = 160, 96
    r = rt_host.Renderer(rt_host.flatten_scene(s0), 0, tlib)
    try:
        first = Frames(tlib, w, h, (h, 0, 1, 1))
        first.render(r)                                      # a launch table in use: the move rebuilds it on the side stream
        cur = s0
        for seed in (1, 2):
            cur, a, b = edit(cur, seed)
            set_objects(r, cur, a, b)
            blob = rt_host.flatten_scene(cur)
            f = rt_host.Renderer(blob, 0, tlib)
            try:
                got, want = state(tlib, r), state(tlib, f)
                for part in PARTS:
                    assert got[part] == want[part], (name, seed, part)
            finally:
                f.close()
            for ranked in (7, 3):
                assert gpu_table(tlib, r, w, h, (h, 0, 1, 1), ranked, s0.get("supersample", 1)) == host_table(tlib, blob, w, h, (h, 0, 1, 1), ranked), (name, seed, ranked)
        first.read()
    finally:
        r.close()


@pytest.mark.parametrize("name,w,h,tiles,n_frames", [
    ("default14", 96, 64, None, 1),          # the refraction kernel
    ("lcg64", 64, 48, None, 1),              # 2x2 supersampling, the many-sphere kernel
    ("h8", 64, 100, (16, 1, 2, 3), 1),       # a tiled band
    ("default14", 64, 40, None, 2)])         # a batch
@pytest.mark.parametrize("flags", [FAST, STRICT])
def test_frames_follow_the_moves_without_a_host_wait(tlib, name, w, h, tiles, n_frames, flags):
    s0 = load(name)
    s1, a1, b1 = edit(s0, 11)
    s2, a2, b2 = edit(s1, 12)
    tiles = tiles or (h, 0, 1, 1)
    r = rt_host.Renderer(rt_host.flatten_scene(s0), 0, tlib)
    try:
        fr = Frames(tlib, w, h, tiles, n_frames)
        fr.render(r, flags)
        set_objects(r, s1, a1, b1)
        fr.render(r, flags)
        set_objects(r, s2, a2, b2)
        fr.render(r, flags)
        got = fr.read()
    finally:
        r.close()
    for k, sc in enumerate((s0, s1, s2)):
        assert got[k] == fresh(tlib, sc, w, h, tiles, flags, n_frames), (name, k)
        if tiles == (h, 0, 1, 1) and n_frames == 1:
            assert near_oracle(got[k], sc, w, h), (name, k)


def test_camera_seed_and_object_moves_interleave(tlib):
    import soak_gpu_parity as soak
    w, h = 96, 64
    s0 = load("default14_stars")
    cam = soak.look_at([0.7, 0.3, -0.4], [0.0, 1.0, 0.0], [0.0, 1.0, 0.0])
    r = rt_host.Renderer(rt_host.flatten_scene(s0), 0, tlib)
    try:
        fr = Frames(tlib, w, h, (h, 0, 1, 1))
        want = []
        s1, a, b = edit(s0, 21)
        r.set_camera(cam); set_objects(r, s1, a, b)                  # camera, then objects
        s1 = dict(s1, camera=cam)
        fr.render(r); want.append(s1)
        s2, a, b = edit(s1, 22)
        set_objects(r, s2, a, b); r.set_stars_seed(77)              # objects, then the seed
        s2 = dict(s2, starsSeed=77)
        fr.render(r); want.append(s2)
        s3, a, b = edit(s2, 23)
        cam3 = soak.look_at([-0.5, 0.2, 0.3], [0.0, 1.0, 0.5], [0.0, 1.0, 0.0])
        set_objects(r, s3, a, b); r.set_camera(cam3)                 # objects, then the camera
        s3 = dict(s3, camera=cam3)
        fr.render(r); want.append(s3)
        got = fr.read()
    finally:
        r.close()
    for k, sc in enumerate(want):
        assert got[k] == fresh(tlib, sc, w, h), k


def test_a_light_on_a_moved_surface_switches_to_the_strict_kernel(tlib):
    w, h = 97, 61                                                    # odd: centre row and column are traced again
    s0 = load("default14")
    s1 = copy.deepcopy(s0)
    L = s1["lights"][0]
    i = next(i for i, o in enumerate(s1["objects"]) if o["r2"] < 1e4)
    o = s1["objects"][i]
    o["origin"] = [L[0] + 0.5, L[1] - 0.25, L[2] + 0.125]
    x, y, z = L[0] - o["origin"][0], L[1] - o["origin"][1], L[2] - o["origin"][2]
    o["r2"] = x * x + y * y + z * z                                  # the light exactly on its surface
    r = rt_host.Renderer(rt_host.flatten_scene(s0), 0, tlib)
    f = rt_host.Renderer(rt_host.flatten_scene(s1), 0, tlib)
    try:
        d = tlib.rt_alloc_device(0, w * h * 4)
        st0 = r.render_tiles(w, h, d, None, want_stats=True)
        set_objects(r, s1, i, i + 1)
        st = r.render_tiles(w, h, d, None, want_stats=True)
        got = C.create_string_buffer(w * h * 4)
        assert tlib.rt_copy_to_host(0, got, d, w * h * 4) == 0
        stf = f.render_tiles(w, h, d, None, want_stats=True)
        want = C.create_string_buffer(w * h * 4)
        assert tlib.rt_copy_to_host(0, want, d, w * h * 4) == 0
        tlib.rt_free_device(0, d)
        assert got.raw == want.raw
        assert st.exact_samples == stf.exact_samples, (st0.exact_samples, st.exact_samples, stf.exact_samples)
    finally:
        r.close()
        f.close()


def test_hits_and_pick_follow_a_move(tlib):
    w, h = 128, 80
    s0 = load("default14")
    s1, a, b = edit(s0, 31, k=2)
    r = rt_host.Renderer(rt_host.flatten_scene(s0), 0, tlib)
    f = rt_host.Renderer(rt_host.flatten_scene(s1), 0, tlib)
    n = w * h
    try:
        set_objects(r, s1, a, b)
        out = []
        for x in (r, f):
            di, dd = tlib.rt_alloc_device(0, n * 4), tlib.rt_alloc_device(0, n * 8)
            x.render_hits(w, h, di, dd, None)
            hi, hd = C.create_string_buffer(n * 4), C.create_string_buffer(n * 8)
            assert tlib.rt_copy_to_host(0, hi, di, n * 4) == 0 and tlib.rt_copy_to_host(0, hd, dd, n * 8) == 0
            tlib.rt_free_device(0, di); tlib.rt_free_device(0, dd)
            out.append((hi.raw, hd.raw))
        assert out[0] == out[1]
        ids = np.frombuffer(out[1][0], dtype=np.int32).reshape(h, w)
        moved = [i for i in range(a, b) if ((ids & 0xffff) == i).any() and s1["objects"][i] != s0["objects"][i]]
        assert moved
        ys, xs = np.nonzero((ids & 0xffff) == moved[0])
        pt = [(int(xs[len(xs) // 2]), int(ys[len(ys) // 2]))]
        p, q = r.pick(w, h, pt)[0], f.pick(w, h, pt)[0]
        assert p is not None and p["object"] == moved[0]
        assert p == q
    finally:
        r.close()
        f.close()


def test_bad_edits_are_refused_and_change_nothing(tlib):
    w, h = 96, 64
    s0 = load("default14")
    blob0 = rt_host.flatten_scene(s0)
    r = rt_host.Renderer(blob0, 0, tlib)
    try:
        before = Frames(tlib, w, h, (h, 0, 1, 1)); before.render(r)
        rec = bytearray(rt_host.sphere_records(s0["objects"][1:2]))
        n = len(s0["objects"])
        buf = C.create_string_buffer(bytes(rec), len(rec))
        assert tlib.rt_scene_set_objects(r.handle, n, 1, buf, None) == -1                    # outside [0, n_objects)
        assert tlib.rt_scene_set_objects(r.handle, n - 1, 2, buf, None) == -1
        bad_kind = bytearray(rec); bad_kind[176:180] = (9).to_bytes(4, "little", signed=True)
        bad_tex = bytearray(rec); bad_tex[176:180] = (1).to_bytes(4, "little"); bad_tex[180:184] = (99).to_bytes(4, "little", signed=True)
        for bad in (bad_kind, bad_tex):
            assert tlib.rt_scene_set_objects(r.handle, 1, 1, C.create_string_buffer(bytes(bad), len(bad)), None) == -1
        sky = next(i for i, o in enumerate(s0["objects"]) if o["r2"] == SKYBOX_R2)
        small = copy.deepcopy(s0)
        small["objects"][sky]["r2"] = 4.0                                                      # no longer encloses everything
        srec = rt_host.sphere_records(small["objects"][sky:sky + 1])
        assert tlib.rt_scene_set_objects(r.handle, sky, 1, C.create_string_buffer(srec, len(srec)), None) == -2
        after = Frames(tlib, w, h, (h, 0, 1, 1)); after.render(r)
        assert before.read() == after.read()
        # the host form re-uploads such an edit and still draws it right
        got, _ = rt_host.render(w, h, small, lib=tlib)
        assert got == fresh(tlib, small, w, h)
    finally:
        r.close()


def test_host_form_renders_an_orbit_without_uploads(tlib):
    import math
    w, h = 96, 64
    s = load("default14")
    i = next(i for i, o in enumerate(s["objects"]) if o["r2"] < 1e4)
    c0 = list(s["objects"][i]["origin"])
    rt_host.render(w, h, s, lib=tlib)
    uploads = tlib.rt_test_upload_count()
    for k in range(4):
        a = 0.4 * (k + 1)
        s["objects"][i]["origin"] = [c0[0] + 0.5 * math.cos(a), c0[1], c0[2] + 0.5 * math.sin(a)]
        got, _ = rt_host.render(w, h, s, lib=tlib)
        assert tlib.rt_test_upload_count() == uploads, k
        assert got == fresh(tlib, s, w, h), k
        uploads = tlib.rt_test_upload_count()              # (the fresh upload of the yardstick)
