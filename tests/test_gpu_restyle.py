"""Restyling the spheres of a resident scene on the GPU (include/rt_hip.h: rt_scene_set_objects) in the ways that change the host's
decisions (rt_scene.hip: object_decisions, camera_decisions): the kernel variant (refraction), strict-kernel routing, the samplers'
boundary tolerance, the mark-weight rule, the enclosing sphere's background, the bounce table's used rows, radii (also degenerate
ones), a camera inside a moved sphere and every texture index of a scene with sixteen textures of odd shapes.  Each edit goes
A -> B -> A.  The yardsticks: a fresh upload of the edited blob (every sphere-dependent region, the launch table, FAST and STRICT
frames, the exact-sample count, hits and picks) and the C restatement, which shares no host decision with the library."""
import copy
import ctypes as C
import math

import numpy as np
import pytest

import nodes_util as nu
import rt_host
import texture_util as tu
from objects_util import FAST, PARTS, SKYBOX_R2, STRICT, Frames, fresh, gpu_table, host_table, load, oracle_gap, state, tlib  # noqa: F401

pytestmark = pytest.mark.gpu

W, H = 160, 96
RT_ERR_UNSUPPORTED = -2


def scene_of(name):
    if name == "lcg64_nosky":                                   # many spheres and no enclosing sphere: any radius may change
        s = load("lcg64")
        s["objects"] = [o for o in s["objects"] if o["r2"] != SKYBOX_R2]
        return s
    return load(name)


def sky_of(s):
    return next(i for i, o in enumerate(s["objects"]) if o["r2"] == SKYBOX_R2)


def small_rank(s, i):
    o = s["objects"][i]
    return -math.sqrt(max(o["r2"], 0.0)) / math.dist(o["origin"], s["camera"]["origin"])


def by_size(s):
    """Indices of the spheres of `s` from the largest apparent size (radius over distance from the camera) down, skybox and ground left out."""
    return sorted((i for i, o in enumerate(s["objects"]) if o["r2"] < 1e4), key=lambda i: small_rank(s, i))


def small(s, k=0):
    return by_size(s)[k]


def matte(s):
    return next(i for i in by_size(s) if s["objects"][i]["mtl"]["albedo"][3] == 0 and s["objects"][i]["mtl"]["albedo"][4] == 0)


def mirror(s):
    return next(i for i in by_size(s) if s["objects"][i]["mtl"]["albedo"][3] > 0 and s["objects"][i]["mtl"]["albedo"][4] == 0)


def checker(m, fu, fv):
    m["sampler"] = {"kind": rt_host.SAMPLER_CHECKER, "freqU": fu, "freqV": fv, "colors": [[0.9, 0.8, 0.1], [0.1, 0.3, 0.9]]}


# ---- the restyles: f(scene) edits a copy in place and returns the indices it changed; `strict`: the edited scene is a strict-kernel scene
def r_refract_off(s):
    ids = [i for i, o in enumerate(s["objects"]) if o["mtl"]["albedo"][4] > 0]
    assert ids
    for i in ids:
        s["objects"][i]["mtl"]["albedo"][4] = 0.0
    return ids


def r_refract_on(s):
    assert not any(o["mtl"]["albedo"][4] > 0 for o in s["objects"])
    i = small(s)
    s["objects"][i]["mtl"]["albedo"][4] = 0.7
    s["objects"][i]["mtl"]["refract_index"] = 1.4
    return [i]


def r_radius_zero(s):
    i = small(s, 1)
    s["objects"][i]["r2"] = 0.0
    return [i]


def r_radius_negative(s):
    i = small(s, 1)
    s["objects"][i]["r2"] = -0.25
    return [i]


def r_radius_nan(s):
    i = small(s, 2)
    s["objects"][i]["r2"] = float("nan")
    return [i]


def r_checker_negative(s):
    i = small(s)
    checker(s["objects"][i]["mtl"], -3.0, 2.0)
    return [i]


def r_checker_nan(s):
    i = small(s)
    checker(s["objects"][i]["mtl"], float("nan"), 2.0)
    return [i]


def r_checker_2_31(s):
    i = small(s)
    checker(s["objects"][i]["mtl"], 4.0, 2147483648.0)
    return [i]


def r_checker_fine(s):                                             # beyond the product kernel's 2^17 per unit
    i = small(s)
    checker(s["objects"][i]["mtl"], 200000.0, 3.0)
    return [i]


def r_checker_wider_tol(s):                                        # a finer checker that the product kernel still takes: flag_tol grows
    i = small(s)
    checker(s["objects"][i]["mtl"], 60000.0, 3.0)
    return [i]


def r_light_on_surface(s):
    L = s["lights"][0]
    i = small(s, 1)
    o = s["objects"][i]
    o["origin"] = [L[0] + 0.5, L[1] - 0.25, L[2] + 0.125]
    x, y, z = L[0] - o["origin"][0], L[1] - o["origin"][1], L[2] - o["origin"][2]
    o["r2"] = x * x + y * y + z * z                                # the light exactly on its surface
    return [i]


def r_colour_over_one(s):
    i = small(s)
    s["objects"][i]["mtl"]["color"] = [1.5, 0.25, 0.5]
    return [i]


def r_albedo_over_one(s):
    i = small(s, 1)
    s["objects"][i]["mtl"]["albedo"][1] = 1.3
    return [i]


def r_colour_negative(s):
    i = small(s, 2)
    s["objects"][i]["mtl"]["color"] = [-0.2, 0.5, 0.5]
    return [i]


def r_matte_to_mirror(s):
    i = matte(s)
    s["objects"][i]["mtl"]["albedo"][3] = 0.5
    return [i]


def r_mirror_to_matte(s):
    i = mirror(s)
    s["objects"][i]["mtl"]["albedo"][3] = 0.0
    return [i]


def r_radius_grow(s):
    ids = [small(s, 0), small(s, 3)]
    for i in ids:
        s["objects"][i]["r2"] *= 2.25
    return ids


def r_radius_shrink(s):
    i = small(s, 1)
    s["objects"][i]["r2"] *= 0.36
    return [i]


def r_camera_inside(s):
    i = small(s, 2)
    c = s["camera"]["origin"]
    s["objects"][i]["origin"] = [c[0] + 0.3, c[1] - 0.2, c[2] + 0.1]
    s["objects"][i]["r2"] = 1.0
    return [i]


def r_sky_colour(s):
    i = sky_of(s)
    s["objects"][i]["mtl"]["color"] = [0.2, 0.4, 0.7]
    s["objects"][i]["mtl"]["sampler"] = {"kind": rt_host.SAMPLER_COLOR}
    return [i]


def r_sky_ambient(s):
    i = sky_of(s)
    s["objects"][i]["mtl"]["color"] = [0.6, 0.5, 0.9]
    s["objects"][i]["mtl"]["albedo"][0] = 0.5
    return [i]


def r_sky_diffuse(s):
    i = sky_of(s)
    s["objects"][i]["mtl"]["color"] = [0.6, 0.5, 0.9]
    s["objects"][i]["mtl"]["albedo"][1] = 0.3
    return [i]


def r_sky_reflect(s):
    i = sky_of(s)
    s["objects"][i]["mtl"]["albedo"][3] = 0.4
    return [i]


def r_sky_stars(s):
    i = sky_of(s)
    s["objects"][i]["mtl"]["sampler"] = {"kind": rt_host.SAMPLER_STARS, "threshold": 0.002, "scale": 1000.0}
    return [i]


def r_sky_texture(s):
    i = sky_of(s)
    s["objects"][i]["mtl"]["sampler"] = {"kind": rt_host.SAMPLER_TEXTURE, "texture": 0}
    s["objects"][i]["mtl"]["color"] = [1.0, 1.0, 1.0]
    return [i]


def r_sky_radius(s):
    i = sky_of(s)
    s["objects"][i]["r2"] = 3.0e7
    return [i]


STRICT_RESTYLES = {r_radius_zero, r_radius_negative, r_radius_nan, r_checker_negative, r_checker_nan, r_checker_2_31, r_checker_fine,
                   r_light_on_surface}
SKY_RESTYLES = {r_sky_colour, r_sky_ambient, r_sky_diffuse, r_sky_reflect, r_sky_stars, r_sky_texture, r_sky_radius}
HIT_RESTYLES = {r_radius_zero, r_radius_negative, r_radius_grow, r_radius_shrink, r_camera_inside, r_sky_radius}

CASES = [
    # the kernel variant: REFRACT and IMAGE_IN_LDS
    ("default14", r_refract_off), ("h8", r_refract_on), ("lcg64", r_refract_on), ("many:10", r_refract_on),
    # strict-kernel routing through a record, and back
    ("default14", r_radius_zero), ("h8", r_checker_negative), ("default14_stars", r_checker_nan), ("h8", r_checker_2_31),
    ("default14", r_checker_fine), ("lcg64", r_light_on_surface), ("lcg64_nosky", r_radius_negative), ("lcg64_nosky", r_radius_nan),
    # the samplers' boundary tolerance
    ("default14", r_checker_wider_tol), ("lcg64", r_checker_wider_tol),
    # the mark-weight rule
    ("default14", r_colour_over_one), ("h8", r_albedo_over_one), ("lcg64", r_colour_negative), ("many:3", r_colour_over_one),
    # the enclosing sphere, still enclosing everything
    ("h8", r_sky_colour), ("default14", r_sky_ambient), ("h8", r_sky_diffuse), ("default14", r_sky_reflect), ("h8", r_sky_stars),
    ("default14_stars", r_sky_colour), ("default14_stars", r_sky_texture), ("h8", r_sky_radius), ("lcg64", r_sky_colour),
    ("lcg64", r_sky_diffuse),
    # bounce-table rows that switch between used and unused
    ("lcg64", r_matte_to_mirror), ("lcg64", r_mirror_to_matte), ("many:3", r_matte_to_mirror), ("lcg64_nosky", r_mirror_to_matte),
    # radii
    ("h8", r_radius_grow), ("lcg64", r_radius_grow), ("lcg64", r_radius_shrink), ("many:3", r_radius_shrink), ("lcg64_nosky", r_radius_zero),
    # a sphere moved over the camera
    ("default14", r_camera_inside), ("lcg64", r_camera_inside),
]


def restyled(s0, fn):
    s = copy.deepcopy(s0)
    ids = fn(s)
    return s, min(ids), max(ids) + 1


def render_with_stats(lib, r, w, h, flags):
    d = lib.rt_alloc_device(0, w * h * 4)
    assert d, lib.rt_last_error()
    try:
        st = r.render_tiles(w, h, d, None, flags=flags, want_stats=True)
        out = C.create_string_buffer(w * h * 4)
        assert lib.rt_copy_to_host(0, out, d, w * h * 4) == 0, lib.rt_last_error()
        return out.raw, st.exact_samples
    finally:
        lib.rt_free_device(0, d)


def check_generation(lib, r, scene, w, h, label, tables=True):
    """The resident scene `r` after an edit against a fresh upload of `scene` and against the C restatement."""
    blob = rt_host.flatten_scene(scene)
    ss = scene.get("supersample", 1)
    f = rt_host.Renderer(blob, 0, lib)
    try:
        got, want = state(lib, r), state(lib, f)
        for part in PARTS:
            assert got[part] == want[part], (label, "state part", part)
        if tables:
            for ranked in (7, 3):
                assert gpu_table(lib, r, w, h, (h, 0, 1, 1), ranked, ss) == host_table(lib, blob, w, h, (h, 0, 1, 1), ranked), (label, "table", ranked)
        frames = {}
        for flags in (FAST, STRICT):
            a, na = render_with_stats(lib, r, w, h, flags)
            b, nb = render_with_stats(lib, f, w, h, flags)
            assert a == b, (label, "frame", flags)
            assert na == nb, (label, "exact samples", flags, na, nb)
            frames[flags] = a
    finally:
        f.close()
    for flags, a in frames.items():
        worst, frac = oracle_gap(a, scene, w, h)
        assert worst <= 1 and frac < 0.01, (label, "oracle", flags, worst, frac)
    return frames[FAST], got


def check_owner_plan(lib, r, want, w, h, strict_scene, label):
    """The sky paths of a frame: senders that leave out the constant background (RT_FLAG_NO_SKY) and an owner that fills it
    (RT_FLAG_SKY_ONLY), then compact bands (RT_FLAG_COMPACT) put back by rt_compact_expand_device - both must give `want`.  A
    strict-kernel scene has no compact bands: RT_ERR_UNSUPPORTED."""
    import shard
    n = w * h * 4
    plan = shard.TilePlan(w, h, 16, 2)
    d = lib.rt_alloc_device(0, n)
    band = lib.rt_alloc_device(0, n + 4096)
    try:
        assert lib.rt_memset_device(0, d, 0, n) == 0
        for g in range(2):
            r.render_scatter(w, h, [d], rt_host.RtTiles(*plan.rt_tiles(g)), flags=rt_host.RT_FLAG_NO_SKY)
        r.render_scatter(w, h, [d], rt_host.RtTiles(h, 0, 1, 1), flags=rt_host.RT_FLAG_SKY_ONLY)
        host = C.create_string_buffer(n)
        assert lib.rt_copy_to_host(0, host, d, n) == 0
        assert host.raw == want, (label, "owner plan")
        tiles = [rt_host.RtTiles(*plan.rt_tiles(g)) for g in range(2)]
        if strict_scene:
            nb, bb = C.c_uint32(), C.c_uint32()
            assert lib.rt_compact_count(r.handle, w, h, C.byref(tiles[0]), None, C.byref(nb), C.byref(bb)) == RT_ERR_UNSUPPORTED, label
            return
        assert lib.rt_memset_device(0, d, 0, n) == 0
        for t in tiles:
            blocks, block_bytes = r.compact_count(w, h, t)
            assert blocks * block_bytes <= n
            r.render_batch(w, h, band, t, 1, 0, flags=rt_host.RT_FLAG_RGB24 | rt_host.RT_FLAG_NO_SKY | rt_host.RT_FLAG_COMPACT)
            r.compact_expand(w, h, t, band, d)
        r.render_scatter(w, h, [d], rt_host.RtTiles(h, 0, 1, 1), flags=rt_host.RT_FLAG_SKY_ONLY)
        assert lib.rt_copy_to_host(0, host, d, n) == 0
        assert host.raw == want, (label, "compact bands")
    finally:
        lib.rt_free_device(0, d)
        lib.rt_free_device(0, band)


def check_hits(lib, r, scene, w, h, ids, label):
    """Hit buffers and picks of `r` equal a fresh upload's; a pick on a restyled sphere, where one shows."""
    f = rt_host.Renderer(rt_host.flatten_scene(scene), 0, lib)
    n = w * h * scene.get("supersample", 1) ** 2
    try:
        out = []
        for x in (r, f):
            di, dd, dn = lib.rt_alloc_device(0, n * 4), lib.rt_alloc_device(0, n * 8), lib.rt_alloc_device(0, n * 12)
            x.render_hits(w, h, di, dd, dn)
            bufs = [C.create_string_buffer(k * n) for k in (4, 8, 12)]
            for buf, dptr, k in zip(bufs, (di, dd, dn), (4, 8, 12)):
                assert lib.rt_copy_to_host(0, buf, dptr, k * n) == 0
                lib.rt_free_device(0, dptr)
            out.append([b.raw for b in bufs])
        assert out[0] == out[1], (label, "hits")
        sw = w * scene.get("supersample", 1)
        idb = np.frombuffer(out[1][0], dtype=np.int32).reshape(-1, sw)
        pts = [(sw // 2, idb.shape[0] // 2), (3, 5)]
        for i in ids:
            ys, xs = np.nonzero((idb >= 0) & ((idb & 0xffff) == i))
            if len(xs):
                pts.append((int(xs[len(xs) // 2]), int(ys[len(ys) // 2])))
        assert r.pick(w, h, pts) == f.pick(w, h, pts), (label, "picks")
    finally:
        f.close()


@pytest.mark.parametrize("name,fn", CASES, ids=["%s-%s" % (n, f.__name__[2:]) for n, f in CASES])
def test_a_restyle_and_its_reversal_leave_the_words_and_frames_of_a_fresh_upload(tlib, name, fn):
    s0 = scene_of(name)
    s1, a, b = restyled(s0, fn)
    strict = fn in STRICT_RESTYLES
    r = rt_host.Renderer(rt_host.flatten_scene(s0), 0, tlib)
    try:
        first = Frames(tlib, W, H, (H, 0, 1, 1))
        first.render(r)                                          # a launch table in use: the edit rebuilds it on the side stream
        first.render(r, STRICT)
        for k, (sc, strict_now) in enumerate(((s1, strict), (s0, False))):
            r.set_objects(sc["objects"][a:b], a)
            label = (name, fn.__name__, "A->B" if k == 0 else "B->A")
            frame, parts = check_generation(tlib, r, sc, W, H, label)
            if k == 0 and name.startswith(("lcg64", "many")):
                assert len(parts[4]) > 0 and len(parts[5]) > 0, (label, "shadow grid / bounce table")    # the many-sphere paths are in play
            if fn in SKY_RESTYLES or strict:
                check_owner_plan(tlib, r, frame, W, H, strict_now, label)
            if fn in HIT_RESTYLES:
                check_hits(tlib, r, sc, W, H, range(a, b), label)
        first.read()
    finally:
        r.close()


def test_restyles_enqueued_without_a_host_wait_keep_their_generations(tlib):
    """Frames and batches enqueued across several restyles - kernel variant, sky, strict routing, marks - with no host wait in between:
    each is the fresh upload's frame of its own generation."""
    w, h = 96, 64
    chain = [r_refract_off, r_sky_colour, r_checker_fine, r_colour_over_one, r_sky_diffuse, r_radius_grow]
    for n_frames in (1, 2):
        for flags in (FAST, STRICT):
            scenes = [load("default14")]
            r = rt_host.Renderer(rt_host.flatten_scene(scenes[0]), 0, tlib)
            try:
                fr = Frames(tlib, w, h, (h, 0, 1, 1), n_frames)
                fr.render(r, flags)
                for fn in chain:
                    s, a, b = restyled(scenes[-1], fn)
                    r.set_objects(s["objects"][a:b], a)
                    scenes.append(s)
                    fr.render(r, flags)
                got = fr.read()
            finally:
                r.close()
            for k, sc in enumerate(scenes):
                assert got[k] == fresh(tlib, sc, w, h, None, flags, n_frames), (n_frames, flags, k)


def test_the_host_form_turns_restyles_into_set_objects(tlib):
    """rt_host.render on a scene dict that differs from the last one only in sphere records: no re-upload, the fresh upload's frame."""
    w, h = 96, 64
    s = load("default14")
    rt_host.render(w, h, s, lib=tlib)
    for fn in (r_sky_colour, r_refract_off, r_checker_fine, r_colour_over_one, r_sky_stars, r_radius_zero, r_camera_inside):
        s, _, _ = restyled(s, fn)
        uploads = tlib.rt_test_upload_count()
        got, _ = rt_host.render(w, h, s, lib=tlib)
        assert tlib.rt_test_upload_count() == uploads, fn.__name__
        assert got == fresh(tlib, s, w, h), fn.__name__


def test_moves_between_renders_on_two_streams(tlib):
    """Launches of the scene in flight on TWO caller streams when a move starts: no single event covers them, and the move drains the
    device and forgets its launch state (rt_scene_sync.h: R2).  Three rounds of render on A, render on B, move - a camera move, a
    one-sphere set_objects, a one-light set_lights - and a last frame on each stream, with the product and the strict kernel: every
    frame is the fresh upload's frame of the scene in that state."""
    w, h = 64, 32
    states = [load("h8")]
    for k in range(3):
        s = copy.deepcopy(states[-1])
        if k == 0:
            s["camera"]["origin"] = [s["camera"]["origin"][0] + 0.75, s["camera"]["origin"][1] + 0.25, s["camera"]["origin"][2] - 0.5]
        elif k == 1:
            s["objects"][small(s)]["origin"][1] += 0.5
        else:
            s["lights"][0] = [s["lights"][0][0] - 3.0, s["lights"][0][1] + 2.0, s["lights"][0][2] + 1.0]
        states.append(s)
    streams = [C.c_void_p(), C.c_void_p()]
    for st in streams:
        assert nu.hip().hipStreamCreate(C.byref(st)) == 0
    try:
        for flags in (FAST, STRICT):
            want = [fresh(tlib, sc, w, h, None, flags) for sc in states]
            assert len(set(want)) == 4                             # (every move shows in the frame)
            r = rt_host.Renderer(rt_host.flatten_scene(states[0]), 0, tlib)
            try:
                bufs = []
                for k in range(4):                                 # three rounds, and the frames of the last move
                    for st in streams:
                        d = tlib.rt_alloc_device(0, w * h * 4)
                        assert d, tlib.rt_last_error()
                        bufs.append(d)
                        r.render_tiles(w, h, d, None, stream=st.value, flags=flags)
                    if k == 0:
                        r.set_camera(states[1]["camera"])
                    elif k == 1:
                        i = small(states[1])
                        r.set_objects(states[2]["objects"][i:i + 1], i)
                    elif k == 2:
                        r.set_lights(states[3]["lights"][:1], 0)
                for st in streams:
                    assert nu.hip().hipStreamSynchronize(st) == 0
                for j, d in enumerate(bufs):
                    host = C.create_string_buffer(w * h * 4)
                    assert tlib.rt_copy_to_host(0, host, d, w * h * 4) == 0, tlib.rt_last_error()
                    tlib.rt_free_device(0, d)
                    assert host.raw == want[j // 2], (flags, "round", j // 2, "stream", j % 2)
            finally:
                r.close()
    finally:
        for st in streams:
            assert nu.hip().hipStreamDestroy(st) == 0


# ---- every texture index of a scene with sixteen textures of odd shapes
TEXTURE_PATHS = {
    "few": ("h8", None),                       # the few-sphere kernel (LDS image with the cull rectangles)
    "many": ("lcg64", 1),                      # the many-sphere kernel, shadow grid and bounce table, 1x1 samples
    "ss2": ("h8", 2),                          # 2x2 supersampling
    "strict": ("h8", "strict"),                # a strict-kernel scene throughout (a negative checker frequency on another sphere)
}


@pytest.mark.parametrize("path", list(TEXTURE_PATHS))
def test_a_sphere_restyled_through_every_texture_index(tlib, path):
    name, mode = TEXTURE_PATHS[path]
    w, h = 96, 64
    s0 = tu.with_textures(load(name))
    if mode in (1, 2):
        s0["supersample"] = mode
    if mode == "strict":
        r_checker_negative(s0)
    i = small(s0, 1 if mode == "strict" else 0)
    r = rt_host.Renderer(rt_host.flatten_scene(s0), 0, tlib)
    try:
        check_generation(tlib, r, s0, w, h, (path, "upload"))
        cur = s0
        for k in list(range(tu.MAX_TEXTURES)) + [0]:
            cur = tu.textured(cur, {i: k})
            r.set_objects(cur["objects"][i:i + 1], i)
            check_generation(tlib, r, cur, w, h, (path, "texture", k), tables=k in (0, 3, 4, 15))
    finally:
        r.close()


@pytest.mark.parametrize("rule", ["flag_tol", "unit_weights"])
def test_stale_mark_rules_show_in_the_exact_sample_count(tlib, rule):
    """A probe sphere whose checker coordinate u * 1e-8 always lies within 2^-20 of 0, so that every hit on it meets the precise
    boundary test: the samples it marks depend on flag_tol (a finer checker elsewhere widens the band) and, for a probe of tiny
    weight, on the mark-weight rule (a colour above 1 elsewhere turns it off).  The restyled scene's exact-sample count must be the
    fresh upload's, and must differ from the count before the restyle - else the probe saw nothing."""
    w, h = W, H
    s0 = load("default14")
    p = small(s0, 0)
    checker(s0["objects"][p]["mtl"], 1e-8, 0.0)
    if rule == "unit_weights":
        s0["objects"][p]["mtl"]["albedo"] = [0.001, 0.0005, 0.0, 0.0, 0.0]
    s1 = copy.deepcopy(s0)
    q = small(s0, 1)
    if rule == "flag_tol":
        checker(s1["objects"][q]["mtl"], 60000.0, 3.0)
    else:
        s1["objects"][q]["mtl"]["color"] = [1.5, 0.25, 0.5]
    r = rt_host.Renderer(rt_host.flatten_scene(s0), 0, tlib)
    try:
        counts = []
        for sc in (s0, s1, s0, s1):
            if len(counts):
                r.set_objects(sc["objects"][q:q + 1], q)
            _, n = render_with_stats(tlib, r, w, h, FAST)
            f = rt_host.Renderer(rt_host.flatten_scene(sc), 0, tlib)
            try:
                _, nf = render_with_stats(tlib, f, w, h, FAST)
            finally:
                f.close()
            assert n == nf, (rule, len(counts), n, nf)
            counts.append(n)
        assert counts[0] != counts[1] and counts[0] == counts[2] and counts[1] == counts[3], (rule, counts)
    finally:
        r.close()
