"""Texel edits of a resident scene on the GPU (include/rt_hip.h: rt_scene_set_texels, rt_scene_set_texels_device).  The yardstick is a
fresh upload of the scene whose texels were edited in numpy (texels_util.edited / with_texels): the resident texel bytes (the test
build's rt_test_scene_texels: from the first texel to the end of the blob, so neighbouring textures and the padding between them are
compared too) and every frame, byte for byte, with the product and the strict kernel; one frame per scene is also held to the C
restatement (objects_util.near_oracle, 1 LSB).  The order of edits and launches is the contract: nothing here waits on the host
between an edit and the launches around it."""
import ctypes as C
import functools

import numpy as np
import pytest

import nodes_util as nu
import rt_host
from lights_util import move_lights, set_lights
from objects_util import FAST, PARTS, STRICT, Frames, fresh, near_oracle, set_objects, state, tlib  # noqa: F401
from texels_util import INVALID, OK, STATE, bind, edited, rows_of, scene_texels, texel_bytes, texture, with_texels
from texture_util import H8_SPHERES, ORACLE_SCENES, oracle_scene, texels, textured, textures

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib(tlib):
    return bind(tlib)


def drain():
    assert nu.hip().hipDeviceSynchronize() == 0


def read_frames(lib, bufs, n):
    drain()
    out = []
    for d in bufs:
        host = C.create_string_buffer(n)
        assert lib.rt_copy_to_host(0, host, d, n) == 0, lib.rt_last_error()
        out.append(host.raw)
        lib.rt_free_device(0, d)
    return out


def whole(r, scene, stream=None, only=None):
    """Every texture of `scene` (or those in `only`) into the resident scene, host form."""
    for k, t in enumerate(scene["textures"]):
        if only is None or k in only:
            r.set_texels(k, t["texels"], stream=stream)


# ------------------------------------------------------------------ 1. whole textures
@pytest.mark.parametrize("name", [x[0] for x in ORACLE_SCENES])
def test_whole_textures_replaced_leave_a_fresh_upload(lib, name):
    s1, w, h = oracle_scene(name)                              # the seed-1 textures
    s2 = dict(s1, textures=textures(2))
    r = rt_host.Renderer(rt_host.flatten_scene(s2), 0, lib)
    f = rt_host.Renderer(rt_host.flatten_scene(s1), 0, lib)
    try:
        fr = Frames(lib, w, h, (h, 0, 1, 1))
        fr.render(r, FAST)                                     # issued before the edit: the old texels
        whole(r, s1)
        fr.render(r, FAST)
        fr.render(r, STRICT)
        old, fast, strict = fr.read()
        assert scene_texels(lib, r) == scene_texels(lib, f)
        assert scene_texels(lib, r) == texel_bytes(s1)
    finally:
        r.close()
        f.close()
    assert old == fresh(lib, s2, w, h) and old != fast, name
    assert fast == fresh(lib, s1, w, h, flags=FAST), name
    assert strict == fresh(lib, s1, w, h, flags=STRICT), name
    assert near_oracle(fast, s1, w, h), name


# ------------------------------------------------------------------ 2. rectangles
RECTS = [((257, 129), (0, 0, 1, 1)), ((257, 129), (256, 128, 1, 1)), ((257, 129), (0, 5, 257, 1)), ((257, 129), (3, 0, 1, 129)),
         ((257, 129), (100, 60, 57, 9)),
         ((16384, 2), (16383, 1, 1, 1)), ((16384, 2), (0, 0, 16384, 2)),
         ((2, 16384), (1, 16383, 1, 1)),
         ((3, 7), (0, 0, 3, 7)), ((3, 7), (1, 3, 1, 1)),
         ((5, 3), (0, 0, 5, 3)), ((5, 3), (2, 1, 1, 1))]


@pytest.mark.parametrize("mode", ["host", "host_pitch", "device", "device_pitch", "device_unaligned"])
def test_rectangles_write_their_texels_and_nothing_else(lib, mode):
    cur, _, _ = oracle_scene("h8_tex_a")
    r = rt_host.Renderer(rt_host.flatten_scene(cur), 0, lib)
    try:
        for i, (shape, (x, y, w, h)) in enumerate(RECTS):
            k, seed = texture(shape), 100 + i
            pitch = 4 * w + 20 if mode.endswith("_pitch") else 0        # (a multiple of 4 and of nothing larger)
            src = rows_of(w, h, seed, pitch)
            if mode.startswith("host"):
                r.set_texels(k, src, x, y, w, h, pitch)
            else:
                shift = 4 if mode == "device_unaligned" else 0          # 4-byte aligned and not 16-byte aligned
                framed = np.full(shift + len(src) + 12, 0xEE, np.uint8)
                framed[shift:shift + len(src)] = np.frombuffer(src, np.uint8)
                d = nu.Dev(lib, framed.nbytes, framed)
                assert d.ptr % 16 == 0
                r.set_texels_device(k, d.ptr + shift, x, y, w, h, pitch)
            cur = edited(cur, k, x, y, w, h, seed)
            assert scene_texels(lib, r) == texel_bytes(cur), (mode, shape, (x, y, w, h))      # (drains: the source may go)
            if not mode.startswith("host"):
                d.close()
    finally:
        r.close()


# ------------------------------------------------------------------ 3. order without a host wait
ORDER_SCENE = "h8_tex_a"
DRAWN = sorted(set(next(x for x in ORACLE_SCENES if x[0] == ORDER_SCENE)[1]))


@functools.lru_cache(maxsize=None)
def order_state(k):
    """State k of the order tests: the scene with the textures it draws taken from seed 2 + k."""
    s, _, _ = oracle_scene(ORDER_SCENE)
    new = textures(2 + k)
    for t in DRAWN:
        s = with_texels(s, t, new[t]["texels"])
    return s


_order_frames = {}


def order_frame(lib, k, flags):
    if (k, flags) not in _order_frames:
        _, w, h = oracle_scene(ORDER_SCENE)
        _order_frames[(k, flags)] = fresh(lib, order_state(k), w, h, flags=flags)
    return _order_frames[(k, flags)]


@pytest.mark.parametrize("plan,flags", [("one stream", FAST), ("one stream", STRICT), ("edits on a second stream", FAST),
                                        ("renders on two streams", FAST)])
def test_frames_and_edits_keep_the_order_of_the_calls(lib, plan, flags):
    _, w, h = oracle_scene(ORDER_SCENE)
    n = w * h * 4
    streams = [C.c_void_p(), C.c_void_p()]
    for s in streams:
        assert nu.hip().hipStreamCreate(C.byref(s)) == 0
    a, b = streams[0].value, streams[1].value
    render_on, edit_on = {"one stream": ([None], None), "edits on a second stream": ([a], b), "renders on two streams": ([a, b], None)}[plan]
    r = rt_host.Renderer(rt_host.flatten_scene(order_state(0)), 0, lib)
    try:
        bufs = []
        for k in range(5):                                     # four rounds of render; set_texels, and the frame of the last edit
            d = lib.rt_alloc_device(0, n)
            assert d, lib.rt_last_error()
            bufs.append(d)
            r.render_tiles(w, h, d, None, stream=render_on[k % len(render_on)], flags=flags)
            if k < 4:
                whole(r, order_state(k + 1), stream=edit_on, only=DRAWN)
        got = read_frames(lib, bufs, n)
        assert scene_texels(lib, r) == texel_bytes(order_state(4))
    finally:
        r.close()
        for s in streams:
            assert nu.hip().hipStreamDestroy(s) == 0
    assert len(set(got)) == 5
    for k in range(5):
        assert got[k] == order_frame(lib, k, flags), (plan, k)


# ------------------------------------------------------------------ 4. rendering into a texture
SCREEN_LIGHT = (50.0, 35.0, 65.0, 20.0)


def screen_scene(window):
    """h8 with a 64x32 and a 31x17 texture, each drawn by two spheres, and one of them by the sky as well (ambient 1: the texel is the
    pixel): a 64x32 frame of it is a texture of its own, and what the texture held shows all over the next frame."""
    s = rt_host.load_scene("h8")
    s["textures"] = [{"width": 64, "height": 32, "texels": texels(64, 32, 7)}, {"width": 31, "height": 17, "texels": texels(31, 17, 8)}]
    sky = next(i for i, o in enumerate(s["objects"]) if o["r2"] == 25000000.0)
    return textured(s, {H8_SPHERES[0]: 0, H8_SPHERES[1]: 1, sky: 1 if window else 0})


@pytest.mark.parametrize("flags", [FAST, STRICT])
@pytest.mark.parametrize("window", [False, True])
def test_a_frame_becomes_a_texture_without_leaving_the_gpu(lib, flags, window):
    """The light's intensity changes with every round (host state: no launch, no wait), so that the feedback does not settle: a frame
    drawn with the texture of the round before the right one is another frame (thousands of bytes, by the C restatement)."""
    w, h, n = 64, 32, 64 * 32 * 4
    s0 = screen_scene(window)
    r = rt_host.Renderer(rt_host.flatten_scene(s0), 0, lib)
    try:
        bufs = []
        for k in range(4):                                     # three rounds of render; set_texels_device, and one more frame
            d = lib.rt_alloc_device(0, n)
            assert d, lib.rt_last_error()
            bufs.append(d)
            r.set_light_intensity(SCREEN_LIGHT[k])
            r.render_tiles(w, h, d, None, flags=flags)
            if k < 3 and not window:
                r.set_texels_device(0, d, 0, 0, 64, 32)
            elif k < 3:
                r.set_texels_device(1, d + (3 * w + 7) * 4, 0, 0, 31, 17, pitch=4 * w)      # the window at (7, 3), the frame's pitch: 256
        got = read_frames(lib, bufs, n)
    finally:
        r.close()
    assert len(set(got)) == 4
    # the host loop: a fresh upload per round, the previous frame (or its window) as the texture
    sc = s0
    for k in range(4):
        sc = dict(sc, light_intensity=SCREEN_LIGHT[k])
        want = fresh(lib, sc, w, h, flags=flags)
        assert got[k] == want, (window, k)
        if window:
            sc = with_texels(sc, 1, np.frombuffer(want, np.uint8).reshape(h, w, 4)[3:20, 7:38].tobytes())
        else:
            sc = with_texels(sc, 0, want)


# ------------------------------------------------------------------ 5. every reader
def hits_and_picks(lib, r, w, h):
    n = w * h
    di, dd = lib.rt_alloc_device(0, n * 4), lib.rt_alloc_device(0, n * 8)
    r.render_hits(w, h, di, dd, None)
    hi, hd = C.create_string_buffer(n * 4), C.create_string_buffer(n * 8)
    assert lib.rt_copy_to_host(0, hi, di, n * 4) == 0 and lib.rt_copy_to_host(0, hd, dd, n * 8) == 0
    lib.rt_free_device(0, di)
    lib.rt_free_device(0, dd)
    return hi.raw, hd.raw, r.pick(w, h, [(w // 2, h // 2), (5, h - 3), (w - 2, 1)])


def test_rays_nodes_hits_picks_and_batches_follow_an_edit(lib):
    from test_gpu_rays import DeviceRays
    s1, w, h = oracle_scene("h8_tex_c")
    s2 = dict(s1, textures=textures(2))
    rays = rt_host.primary_rays(w, h, s1)
    r = rt_host.Renderer(rt_host.flatten_scene(s2), 0, lib)
    f = rt_host.Renderer(rt_host.flatten_scene(s1), 0, lib)
    try:
        nodes_old = nu.shade(lib, r, rays)
        geometry_old = hits_and_picks(lib, r, w, h)
        whole(r, s1)
        dr = DeviceRays(lib, rays, want=("rgba",))
        dr.run(r)
        assert dr.read("rgba").tobytes() == fresh(lib, s1, w, h, flags=STRICT)      # (the list of a frame's primary rays is its strict frame)
        dr.close()
        nodes = nu.shade(lib, r, rays)
        assert nodes.tobytes() == nu.shade(lib, f, rays).tobytes()                  # `sample` included
        assert (nodes["sample"] != nodes_old["sample"]).any()
        assert hits_and_picks(lib, r, w, h) == geometry_old                         # what is hit does not depend on a texel
        assert geometry_old == hits_and_picks(lib, f, w, h)
        fr = Frames(lib, w, h, (h, 0, 1, 1), 2)
        fr.render(r)
        assert fr.read()[0] == fresh(lib, s1, w, h, n_frames=2)
    finally:
        r.close()
        f.close()


# ------------------------------------------------------------------ 6. between other edits
def test_texels_survive_camera_object_restyle_and_light_moves(lib):
    import soak_gpu_parity as soak
    from test_gpu_objects import edit
    cur, w, h = oracle_scene("h8_tex_a")
    r = rt_host.Renderer(rt_host.flatten_scene(cur), 0, lib)
    frames, want = Frames(lib, w, h, (h, 0, 1, 1)), []

    def step(what):
        f = rt_host.Renderer(rt_host.flatten_scene(cur), 0, lib)
        try:
            got, fresh_state = state(lib, r), state(lib, f)
            for part in PARTS:
                assert got[part] == fresh_state[part], (what, part)
            assert scene_texels(lib, r) == scene_texels(lib, f), what
        finally:
            f.close()
        frames.render(r)
        want.append(cur)

    try:
        frames.render(r)                                       # a launch table in use: the moves rebuild it
        want.append(cur)
        k = texture((1, 9))
        cur = edited(cur, k, 0, 0, 1, 9, 61)
        r.set_texels(k, rows_of(1, 9, 61))
        step("texels")
        c, z = cur["camera"]["origin"], cur["camera"]["axisZ"]
        cam = soak.look_at([c[0] + 0.25, c[1] + 0.125, c[2] - 0.25], [c[0] + z[0], c[1] + z[1], c[2] + z[2]], [0.0, 1.0, 0.0])
        cur = dict(cur, camera=cam)
        r.set_camera(cam)
        step("camera")
        cur, a, b = edit(cur, 62)                              # (a mirror turns refractive: another kernel variant)
        set_objects(r, cur, a, b)
        step("objects")
        k = texture((257, 129))
        cur = edited(cur, k, 100, 60, 57, 9, 63)
        r.set_texels(k, rows_of(57, 9, 63), 100, 60, 57, 9)
        k = texture((3, 7))
        cur = edited(cur, k, 0, 0, 3, 7, 64)
        r.set_texels(k, rows_of(3, 7, 64))
        step("texels again")
        i = H8_SPHERES[1]
        cur = textured(cur, {i: texture((2, 2))})              # a sphere takes a texture no sphere drew
        set_objects(r, cur, i, i + 1)
        step("restyle")
        cur = move_lights(cur, 65)
        set_lights(r, cur)
        step("lights")
        got = frames.read()
    finally:
        r.close()
    assert len(got) == len(want) == 7
    for j, sc in enumerate(want):
        assert got[j] == fresh(lib, sc, w, h), j


# ------------------------------------------------------------------ 7. refusals
def test_bad_edits_are_refused_and_change_nothing(lib):
    s0, w, h = oracle_scene("h8_tex_a")
    r = rt_host.Renderer(rt_host.flatten_scene(s0), 0, lib)
    bare = rt_host.Renderer(rt_host.flatten_scene(rt_host.load_scene("cfg1")), 0, lib)        # a scene without textures
    src = C.create_string_buffer(rows_of(8, 8, 71))
    dev = nu.Dev(lib, 256, np.frombuffer(rows_of(8, 8, 71), np.uint8))
    k = texture((257, 129))
    try:
        fr = Frames(lib, w, h, (h, 0, 1, 1))
        fr.render(r)
        texels0 = scene_texels(lib, r)
        for fn, p in ((lib.rt_scene_set_texels, C.addressof(src)), (lib.rt_scene_set_texels_device, dev.ptr)):
            assert fn(r.handle, k, 0, 0, 2, 2, None, 0, None) == INVALID                      # a NULL source
            assert fn(r.handle, 16, 0, 0, 1, 1, p, 0, None) == INVALID                        # texture >= n_textures
            assert fn(r.handle, 0xFFFFFFFF, 0, 0, 1, 1, p, 0, None) == INVALID
            assert fn(r.handle, k, 256, 0, 2, 1, p, 0, None) == INVALID                       # one texel beyond the right edge
            assert fn(r.handle, k, 0, 128, 1, 2, p, 0, None) == INVALID                       # ... the bottom edge
            assert fn(r.handle, k, 257, 0, 1, 1, p, 0, None) == INVALID
            assert fn(r.handle, k, 0xFFFFFFFF, 0, 2, 1, p, 0, None) == INVALID                # x + w wraps in 32 bits
            assert fn(r.handle, k, 0, 0xFFFFFFFF, 1, 2, p, 0, None) == INVALID
            assert fn(r.handle, k, 1, 0, 0xFFFFFFFF, 1, p, 0, None) == INVALID
            assert fn(r.handle, k, 0, 0, 4, 2, p, 12, None) == INVALID                        # pitch below 4 * w
            assert fn(r.handle, k, 0, 0, 2, 2, p, 10, None) == INVALID                        # pitch no multiple of 4
            assert fn(None, k, 0, 0, 2, 2, p, 0, None) == STATE                               # a NULL scene
            assert fn(bare.handle, 0, 0, 0, 1, 1, p, 0, None) == INVALID                      # no texture at all
            assert fn(r.handle, k, 0, 0, 0, 5, p, 0, None) == OK                              # nothing to store
            assert fn(r.handle, k, 257, 129, 0, 0, None, 0, None) == OK
        for off in (1, 2, 3):
            assert lib.rt_scene_set_texels_device(r.handle, k, 0, 0, 2, 2, dev.ptr + off, 0, None) == INVALID
        fr.render(r)
        assert scene_texels(lib, r) == texels0
        # a texture no sphere draws: the edit succeeds, its texels are stored, no frame changes
        assert k not in next(x for x in ORACLE_SCENES if x[0] == "h8_tex_a")[1]
        r.set_texels(k, rows_of(8, 8, 71), 9, 9, 8, 8)
        r.set_texels_device(k, dev.ptr, 40, 40, 8, 8)
        fr.render(r)
        a, b, c = fr.read()
        assert a == b == c
        assert scene_texels(lib, r) == texel_bytes(edited(edited(s0, k, 9, 9, 8, 8, 71), k, 40, 40, 8, 8, 71))
    finally:
        dev.close()
        r.close()
        bare.close()


# ------------------------------------------------------------------ 8. the host forms
def test_host_forms_edit_the_resident_scene_instead_of_uploading(lib):
    import soak_gpu_parity as soak
    s, w, h = oracle_scene("h8_tex_c")
    drawn = next(x for x in ORACLE_SCENES if x[0] == "h8_tex_c")[1]
    rt_host.render(w, h, s, lib=lib)
    uploads = lib.rt_test_upload_count()
    seen = set()
    for j in range(4):                                         # four successive pictures
        k = drawn[j]
        tw, th = s["textures"][k]["width"], s["textures"][k]["height"]
        s = edited(s, k, 0, th // 3, tw, th - th // 3, 80 + j)
        if j == 3:                                             # ... the last with a camera and a light change in the same call
            c, z = s["camera"]["origin"], s["camera"]["axisZ"]
            s = dict(move_lights(s, 84), camera=soak.look_at([c[0] + 0.25, c[1] + 0.125, c[2] - 0.25], [c[0] + z[0], c[1] + z[1], c[2] + z[2]], [0.0, 1.0, 0.0]))
        got, _ = rt_host.render(w, h, s, lib=lib)
        assert lib.rt_test_upload_count() == uploads, j
        assert got == fresh(lib, s, w, h), j
        seen.add(got)
        uploads = lib.rt_test_upload_count()                   # (the fresh upload of the yardstick)
    assert len(seen) == 4
    # ray lists and nodes of the host form share that resident scene
    k = drawn[0]
    s = edited(s, k, 0, 0, s["textures"][k]["width"], 1, 85)
    rays = rt_host.primary_rays(w, h, s)
    rgba = rt_host.trace_rays(s, rays, want=("rgba",), lib=lib)["rgba"]
    assert lib.rt_test_upload_count() == uploads
    assert rgba.tobytes() == fresh(lib, s, w, h, flags=STRICT)
    uploads = lib.rt_test_upload_count()
    s = edited(s, k, 0, 0, s["textures"][k]["width"], 1, 86)
    nodes = rt_host.shade_rays(s, rays, lib=lib)
    assert lib.rt_test_upload_count() == uploads
    f = rt_host.Renderer(rt_host.flatten_scene(s), 0, lib)
    try:
        assert nodes.tobytes() == nu.shade(lib, f, rays).tobytes()
    finally:
        f.close()
    # a texture of another size (7x5 -> 5x7: the same bytes, another descriptor) is one upload, and draws right
    uploads = lib.rt_test_upload_count()
    k = texture((7, 5))
    assert k in drawn
    s = dict(s, textures=list(s["textures"]))
    s["textures"][k] = {"width": 5, "height": 7, "texels": texels(5, 7, 87)}
    got, _ = rt_host.render(w, h, s, lib=lib)
    assert lib.rt_test_upload_count() == uploads + 1
    assert got == fresh(lib, s, w, h)
