"""Caller-supplied rays on the GPU (include/rt_hip.h: rt_scene_trace_rays_device, rt_trace_rays).  Arbitrary rays are held to the
unchanged C restatement through micro-cameras (tests/rays_util.py): rgba within 1 LSB per channel - the project's parity rule; the
differing fraction is printed and recorded in docs/EVIDENCE.md - and the hit record bit for bit.  A frame's primary rays are held
to the library's own RT_FLAG_STRICT_FP frame byte for byte, and to the reference-made golden frames within 1 LSB."""
import base64
import ctypes as C
import json
import math
import os
import subprocess

import numpy as np
import pytest

import objects_util as obu
import oracle_util as ou
import rays_util as ru
import rt_host
from objects_util import tlib  # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu
ROOT = ou.ROOT
STRICT = rt_host.RT_FLAG_STRICT_FP
FRAMES = {f["name"]: f for f in ou.manifest()["frames"]}
CANARY = 0x5A
N_CAMERAS = 500


def _random_scene(seed, n, segs):
    from test_gpu_parity import random_scene
    return random_scene(seed, n, True, segs)


SCENES = {
    "h8": lambda: rt_host.load_scene("h8"),
    "default14": lambda: rt_host.load_scene("default14"),
    "cfg2": lambda: rt_host.load_scene("cfg2"),
    "lcg64": lambda: rt_host.load_scene("lcg64"),
    "random3": lambda: _random_scene(3, 10, 4),
    "random4": lambda: _random_scene(4, 20, 6),
}
_cases = {}


def case(name):
    """Per scene: 500 micro-cameras from a fixed seed, their 2000 rays, the restatement's bytes and root records, and ONE host-form
    call with all three outputs."""
    if name not in _cases:
        scene = SCENES[name]()
        cams = ru.draw_cameras(scene, N_CAMERAS, 1000 + len(name), outside_radius=5000.0 if name == "default14" else None)
        oracle = ru.MicroOracle(scene)
        rays = ru.micro_rays(cams, oracle.fov)
        rgba, roots = oracle.expected(cams)
        got = rt_host.trace_rays(scene, rays, want=("rgb", "rgba", "hits"))
        _cases[name] = {"scene": scene, "cams": cams, "oracle": oracle, "rays": rays, "rgba": rgba, "roots": roots, "got": got}
    return _cases[name]


@pytest.fixture(scope="module")
def lib(built):
    lib = rt_host.load_library()
    assert lib.rt_init(1) == 0, lib.rt_last_error()
    return lib


class DeviceRays:
    """A ray list in device memory and canary-framed device outputs for Renderer.trace_rays."""
    PAD = 256

    def __init__(self, lib, rays, want=("rgb", "rgba", "hits")):
        self.lib, self.n = lib, len(rays)
        src = np.ascontiguousarray(rays, np.float64)
        self.d_rays = lib.rt_alloc_device(0, src.nbytes)
        assert self.d_rays, lib.rt_last_error()
        hip = C.CDLL("libamdhip64.so")                     # (the ABI has no upload helper: hosts hand over memory they filled themselves)
        assert hip.hipMemcpy(C.c_void_p(self.d_rays), src.ctypes.data_as(C.c_void_p), C.c_size_t(src.nbytes), 1) == 0
        self.each = {"rgb": 24, "rgba": 4, "hits": 80}
        self.p = {}
        for k in want:
            nbytes = self.n * self.each[k] + 2 * self.PAD
            self.p[k] = lib.rt_alloc_device(0, nbytes)
            assert self.p[k], lib.rt_last_error()
            assert lib.rt_memset_device(0, self.p[k], CANARY, nbytes) == 0

    def ptr(self, k):
        return self.p[k] + self.PAD if k in self.p else 0

    def run(self, r, segs=0, want_stats=False):
        return r.trace_rays(self.n, self.d_rays, self.ptr("rgb"), self.ptr("rgba"), self.ptr("hits"), segs=segs, want_stats=want_stats)

    def read(self, k):
        """-> the output (canaries checked)."""
        nbytes = self.n * self.each[k] + 2 * self.PAD
        raw = np.empty(nbytes, np.uint8)
        assert self.lib.rt_copy_to_host(0, raw.ctypes.data, self.p[k], nbytes) == 0
        assert (raw[:self.PAD] == CANARY).all() and (raw[-self.PAD:] == CANARY).all(), k
        body = raw[self.PAD:-self.PAD]
        if k == "rgb":
            return body.view(np.float64).reshape(self.n, 3).copy()
        if k == "rgba":
            return body.reshape(self.n, 4).copy()
        return body.reshape(self.n, 80).copy()

    def close(self):
        for p in list(self.p.values()) + [self.d_rays]:
            self.lib.rt_free_device(0, p)
        self.p = {}


class DeviceFrame:
    """A w x h RGBA8 frame in device memory."""

    def __init__(self, lib, w, h):
        self.lib, self.n = lib, w * h * 4
        self.p = lib.rt_alloc_device(0, self.n)
        assert self.p, lib.rt_last_error()

    def data_ptr(self):
        return self.p

    def host(self):
        out = np.empty(self.n, np.uint8)
        assert self.lib.rt_copy_to_host(0, out.ctypes.data, self.p, self.n) == 0
        return out

    def close(self):
        self.lib.rt_free_device(0, self.p)


def hit_bytes(hits):
    """host-form hit dicts -> (n, 80) uint8 rt_hit records."""
    recs = (rt_host.RtHit * len(hits))()
    for r, h in zip(recs, hits):
        if h is None:
            r.object, r.inside, r.t = -1, 0, math.inf
        else:
            r.object, r.inside, r.t, r.u, r.v = h["object"], int(h["inside"]), h["t"], h["u"], h["v"]
            r.point[:] = h["point"]
            r.normal[:] = h["normal"]
    return np.frombuffer(bytes(recs), np.uint8).reshape(len(hits), 80).copy()


# ------------------------------------------------------------------ 6. arbitrary rays against the restatement
@pytest.mark.parametrize("name", list(SCENES))
def test_arbitrary_rays_match_the_restatement(lib, name):
    c = case(name)
    scene, rays, roots, objs = c["scene"], c["rays"], c["roots"], c["scene"]["objects"]
    assert len(rays) == 4 * N_CAMERAS
    # the inputs are what they claim to be: the restatement traced these very rays ...
    assert rays[:, 3:6].tobytes() == np.ascontiguousarray(roots[:, 9:12]).tobytes()
    assert rays[:, 0:3].tobytes() == np.ascontiguousarray(roots[:, 19:22]).tobytes()
    # ... in all eight octants, from inside spheres, and (default14) from outside the skybox
    assert len({tuple(bool(x) for x in (r[3:6] > 0)) for r in rays}) == 8
    codes = roots[:, 1].astype(int)
    small_in = [c_ >> 1 for c_ in codes if c_ >= 0 and c_ & 1 and objs[c_ >> 1]["r2"] < ru.SMALL_R2]
    assert any(objs[i]["mtl"]["albedo"][4] == 0 for i in small_in), "no origin inside an opaque sphere"
    if name in ("default14", "random3", "random4"):
        assert any(objs[i]["mtl"]["albedo"][4] > 0 for i in small_in), "no origin inside a refracting sphere"
    if name == "default14":
        far = np.linalg.norm(rays[:, 0:3], axis=1) > 5000.0
        assert far.sum() >= 100 and any(c_ >= 0 and not (c_ & 1) and objs[c_ >> 1]["r2"] > 1e7 for c_ in codes[far])
    assert len({bytes(p) for p in c["rgba"]}) > 50                      # not all sky
    # colour: every ray, every channel
    got = c["got"]["rgba"].astype(np.int16)
    diff = np.abs(got - c["rgba"].astype(np.int16))
    print("RAYS %s: %d rays, %d of %d channels differ from the restatement (fraction %.3g), max %d LSB"
          % (name, len(rays), int((diff != 0).sum()), diff.size, float((diff != 0).mean()), int(diff.max())))
    assert diff.shape == (4 * N_CAMERAS, 4) and diff.max() <= 1, (name, int(diff.max()), np.argwhere(diff > 1)[:8].tolist())
    # hit records: every ray
    bad = [j for j in range(len(rays)) if not ru.hits_equal(c["got"]["hits"][j], c["oracle"].hit_of(roots[j]))]
    assert not bad, (name, bad[:8], c["got"]["hits"][bad[0]], c["oracle"].hit_of(roots[bad[0]]))


# ------------------------------------------------------------------ 7. a frame's rays are the frame
@pytest.mark.parametrize("name,w,h", [("h8", 200, 120), ("default14", 131, 77), ("cfg2", 160, 90), ("lcg64_ss1", 96, 50), ("default14_stars", 96, 54)])
def test_a_frames_rays_are_the_strict_frame(lib, name, w, h):
    scene = rt_host.load_scene(name)
    for seed in ([None, 7] if name == "default14_stars" else [None]):
        if seed is not None:
            scene = dict(scene, starsSeed=seed)
        frame, _ = rt_host.render(w, h, scene, flags=STRICT, lib=lib)
        got = rt_host.trace_rays(scene, rt_host.primary_rays(w, h, scene), want=("rgba",))["rgba"]
        assert got.tobytes() == frame, (name, seed, int((np.frombuffer(frame, np.uint8) != got.reshape(-1)).sum()))
    if name == "default14_stars":
        plain = rt_host.render(w, h, dict(scene, starsSeed=0), flags=STRICT, lib=lib)[0]
        assert plain != frame                                            # the seed shows


def test_the_stars_seed_of_a_resident_scene_reaches_its_rays(lib):
    """Renderer.set_stars_seed, then rays and the strict frame: the same sky."""
    w, h = 96, 54
    scene = rt_host.load_scene("default14_stars")
    r = rt_host.Renderer(scene, 0, lib)
    d = DeviceRays(lib, rt_host.primary_rays(w, h, scene), want=("rgba",))
    frame = DeviceFrame(lib, w, h)
    try:
        seen = []
        for seed in (0, 7):
            r.set_stars_seed(seed)
            r.render_tiles(w, h, frame.data_ptr(), flags=STRICT, want_stats=True)
            d.run(r, want_stats=True)
            assert d.read("rgba").tobytes() == frame.host().tobytes(), seed
            seen.append(d.read("rgba").tobytes())
        assert seen[0] != seen[1]
    finally:
        d.close()
        frame.close()
        r.close()


@pytest.mark.parametrize("golden", ["default14_160x90", "h8_240x135", "cfg2_240x135", "lcg64_ss1_192x192"])
def test_a_frames_rays_are_within_1_lsb_of_the_reference(lib, golden):
    f = FRAMES[golden]
    scene = rt_host.load_scene(f["scene"])
    got = rt_host.trace_rays(scene, rt_host.primary_rays(f["w"], f["h"], scene), want=("rgba",))["rgba"]
    want = ou.golden_frame(f)
    assert got.size == want.size
    worst, frac = ou.max_lsb(got.tobytes(), want)
    print("RAYS golden %s: max %d LSB, fraction %.3g" % (golden, worst, frac))
    assert worst <= 1, (golden, worst)


# ------------------------------------------------------------------ 8. rgb and rgba of one call
@pytest.mark.parametrize("name", list(SCENES))
def test_rgb_and_rgba_are_consistent(lib, name):
    c = case(name)
    assert np.array_equal(c["got"]["rgba"], ru.store_rule(c["got"]["rgb"]))
    alone = rt_host.trace_rays(c["scene"], c["rays"], want=("rgb",))["rgb"]
    assert alone.tobytes() == c["got"]["rgb"].tobytes()


# ------------------------------------------------------------------ 9. segs
def test_segs(lib):
    c = case("default14")
    scene, rays = c["scene"], c["rays"]
    own = rt_host.trace_rays(scene, rays, segs=scene["segs"], want=("rgb", "hits"))
    assert own["rgb"].tobytes() == c["got"]["rgb"].tobytes()           # segs = 0 is the scene's depth
    flat = ru.MicroOracle(scene, segs=1)
    want, _ = flat.expected(c["cams"])
    one = rt_host.trace_rays(scene, rays, segs=1, want=("rgba", "hits"))
    diff = np.abs(one["rgba"].astype(np.int16) - want.astype(np.int16))
    print("RAYS default14 segs=1: %d of %d channels differ, max %d LSB" % (int((diff != 0).sum()), diff.size, int(diff.max())))
    assert diff.max() <= 1
    assert (one["rgba"] != c["got"]["rgba"]).any()                     # the depth shows in the colours ...
    assert hit_bytes(one["hits"]).tobytes() == hit_bytes(own["hits"]).tobytes() == hit_bytes(c["got"]["hits"]).tobytes()   # ... not in the hits
    deep = rt_host.trace_rays(scene, rays[:64], segs=16, want=("rgba",))["rgba"]
    assert deep.shape == (64, 4)


# ------------------------------------------------------------------ 10. resident-scene interplay
def test_resident_scene_interplay(tlib):  # noqa: F811
    c = case("default14")
    scene = json.loads(json.dumps({k: v for k, v in c["scene"].items() if k != "textures"}))
    scene["textures"] = c["scene"]["textures"]
    rays, w, h = c["rays"], 96, 64
    r = rt_host.Renderer(scene, 0, tlib)
    d = DeviceRays(tlib, rays)
    only = DeviceRays(tlib, rays, want=("rgba",))
    frame = DeviceFrame(tlib, w, h)
    try:
        uploads = tlib.rt_test_upload_count()
        r.render_tiles(w, h, frame.data_ptr(), want_stats=True)
        before = frame.host().copy()
        st = d.run(r, want_stats=True)
        assert st.pixels == len(rays) and st.kernel_ms > 0
        first = {k: d.read(k) for k in ("rgb", "rgba", "hits")}
        assert first["rgba"].tobytes() == c["got"]["rgba"].tobytes() and first["rgb"].tobytes() == c["got"]["rgb"].tobytes()
        assert first["hits"].tobytes() == hit_bytes(c["got"]["hits"]).tobytes()
        # a call with rgb and hits NULL writes rgba alone - the other buffers of the first call keep their bytes - and every buffer
        # is still framed by its canaries (read())
        only.run(r)
        assert only.read("rgba").tobytes() == first["rgba"].tobytes()
        assert all(d.read(k).tobytes() == first[k].tobytes() for k in first)
        # a colour frame after the rays is the frame before them
        r.render_tiles(w, h, frame.data_ptr(), want_stats=True)
        assert np.array_equal(frame.host(), before)
        # a camera move changes nothing in the ray results
        cam = dict(scene["camera"], origin=[1.0, 2.0, 9.0])
        r.set_camera(cam)
        d.run(r, want_stats=True)
        assert all(d.read(k).tobytes() == first[k].tobytes() for k in first)
        # an orbit step of one sphere: the restatement's answer for the moved spheres, and no upload
        i = next(i for i, o in enumerate(scene["objects"]) if o["r2"] < 1e4 and o["mtl"]["albedo"][4] > 0)
        c0 = list(scene["objects"][i]["origin"])
        scene["objects"][i]["origin"] = [c0[0] + 0.5 * math.cos(0.4), c0[1], c0[2] + 0.5 * math.sin(0.4)]
        obu.set_objects(r, scene, i, i + 1)
        d.run(r, want_stats=True)
        assert tlib.rt_test_upload_count() == uploads + 0
        moved = ru.MicroOracle(scene)
        want, roots = moved.expected(c["cams"])
        got = d.read("rgba")
        diff = np.abs(got.astype(np.int16) - want.astype(np.int16))
        print("RAYS default14 after an orbit step: %d of %d channels differ, max %d LSB" % (int((diff != 0).sum()), diff.size, int(diff.max())))
        assert diff.max() <= 1 and (got != first["rgba"]).any()
        recs = d.read("hits")
        want_hits = hit_bytes([moved.hit_of(q) for q in roots])
        assert recs.tobytes() == want_hits.tobytes()
    finally:
        d.close()
        only.close()
        frame.close()
        r.close()


# ------------------------------------------------------------------ 11. non-finite rays
def test_non_finite_rays_are_not_traced(lib):
    c = case("default14")
    rays = c["rays"][:200].copy()
    bad_at = {}
    j = 3
    for slot in range(6):
        for v in (math.nan, math.inf, -math.inf):
            rays[j, slot] = v
            bad_at[j] = (slot, v)
            j += 5
    got = rt_host.trace_rays(c["scene"], rays, want=("rgb", "rgba", "hits"))
    keep = np.array([k not in bad_at for k in range(len(rays))])
    for k in bad_at:
        assert np.isnan(got["rgb"][k]).all() and got["rgba"][k].tolist() == [0, 0, 0, 255] and got["hits"][k] is None, (k, bad_at[k])
    # the neighbours' results are those of the list without them (their indices - the stars sampler's pix - apart: no stars here)
    assert got["rgb"][keep].tobytes() == c["got"]["rgb"][:200][keep].tobytes()
    assert got["rgba"][keep].tobytes() == c["got"]["rgba"][:200][keep].tobytes()
    assert hit_bytes([h for h, k in zip(got["hits"], keep) if k]).tobytes() == hit_bytes([h for h, k in zip(c["got"]["hits"][:200], keep) if k]).tobytes()
    zero = rt_host.trace_rays(c["scene"], np.array([[0.0, 1.5, 10.0, 0.0, 0.0, 0.0]]), want=("rgb",))["rgb"]     # a zero direction is traced
    assert np.isfinite(zero).all()


# ------------------------------------------------------------------ 12. sizes
@pytest.mark.parametrize("n", [1, 63, 65])
def test_small_lists(lib, n):
    c = case("h8")
    r = rt_host.Renderer(c["scene"], 0, lib)
    d = DeviceRays(lib, c["rays"][:n])
    try:
        d.run(r)
        assert d.read("rgba").tobytes() == c["got"]["rgba"][:n].tobytes()
        assert d.read("rgb").tobytes() == c["got"]["rgb"][:n].tobytes()
        assert d.read("hits").tobytes() == hit_bytes(c["got"]["hits"][:n]).tobytes()
    finally:
        d.close()
        r.close()


def test_a_4k_frame_of_rays_and_the_host_forms_chunks(lib):
    w, h = 3840, 2160
    scene = rt_host.load_scene("h8")
    rays = rt_host.primary_rays(w, h, scene)
    r = rt_host.Renderer(scene, 0, lib)
    d = DeviceRays(lib, rays, want=("rgba",))
    frame = DeviceFrame(lib, w, h)
    try:
        r.render_tiles(w, h, frame.data_ptr(), flags=STRICT, want_stats=True)
        st = d.run(r, want_stats=True)
        assert st.pixels == w * h
        got = d.read("rgba")
        assert got.tobytes() == frame.host().tobytes()
    finally:
        d.close()
        frame.close()
        r.close()
    # the host form above one chunk (2^18 rays): the same bytes, and a stars scene keeps pix = i across chunks
    n = 3 * (1 << 18) + 1001
    host = rt_host.trace_rays(scene, rays[:n], want=("rgba",))["rgba"]
    assert host.tobytes() == got[:n].tobytes()
    stars = rt_host.load_scene("default14_stars")
    sw, sh = 1024, 600                                                  # 614 400 rays: three chunks
    sframe, _ = rt_host.render(sw, sh, stars, flags=STRICT, lib=lib)
    assert rt_host.trace_rays(stars, rt_host.primary_rays(sw, sh, stars), want=("rgba",))["rgba"].tobytes() == sframe


# ------------------------------------------------------------------ 13. Node and the bridge
@pytest.mark.skipif(ou.node_path() is None, reason="node not installed")
def test_node_and_bridge_agree_with_python(lib):
    c = case("default14")
    rays = c["rays"][:64]
    pkg = os.path.join(ROOT, "html5-canvas-raytracer_amd")
    out = subprocess.check_output([ou.node_path(), os.path.join(ROOT, "tests", "js_rays_check.js"), pkg, "default14",
                                   base64.b64encode(np.ascontiguousarray(rays).tobytes()).decode()], text=True, timeout=300)
    res = json.loads(out.strip().splitlines()[-1])
    assert res["rgba"] == c["got"]["rgba"][:64].reshape(-1).tolist()
    assert base64.b64decode(res["rgb"]) == c["got"]["rgb"][:64].tobytes()
    for j, h in enumerate(res["hits"]):
        want = c["got"]["hits"][j]
        assert (h is None) == (want is None), j
        if h:
            assert h["index"] == want["object"] and h["inside"] == want["inside"] and h["t"] == want["t"] and h["point"] == want["point"] and \
                h["normal"] == want["normal"] and h["u"] == want["u"] and h["v"] == want["v"], j
    # GET /ray for ray 0 (decimal round trip of binary64 is exact in both directions)
    b = res["bridge"]
    assert b["status"] == 200 and b["body"]["rgba"] == c["got"]["rgba"][0].tolist() and b["body"]["rgb"] == c["got"]["rgb"][0].tolist()
    want = c["got"]["hits"][0]
    assert (b["body"]["hit"] is None) == (want is None)
    if want:
        assert b["body"]["hit"]["index"] == want["object"] and b["body"]["hit"]["t"] == want["t"]
    assert res["bad"] == [400, 400, 404]
