"""Views on the GPU (include/rt_hip.h: rt_view): the generator kernel against the host probe, and the traces of a whole view against
paths that exist without it - the RT_FLAG_STRICT_FP frame for a REFERENCE view, rt_host.trace_rays of the probe's rays for the other
models.  Every comparison is byte for byte: the generator runs + - * / and sqrt without FMA contraction on the probe's own source, and
the trace is the launch of a caller's ray list, band by band."""
import ctypes as C
import math

import numpy as np
import pytest

import rt_host
import views_util as vu

pytestmark = pytest.mark.gpu
STRICT = rt_host.RT_FLAG_STRICT_FP
CANARY = 0x5A
PAD = 48                     # bytes before and behind a device buffer: one ray record
MODELS = [vu.REFERENCE, vu.PINHOLE, vu.ORTHO, vu.EQUIRECT]
FOV, SCALE = 52.0, 0.037
INVALID = -1


@pytest.fixture(scope="module")
def lib(built):
    lib = rt_host.load_library()
    assert lib.rt_init(1) == 0, lib.rt_last_error()
    return lib


@pytest.fixture(scope="module")
def hip():
    return C.CDLL("libamdhip64.so")       # (the ABI has no upload helper: hosts hand over memory they filled themselves)


class Dev:
    """nbytes of device memory framed by PAD canary bytes at each end."""

    def __init__(self, lib, nbytes):
        self.lib, self.n = lib, nbytes
        self.base = lib.rt_alloc_device(0, nbytes + 2 * PAD)
        assert self.base and self.base % 16 == 0, lib.rt_last_error()
        assert lib.rt_memset_device(0, self.base, CANARY, nbytes + 2 * PAD) == 0
        self.p = self.base + PAD

    def read(self, dtype=np.uint8):
        """-> the body (canaries checked)."""
        raw = np.empty(self.n + 2 * PAD, np.uint8)
        assert self.lib.rt_copy_to_host(0, raw.ctypes.data, self.base, raw.size) == 0
        assert (raw[:PAD] == CANARY).all() and (raw[-PAD:] == CANARY).all(), "written outside the buffer"
        return raw[PAD:-PAD].view(dtype).copy()

    def close(self):
        self.lib.rt_free_device(0, self.base)


def upload(lib, hip, a):
    a = np.ascontiguousarray(a)
    p = lib.rt_alloc_device(0, max(a.nbytes, 16))
    assert p and p % 16 == 0, lib.rt_last_error()
    assert hip.hipMemcpy(C.c_void_p(p), a.ctypes.data_as(C.c_void_p), C.c_size_t(a.nbytes), 1) == 0
    return p


class Views:
    """A host view and its device twin (an EQUIRECT view's tables uploaded) at one size."""

    def __init__(self, lib, hip, model, w, h, cam=None, fov=FOV, scale=SCALE):
        o, ax, ay, az = cam or vu.look_at(*vu.OBLIQUE)
        self.lib, self.ptrs = lib, []
        tables = rt_host.equirect_tables(w, h) if model == vu.EQUIRECT else None
        self.host = rt_host.view(model, o, ax, ay, az, fov, scale, tables=tables)
        if tables:
            self.ptrs = [upload(lib, hip, t) for t in tables]
        self.dev = rt_host.view(model, o, ax, ay, az, fov, scale, tables=tuple(self.ptrs) if tables else None)

    def close(self):
        for p in self.ptrs:
            self.lib.rt_free_device(0, p)


def hit_bytes(hits):
    """host-form hit dicts -> (n, 80) uint8 rt_hit records (a miss: object -1, t +Infinity, everything else 0)."""
    recs = (rt_host.RtHit * len(hits))()
    for r, h in zip(recs, hits):
        if h is None:
            r.object, r.inside, r.t = -1, 0, math.inf
        else:
            r.object, r.inside, r.t, r.u, r.v = h["object"], int(h["inside"]), h["t"], h["u"], h["v"]
            r.point[:] = h["point"]
            r.normal[:] = h["normal"]
    return np.frombuffer(bytes(recs), np.uint8).copy()


class Outputs:
    """Canary-framed rgb, rgba and hits of n rays, and a canary-framed workspace."""
    EACH = {"rgb": 24, "rgba": 4, "hits": 80}

    def __init__(self, lib, n, work_bytes):
        self.b = {k: Dev(lib, n * e) for k, e in self.EACH.items()}
        self.work = Dev(lib, work_bytes)
        self.work_bytes = work_bytes

    def trace(self, r, v, w, h, want=("rgb", "rgba", "hits"), **kw):
        p = {k: (self.b[k].p if k in want else 0) for k in self.EACH}
        return r.trace_view(v, w, h, p["rgb"], p["rgba"], p["hits"], self.work.p, self.work_bytes, **kw)

    def read(self, k):
        self.work.read()                     # (its canaries)
        return self.b[k].read()

    def close(self):
        for d in list(self.b.values()) + [self.work]:
            d.close()


# ------------------------------------------------------------------ the generator against the host probe
@pytest.mark.parametrize("model", MODELS)
def test_generated_rays_are_the_probes(lib, hip, model):
    r = rt_host.Renderer(rt_host.load_scene("h8"), 0, lib)
    try:
        for w, h, first, rows in [(w, h, 0, h) for w, h in vu.SIZES] + [vu.BAND]:
            v = Views(lib, hip, model, w, h)
            d = Dev(lib, rows * w * 48)
            try:
                r.view_rays(v.dev, w, h, d.p, first, rows)
                got = d.read(np.uint64)                                         # nothing is written outside rows * w records
                want = rt_host.view_rays(v.host, w, h, first, rows)
                assert (got == vu.bits(want).reshape(-1)).all(), (model, w, h, first, rows)
                assert (vu.bits(want) == vu.bits(vu.rays(model, w, h, list(v.host.origin), list(v.host.axis_x), list(v.host.axis_y),
                                                         list(v.host.axis_z), FOV, SCALE, *(getattr(v.host, "_tables", (None, None))),
                                                         first_row=first, rows=rows))).all()
            finally:
                d.close()
                v.close()
    finally:
        r.close()


@pytest.mark.parametrize("model", [vu.PINHOLE, vu.EQUIRECT])
def test_a_view_taller_than_one_launch(lib, hip, model):
    """70 000 rows of one pixel: the generator's grid holds 65 535 rows, so the launcher splits - the second launch's first row and
    its place in the list are what this holds."""
    w, h = 1, 70000
    r = rt_host.Renderer(rt_host.load_scene("h8"), 0, lib)
    v = Views(lib, hip, model, w, h)
    d = Dev(lib, w * h * 48)
    try:
        r.view_rays(v.dev, w, h, d.p)
        want = rt_host.view_rays(v.host, w, h)
        assert (d.read(np.uint64) == vu.bits(want).reshape(-1)).all()
        assert len({bytes(q) for q in want[65530:65540, 3:]}) == 10                 # the rows differ where the launches meet
    finally:
        d.close()
        v.close()
        r.close()


def test_generator_arguments(lib, hip):
    w, h = 8, 4
    v = Views(lib, hip, vu.PINHOLE, w, h)
    e = Views(lib, hip, vu.EQUIRECT, w, h)
    d = Dev(lib, w * h * 48)
    try:
        call = lambda view, first, rows, p: lib.rt_view_rays_device(0, C.byref(view), w, h, first, rows, C.c_void_p(p), None)
        assert call(v.dev, 0, h + 1, d.p) == INVALID and call(v.dev, 3, 2, d.p) == INVALID and "rows" in lib.rt_last_error().decode()
        assert call(v.dev, 0, h, 0) == INVALID and call(v.dev, 0, h, d.p + 8) == INVALID
        nul = rt_host.view(vu.EQUIRECT, (0, 0, 0), (1, 0, 0), (0, 1, 0), (0, 0, -1))
        assert call(nul, 0, h, d.p) == INVALID and "tables" in lib.rt_last_error().decode()
        assert call(v.dev, 2, 0, d.p) == 0                                          # rows == 0: RT_OK, nothing written
        assert (d.read() == CANARY).all()
        assert call(e.dev, 1, 2, d.p) == 0
        got = d.read(np.uint64)
        assert (got[:2 * w * 6] == vu.bits(rt_host.view_rays(e.host, w, h, 1, 2)).reshape(-1)).all()
        assert (got[2 * w * 6:].view(np.uint8) == CANARY).all()
    finally:
        d.close()
        v.close()
        e.close()


# ------------------------------------------------------------------ a REFERENCE view with the scene's camera is the strict frame
@pytest.mark.parametrize("name,w,h", [("default14_stars", 64, 48), ("h8", 96, 40)])
def test_a_reference_view_is_the_strict_frame(lib, hip, name, w, h):
    scene = rt_host.load_scene(name)
    assert scene.get("supersample", 1) == 1
    cam = scene["camera"]
    v = rt_host.view(vu.REFERENCE, cam["origin"], cam["axisX"], cam["axisY"], cam["axisZ"], scene["fovDeg"])
    r = rt_host.Renderer(scene, 0, lib)
    frame = Dev(lib, w * h * 4)
    pref, one_row = rt_host.view_work_bytes(w, h), 48 * w
    assert pref == 48 * w * h                                                        # (a small view: one band)
    outs = [Outputs(lib, w * h, pref), Outputs(lib, w * h, one_row), Outputs(lib, w * h, 5 * one_row + 47)]    # 1 band, h bands, bands of 5 rows and a rest
    try:
        seen = []
        for seed in ([None, 7] if name == "default14_stars" else [None]):
            if seed is not None:
                r.set_stars_seed(seed)
            r.render_tiles(w, h, frame.p, flags=STRICT, want_stats=True)
            want = frame.read().tobytes()
            for o in outs:
                st = o.trace(r, v, w, h, want_stats=True)
                assert st.pixels == w * h and st.kernel_ms > 0
                assert o.read("rgba").tobytes() == want, (name, seed, o.work_bytes)
            assert all(outs[0].read(k).tobytes() == o.read(k).tobytes() for o in outs[1:] for k in ("rgb", "hits"))
            seen.append(want)
        assert len(set(seen)) == len(seen)                                           # the seed shows
    finally:
        for o in outs:
            o.close()
        frame.close()
        r.close()


# ------------------------------------------------------------------ the other models against trace_rays of the probe's rays
_traced = {}


def traced(scene, name, model, w, h, cam, scale):
    """The probe's rays of the view through rt_host.trace_rays: computed once per case."""
    key = (name, model, w, h)
    if key not in _traced:
        o, ax, ay, az = cam
        tables = rt_host.equirect_tables(w, h) if model == vu.EQUIRECT else None
        hv = rt_host.view(model, o, ax, ay, az, FOV, scale, tables=tables)
        _traced[key] = rt_host.trace_rays(scene, rt_host.view_rays(hv, w, h), want=("rgb", "rgba", "hits"))
    return _traced[key]


CAMS = {vu.PINHOLE: (vu.look_at(*vu.OBLIQUE), SCALE),
        vu.ORTHO: (([0.0, 1.5, 10.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, -1.0]), 0.2),          # 8 x 4.8 world units around the reference's eye
        vu.EQUIRECT: (([0.0, 1.5, 4.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, -1.0]), SCALE)}


@pytest.mark.parametrize("model", [vu.PINHOLE, vu.ORTHO, vu.EQUIRECT])
def test_a_traced_view_is_trace_rays_of_its_rays(lib, hip, model):
    w, h = 40, 24
    scene = rt_host.load_scene("default14")
    cam, scale = CAMS[model]
    want = traced(scene, "default14", model, w, h, cam, scale)
    assert not np.isnan(want["rgb"]).any() and len({bytes(p) for p in want["rgba"]}) > 20       # a picture, not a constant
    r = rt_host.Renderer(scene, 0, lib)
    v = Views(lib, hip, model, w, h, cam, FOV, scale)
    o = Outputs(lib, w * h, 7 * 48 * w)                                                  # bands of 7 rows: 3 and a rest of 3
    try:
        o.trace(r, v.dev, w, h)
        assert o.read("rgb").tobytes() == want["rgb"].tobytes()
        assert o.read("rgba").tobytes() == want["rgba"].tobytes()
        assert o.read("hits").tobytes() == hit_bytes(want["hits"]).tobytes()
        # the host form: the same bytes
        got = rt_host.trace_view(scene, v.host, w, h, want=("rgb", "rgba", "hits"))
        assert got["rgb"].tobytes() == want["rgb"].tobytes() and got["rgba"].tobytes() == want["rgba"].tobytes()
        assert hit_bytes(got["hits"]).tobytes() == hit_bytes(want["hits"]).tobytes()
    finally:
        o.close()
        v.close()
        r.close()


def one_sphere_scene():
    s = rt_host.load_scene("h8")
    ball = next(o for o in s["objects"] if o["r2"] < 100)
    return dict(s, objects=[dict(ball, origin=[0.0, 1.5, 0.0])], lights=[], segs=1)


def test_the_host_form_chunks_whole_rows(lib, hip):
    """700 x 400 = 280 000 rays: more than one chunk of 2^18 (374 rows and a rest of 26).  One sphere, no lights: it takes no time."""
    w, h = 700, 400
    assert w * h > 1 << 18
    scene = one_sphere_scene()
    o_, ax, ay, az = vu.look_at([0.8, 1.9, 1.6], [0.0, 1.5, 0.0], [0.0, 1.0, 0.0])
    v = rt_host.view(vu.PINHOLE, o_, ax, ay, az, FOV)
    got = rt_host.trace_view(scene, v, w, h, want=("rgb", "rgba"))
    r = rt_host.Renderer(scene, 0, lib)
    o = Outputs(lib, w * h, rt_host.view_work_bytes(w, h))
    try:
        o.trace(r, v, w, h, want=("rgb", "rgba"))
        assert o.read("rgba").tobytes() == got["rgba"].tobytes() and o.read("rgb").tobytes() == got["rgb"].tobytes()
        assert (o.read("hits") == CANARY).all()                                      # not asked for, not touched
        rows = got["rgba"].reshape(h, w, 4)
        assert len({bytes(p) for p in rows[373].reshape(-1, 4)}) > 1 and (rows[373] != rows[374]).any()     # the sphere crosses the chunks' seam
    finally:
        o.close()
        r.close()


# ------------------------------------------------------------------ arguments of the device trace
def test_refused_calls_leave_the_scene_usable(lib, hip):
    w, h = 64, 48
    scene = rt_host.load_scene("default14_stars")
    cam = scene["camera"]
    v = rt_host.view(vu.REFERENCE, cam["origin"], cam["axisX"], cam["axisY"], cam["axisZ"], scene["fovDeg"])
    r = rt_host.Renderer(scene, 0, lib)
    frame = Dev(lib, w * h * 4)
    o = Outputs(lib, w * h, 48 * w * 8)
    try:
        def call(view=v, rgba=o.b["rgba"].p, work=o.work.p, work_bytes=o.work_bytes, segs=0, outs=True):
            out = rt_host.RtRayOutputs(None, rgba or None, None)
            return lib.rt_scene_trace_view_device(r.handle, C.byref(view), w, h, segs, C.byref(out) if outs else None, C.c_void_p(work), work_bytes, None, None)

        def refused(needle, **kw):
            assert call(**kw) == INVALID
            assert needle in lib.rt_last_error().decode(), lib.rt_last_error()

        refused("below one row", work_bytes=48 * w - 1)
        refused("workspace", work=0)
        refused("workspace", work=o.work.p + 8)
        refused("every output is NULL", rgba=0)
        refused("NULL outputs", outs=False)
        refused("misaligned output", rgba=o.b["rgba"].p + 2)
        refused("segs", segs=rt_host.RT_MAX_SEGS + 1)
        refused("tables", view=rt_host.view(vu.EQUIRECT, cam["origin"], cam["axisX"], cam["axisY"], cam["axisZ"]))
        bad = rt_host.view(vu.PINHOLE, cam["origin"], cam["axisX"], cam["axisY"], cam["axisZ"], 180.0)
        refused("fov_deg", view=bad)
        out = rt_host.RtRayOutputs(None, o.b["rgba"].p, None)
        assert lib.rt_scene_trace_view_device(None, C.byref(v), w, h, 0, C.byref(out), C.c_void_p(o.work.p), o.work_bytes, None, None) == -5
        assert lib.rt_view_rays_device(0, C.byref(v), w, h, h - 1, 2, C.c_void_p(o.work.p), None) == INVALID
        assert (o.read("rgba") == CANARY).all() and (o.work.read() == CANARY).all()    # nothing was launched
        # ... and a valid call still renders the right frame
        assert call() == 0
        r.render_tiles(w, h, frame.p, flags=STRICT, want_stats=True)
        assert o.read("rgba").tobytes() == frame.read().tobytes()
    finally:
        o.close()
        frame.close()
        r.close()


def test_a_view_sees_a_moved_sphere(lib, hip):
    """set_objects, then a view before any render: the trace launch behind the generator waits for the move like every other."""
    w, h = 40, 24
    scene = rt_host.load_scene("default14")
    cam, _ = CAMS[vu.PINHOLE]
    v = Views(lib, hip, vu.PINHOLE, w, h, cam)
    r = rt_host.Renderer(scene, 0, lib)
    o = Outputs(lib, w * h, 48 * w * 5)
    rays = Dev(lib, w * h * 48)
    ref = {k: Dev(lib, w * h * e) for k, e in Outputs.EACH.items()}
    try:
        o.trace(r, v.dev, w, h)
        before = o.read("rgba")
        i = next(i for i, ob in enumerate(scene["objects"]) if ob["r2"] < 1e4 and ob["mtl"]["albedo"][4] > 0)
        c0 = scene["objects"][i]["origin"]
        r.set_objects([dict(scene["objects"][i], origin=[c0[0] + 0.7, c0[1] + 0.3, c0[2] - 0.4])], first=i)
        o.trace(r, v.dev, w, h)
        r.view_rays(v.dev, w, h, rays.p)
        r.trace_rays(w * h, rays.p, ref["rgb"].p, ref["rgba"].p, ref["hits"].p, want_stats=True)
        assert all(o.read(k).tobytes() == ref[k].read().tobytes() for k in ref)
        assert (o.read("rgba") != before).any()
    finally:
        for d in [rays] + list(ref.values()):
            d.close()
        o.close()
        v.close()
        r.close()
