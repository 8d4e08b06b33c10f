"""Ambient occlusion on the GPU (include/rt_hip.h: struct rt_ambient).  The segment generator is held to the host probe; the fused kernel
to a value built from paths that exist without it: per sample the probe's segments through the existing rt_host.occlusion (length =
radius, intensity = 1.0, the probe's skips), folded in numpy in the stated order (tests/ambient_util.py).  Every comparison is of bytes:
the segments are + - * / and sqrt without FMA contraction on the probe's own source, the scan is rt_scene_occlusion_device's own step,
the fold is binary64 additions in a fixed order and one correctly rounded division.  No tolerance, no receiver left out.

Receivers: the hit records of a 96 x 54 pinhole at the reference's camera on default14 (glass, a skybox seen from inside), on h8, and on
h8 without its skybox (misses), as rt_trace_view writes them; hand-built records for receivers inside a sphere and records with a NaN."""
import ctypes as C
import json
import math

import numpy as np
import pytest

import ambient_util as au
import rt_host
from test_gpu_views import CANARY, Dev, hip, lib, upload  # noqa: F401  (lib and hip are fixtures)

pytestmark = pytest.mark.gpu
W, H = 96, 54
CONFIGS = [(1, 1, 0), (5, 5, 0), (16, 16, 0), (16, 64, 7)]            # n_samples, n_dirs, stride: n_dirs == n_samples with stride 0; a walk that wraps
RADII = [0.5, 2.0, math.inf]
SENTINEL_F64 = np.frombuffer(bytes([CANARY] * 8), np.uint64)[0]
SENTINEL_U32 = np.frombuffer(bytes([CANARY] * 4), np.uint32)[0]


def the_scene(name):
    s = rt_host.load_scene("h8" if name == "nosky" else name)
    if name == "nosky":
        s = dict(s, objects=[o for o in s["objects"] if o["r2"] < 1e7])      # without the enclosing sphere: rays that leave the scene miss
    return s


def camera_view(scene):
    c = scene["camera"]
    return rt_host.view(rt_host.RT_VIEW_PINHOLE, c["origin"], c["axisX"], c["axisY"], c["axisZ"], scene["fovDeg"])


_receivers = {}


def receivers(lib, name):
    """Per scene, once: (scene, hit records of the W x H view).  nosky's list ends in the hand-built records."""
    if name not in _receivers:
        scene = the_scene(name)
        h = rt_host.view_hit_records(scene, camera_view(scene), W, H, lib=lib)
        assert len(h) == W * H and (h["object"] >= 0).any()
        if name == "nosky":
            assert (h["object"] < 0).any()
            h = np.concatenate([h, au.hand_built()])
        else:
            assert (h["object"] >= 0).all() and (h["inside"] != 0).any()     # (the skybox is seen from inside)
        _receivers[name] = (scene, h)
    return _receivers[name]


class Fused:
    """Receivers and a table in device memory, canary-framed outputs, and Renderer.ambient on them."""
    EACH = {"open": (8, np.float64), "intensity": (8, np.float64), "rgba": (4, np.uint32)}

    def __init__(self, lib, hip, hits, dirs):
        self.lib, self.n, self.n_dirs = lib, len(hits), len(dirs)
        self.d_hits, self.d_dirs = upload(lib, hip, hits), upload(lib, hip, dirs)
        self.out = {k: Dev(lib, self.n * e) for k, (e, _) in self.EACH.items()}
        self.extra = []

    def reset(self):
        for k, d in self.out.items():
            assert self.lib.rt_memset_device(0, d.p, CANARY, d.n) == 0

    def run(self, r, n_samples, radius, stride, want=("open", "intensity", "rgba"), n=None, **kw):
        p = {k: (self.out[k].p if k in want else 0) for k in self.EACH}
        return r.ambient(self.n if n is None else n, self.d_hits, self.d_dirs, self.n_dirs, n_samples, radius, p["open"], p["intensity"], p["rgba"], stride=stride, **kw)

    def read(self, k):
        return self.out[k].read(self.EACH[k][1])

    def read_all(self):
        return tuple(self.read(k) for k in ("open", "intensity", "rgba"))

    def close(self):
        for d in self.out.values():
            d.close()
        for p in [self.d_hits, self.d_dirs] + self.extra:
            self.lib.rt_free_device(0, p)


def same(got, want, what):
    for g, w, k in zip(got, want, ("open", "intensity", "rgba")):
        g, w = np.ascontiguousarray(g), np.ascontiguousarray(w).astype(g.dtype, copy=False)
        diff = g.view(np.uint8).reshape(len(g), -1) != w.view(np.uint8).reshape(len(w), -1)
        assert not diff.any(), (what, k, int(diff.any(axis=1).sum()), int(np.flatnonzero(diff.any(axis=1))[0]))


# ------------------------------------------------------------------ 1. the generator against the host probe
def test_device_segments_are_the_probes(lib, hip):
    """Lists of 1, 63, 64, 65 and 257 receivers (a wave less one, a wave, a wave and one, a second workgroup with one live lane), every
    sample, from two places of a list that holds scanned receivers, misses and records with a non-finite word."""
    _, nosky = receivers(lib, "nosky")
    _, d14 = receivers(lib, "default14")
    mix = np.concatenate([au.hand_built(), nosky[W * 20:W * 20 + 150], d14[W * 30:W * 30 + 150]])
    assert 0 < au.scanned(mix).sum() < len(mix) and not au.scanned(mix[2:3]).any() and au.scanned(mix[0:1]).all()
    n_samples, n_dirs, stride, base = 5, 64, 7, 2 ** 40 + 3
    dirs = rt_host.ambient_dirs(n_dirs)
    r = rt_host.Renderer(the_scene("h8"), 0, lib)
    d_dirs = upload(lib, hip, dirs)
    try:
        for n in (1, 63, 64, 65, 257):
            for first in (0, 2):
                hits = mix[first:first + n]
                assert len(hits) == n
                d_hits = upload(lib, hip, hits)
                rays, skip = Dev(lib, n * 48), Dev(lib, n * 4)
                try:
                    for s in range(n_samples):
                        r.ambient_segments(n, d_hits, d_dirs, n_dirs, s, rays.p, skip.p, n_samples=n_samples, stride=stride, base=base)
                        want_rays, want_skip = rt_host.ambient_segments(hits, s, n_samples, dirs=dirs, stride=stride, base=base, lib=lib)
                        assert (rays.read(np.uint64) == au.bits(want_rays).reshape(-1)).all(), (n, first, s)       # (and nothing outside n records)
                        assert np.array_equal(skip.read(np.int32), want_skip), (n, first, s)
                    r.ambient_segments(n, d_hits, d_dirs, n_dirs, 0, rays.p, 0, n_samples=n_samples, stride=stride, base=base)   # without skips
                    assert np.array_equal(skip.read(np.int32), want_skip)
                finally:
                    rays.close(); skip.close()
                    lib.rt_free_device(0, d_hits)
    finally:
        lib.rt_free_device(0, d_dirs)
        r.close()


# ------------------------------------------------------------------ 2. the fused kernel against the fold of occlusion over the probe's segments
@pytest.mark.parametrize("name", ["default14", "h8", "nosky"])
def test_fused_is_the_fold_of_occlusion_over_the_probes_segments(lib, hip, name):
    scene, hits = receivers(lib, name)
    r = rt_host.Renderer(scene, 0, lib)
    try:
        for n_samples, n_dirs, stride in CONFIGS:
            dirs = rt_host.ambient_dirs(n_dirs)
            f = Fused(lib, hip, hits, dirs)
            try:
                at_2 = None
                for radius in RADII:
                    open_, intensity, rgba, li, bl = au.by_occlusion(scene, hits, dirs, n_samples, radius, stride=stride, lib=lib)
                    if radius == 2.0:
                        at_2 = (open_, intensity, rgba)
                    f.reset()
                    st = f.run(r, n_samples, radius, stride, want_stats=True)
                    assert st.pixels == len(hits) and st.kernel_ms > 0
                    same(f.read_all(), (open_, intensity, rgba), (name, n_samples, n_dirs, stride, radius))
                    ok = au.scanned(hits)
                    assert (open_[~ok] == 1.0).all() and np.isnan(intensity[~ok]).all() and not np.isnan(intensity[ok]).any()
                    assert (rgba >> 24 == 255).all() and ((rgba & 255) == (rgba >> 8 & 255)).all() and ((rgba & 255) == (rgba >> 16 & 255)).all()
                    if name == "default14" and radius == 2.0 and n_samples == 16:
                        # from the occlusion results alone: this view has partly open receivers, and scans that crossed glass
                        partly = int(((open_ > 0) & (open_ < 1)).sum())
                        glass = int(((li != 0.0) & (li != 1.0) & ~np.isnan(li)).sum())
                        print("AMBIENT default14 %dx%d, 16 samples (n_dirs %d, stride %d), radius 2.0: %d receivers partly open, %d scans crossed glass, "
                              "largest intensity %.4g" % (W, H, n_dirs, stride, partly, glass, np.nanmax(intensity)))
                        assert partly > 100 and glass > 100 and np.nanmax(intensity) > 1.0
                    if name == "nosky":
                        assert (~ok).sum() > 100                                   # misses, and the hand-built records
                # the host form gives the device form's bytes
                got = rt_host.ambient(scene, hits, n_samples, 2.0, dirs=dirs, stride=stride, want=("open", "intensity", "rgba"), lib=lib)
                same((got["open"], got["intensity"], got["rgba"].view(np.uint32).reshape(-1)), at_2, (name, "host form", n_samples))
            finally:
                f.close()
    finally:
        r.close()


# ------------------------------------------------------------------ 3. orders, NULL outputs, sentinels
def test_orders_and_null_outputs(lib, hip):
    scene, hits = receivers(lib, "default14")
    hits = np.concatenate([hits[W * 28:W * 28 + 700], au.hand_built()])
    n = len(hits)
    n_samples, n_dirs, stride, radius = 5, 64, 7, 2.0
    dirs = rt_host.ambient_dirs(n_dirs)
    want = au.by_occlusion(scene, hits, dirs, n_samples, radius, stride=stride, lib=lib)[:3]
    r = rt_host.Renderer(scene, 0, lib)
    f = Fused(lib, hip, hits, dirs)
    try:
        f.run(r, n_samples, radius, stride)
        same(f.read_all(), want, "the list's order")
        perm = np.random.default_rng(5).permutation(n).astype(np.uint32)
        f.extra.append(upload(lib, hip, perm))
        f.reset(); f.run(r, n_samples, radius, stride, order_ptr=f.extra[-1])
        same(f.read_all(), want, "a permutation")
        # entries >= n are skipped: the receivers no entry names keep the sentinel
        holes = perm.copy()
        dropped = np.arange(n) % 3 == 0
        holes[dropped] = np.where(np.arange(int(dropped.sum())) % 2 == 0, n, 0xFFFFFFFF).astype(np.uint32)
        named = np.zeros(n, bool)
        named[perm[~dropped]] = True
        assert named.any() and not named.all()
        f.extra.append(upload(lib, hip, holes))
        f.reset(); f.run(r, n_samples, radius, stride, order_ptr=f.extra[-1])
        got = f.read_all()
        same([g[named] for g in got], [w[named] for w in want], "an order with holes")
        assert (got[0][~named].view(np.uint64) == SENTINEL_F64).all() and (got[1][~named].view(np.uint64) == SENTINEL_F64).all()
        assert (got[2][~named] == SENTINEL_U32).all()
        # each output asked for alone is itself asked for with the others; the others keep the sentinel
        for i, k in enumerate(("open", "intensity", "rgba")):
            f.reset(); f.run(r, n_samples, radius, stride, want=(k,))
            got = f.read_all()
            same([got[i]], [want[i]], k + " alone")
            for j in range(3):
                if j != i:
                    assert (got[j].view(np.uint8) == CANARY).all(), (k, j)
        # a shorter list: nothing behind it is written
        f.reset(); f.run(r, n_samples, radius, stride, n=65)
        got = f.read_all()
        same([g[:65] for g in got], [w[:65] for w in want], "the first 65")
        assert all((g[65:].view(np.uint8) == CANARY).all() for g in got)
    finally:
        f.close()
        r.close()


# ------------------------------------------------------------------ 4. the host form past its chunk edge
def test_the_host_form_passes_each_chunk_its_base(lib):
    """2^18 + 1 receivers: the second chunk is one receiver, index 2^18, whose table entries differ from index 0's (n_dirs = 61 is prime)."""
    scene, base_list = receivers(lib, "default14")
    n, n_samples, n_dirs, stride, radius = 2 ** 18 + 1, 4, 61, 7, 2.0
    assert au.entry(0, 2 ** 18, stride, 0, n_dirs) != au.entry(0, 0, stride, 0, n_dirs)
    hits = base_list[np.arange(n) % len(base_list)]
    assert hits[2 ** 18].tobytes() == base_list[2 ** 18 % len(base_list)].tobytes()
    dirs = rt_host.ambient_dirs(n_dirs)
    want = ("open", "intensity", "rgba")
    whole = rt_host.ambient(scene, hits, n_samples, radius, dirs=dirs, stride=stride, want=want, lib=lib)
    a = rt_host.ambient(scene, hits[:2 ** 18], n_samples, radius, dirs=dirs, stride=stride, want=want, lib=lib)
    b = rt_host.ambient(scene, hits[2 ** 18:], n_samples, radius, dirs=dirs, stride=stride, want=want, base=2 ** 18, lib=lib)
    for k in want:
        assert whole[k].tobytes() == np.concatenate([a[k], b[k]]).tobytes(), k
    # ... and the receiver behind the edge against the yardstick, with the base and without it
    last = hits[2 ** 18:]
    assert au.scanned(last).all()
    open_, intensity, rgba, _, _ = au.by_occlusion(scene, last, dirs, n_samples, radius, stride=stride, base=2 ** 18, lib=lib)
    same((whole["open"][-1:], whole["intensity"][-1:], whole["rgba"].view(np.uint32).reshape(-1)[-1:]), (open_, intensity, rgba), "behind the chunk edge")
    # the first tile of the list is the small list's own answer
    small = rt_host.ambient(scene, base_list, n_samples, radius, dirs=dirs, stride=stride, want=want, lib=lib)
    for k in want:
        assert whole[k][:len(base_list)].tobytes() == small[k].tobytes(), k


# ------------------------------------------------------------------ 5. a whole view
@pytest.mark.parametrize("name", ["default14", "nosky"])
def test_ambient_view_is_ambient_of_the_views_hit_records(lib, hip, name):
    w, h = 33, 17
    scene = the_scene(name)
    v = camera_view(scene)
    n_samples, n_dirs, stride, radius = 5, 64, 7, 2.0
    dirs = rt_host.ambient_dirs(n_dirs)
    want_keys = ("open", "intensity", "rgba")
    hits = rt_host.view_hit_records(scene, v, w, h, lib=lib)
    want = rt_host.ambient(scene, hits, n_samples, radius, dirs=dirs, stride=stride, want=want_keys, lib=lib)
    got = rt_host.ambient_view(scene, v, w, h, n_samples, radius, dirs=dirs, stride=stride, want=want_keys, lib=lib)
    for k in want_keys:
        assert got[k].tobytes() == want[k].tobytes(), k
    assert len(set(got["rgba"].view(np.uint32).reshape(-1).tolist())) > 1                       # a picture, not a constant
    # the resident form: the least workspace (one row per band) and plenty give the host form's bytes
    r = rt_host.Renderer(scene, 0, lib)
    d_dirs = upload(lib, hip, dirs)
    try:
        for work_bytes in (128 * w, 128 * w * 5, rt_host.ambient_view_work_bytes(w, h)):
            out = {k: Dev(lib, w * h * e) for k, e in (("open", 8), ("intensity", 8), ("rgba", 4))}
            work = Dev(lib, work_bytes)
            try:
                st = r.ambient_view(v, w, h, d_dirs, n_dirs, n_samples, radius, out["open"].p, out["intensity"].p, out["rgba"].p, work.p, work_bytes, stride=stride,
                                    want_stats=True)
                assert st.pixels == w * h
                work.read()                                                                     # (its canaries)
                for k in want_keys:
                    assert out[k].read().tobytes() == want[k].tobytes(), (k, work_bytes)
            finally:
                work.close()
                for d in out.values():
                    d.close()
    finally:
        lib.rt_free_device(0, d_dirs)
        r.close()


# ------------------------------------------------------------------ 6. edits of the resident scene
def test_a_moved_occluder_shows_on_another_stream(lib, hip):
    scene, hits = receivers(lib, "h8")
    scene = dict(json.loads(json.dumps({k: v for k, v in scene.items() if k != "textures"})), textures=scene["textures"])      # (a copy to edit)
    n_samples, n_dirs, stride, radius = 5, 64, 7, 2.0
    dirs = rt_host.ambient_dirs(n_dirs)
    objs = scene["objects"]
    k = next(i for i, o in enumerate(objs) if o["r2"] == 1 and o["mtl"]["albedo"][4] == 0)
    r = rt_host.Renderer(scene, 0, lib)
    f = Fused(lib, hip, hits, dirs)
    other = C.c_void_p()
    assert hip.hipStreamCreate(C.byref(other)) == 0
    try:
        f.run(r, n_samples, radius, stride)
        before = f.read_all()
        objs[k]["origin"] = [objs[k]["origin"][0] + 0.75, objs[k]["origin"][1] + 0.5, objs[k]["origin"][2] + 0.25]
        r.set_objects(objs[k:k + 1], k, stream=other.value)
        f.reset(); f.run(r, n_samples, radius, stride, stream=other.value)
        assert hip.hipStreamSynchronize(other) == 0
        moved = f.read_all()
        fresh = rt_host.Renderer(scene, 0, lib)
        try:
            f.reset(); f.run(fresh, n_samples, radius, stride)
            want = f.read_all()
        finally:
            fresh.close()
        same(moved, want, "moved, another stream")
        assert moved[0].tobytes() != before[0].tobytes()                                       # the move shows
        same(moved, au.by_occlusion(scene, hits, dirs, n_samples, radius, stride=stride, lib=lib)[:3], "moved, the yardstick")
    finally:
        assert hip.hipStreamDestroy(other) == 0
        f.close()
        r.close()
