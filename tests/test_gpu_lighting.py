"""Sampled lights on the GPU (include/rt_hip.h: struct rt_lighting).  The fused kernel is held to two things that exist without it.
The restatement: with one sample and point lights, `intensity` is q[18] and min(1, diffuse) * albedo[1] is q[15] of the C restatement's
probe (oracle/rt_oracle.c) for every lit node of the occlusion cases.  Its parts: per (sample, light) the host probe's segments through
the existing rt_host.occlusion - the intensity chained from light to light, only the receivers that face the light scanned -, folded in
numpy in the stated order (tests/lighting_util.py).  Every comparison is of bytes: the segments are + - * / and sqrt without FMA
contraction on the probe's own source, the scan is rt_scene_occlusion_device's own step, the fold is binary64 additions in a fixed
order and one correctly rounded division.  No tolerance, no receiver left out."""
import ctypes as C
import json

import numpy as np
import pytest

import lighting_util as lu
import occlusion_util as ocu
import rt_host
from test_gpu_views import CANARY, Dev, hip, lib, upload  # noqa: F401  (lib and hip are fixtures)

pytestmark = pytest.mark.gpu
W, H = 96, 54
KEYS = lu.OUTPUTS
SENTINEL_F64 = np.frombuffer(bytes([CANARY] * 8), np.uint64)[0]
SENTINEL_U32 = np.frombuffer(bytes([CANARY] * 4), np.uint32)[0]


def copy_of(scene, **changes):
    """A scene dict to edit: everything but the textures' texels copied."""
    return dict(json.loads(json.dumps({k: v for k, v in scene.items() if k != "textures"})), textures=scene["textures"], **changes)


_receivers = {}


def receivers(lib, name):
    """Per scene, once: (scene, hit records of the W x H view from the scene's camera)."""
    if name not in _receivers:
        scene = rt_host.load_scene(name)
        h = rt_host.view_hit_records(scene, lu.camera_view(scene), W, H, lib=lib)
        assert len(h) == W * H and (h["object"] >= 0).all() and (h["inside"] != 0).any()     # (the skybox is seen from inside)
        _receivers[name] = (scene, h)
    return _receivers[name]


class Fused:
    """Receivers and a table in device memory, canary-framed outputs, and Renderer.lighting on them."""
    EACH = {"diffuse": (8, np.float64), "intensity": (8, np.float64), "lit": (8, np.float64), "rgba": (4, np.uint32)}

    def __init__(self, lib, hip, hits, offs=None):
        self.lib, self.n, self.n_offs = lib, len(hits), 0 if offs is None else len(offs)
        self.d_hits = upload(lib, hip, hits)
        self.d_offs = upload(lib, hip, offs) if offs is not None else 0
        self.out = {k: Dev(lib, self.n * e) for k, (e, _) in self.EACH.items()}
        self.extra = []

    def reset(self):
        for d in self.out.values():
            assert self.lib.rt_memset_device(0, d.p, CANARY, d.n) == 0

    def run(self, r, n_samples, light_radius, stride, want=KEYS, n=None, **kw):
        p = {k: (self.out[k].p if k in want else 0) for k in self.EACH}
        return r.lighting(self.n if n is None else n, self.d_hits, self.d_offs, self.n_offs or n_samples, n_samples, light_radius, p["diffuse"], p["intensity"],
                          p["lit"], p["rgba"], stride=stride, **kw)

    def read_all(self):
        return tuple(self.out[k].read(self.EACH[k][1]) for k in KEYS)

    def close(self):
        for d in self.out.values():
            d.close()
        for p in [self.d_hits] + ([self.d_offs] if self.d_offs else []) + self.extra:
            self.lib.rt_free_device(0, p)


def tup(d):
    """The four outputs of a dict (rt_host.lighting's, lighting_util.by_occlusion's) as arrays of the buffers' types."""
    return tuple(np.ascontiguousarray(d[k]).view(np.uint32).reshape(-1) if k == "rgba" else d[k] for k in KEYS)


def same(got, want, what):
    for g, w, k in zip(got, want, KEYS):
        g, w = np.ascontiguousarray(g), np.ascontiguousarray(w).astype(g.dtype, copy=False)
        assert g.shape == w.shape, (what, k)
        diff = g.view(np.uint8).reshape(len(g), -1) != w.view(np.uint8).reshape(len(w), -1)
        assert not diff.any(), (what, k, int(diff.any(axis=1).sum()), int(np.flatnonzero(diff.any(axis=1))[0]))


# ------------------------------------------------------------------ 1. the restatement: q[18] and q[15] of every lit node
@pytest.mark.parametrize("case", ["default14", "h8", "lcg64_ss1"])
def test_one_sample_of_point_lights_is_the_reference_loop(lib, hip, case):
    """Receivers from hit_records(point, normal, sphere, inside) of the C restatement's lit nodes; n_samples = 1, light_radius = 0.
    No sample is left out: none of the three cases overflows its probe (asserted here and in tests/test_lighting.py - the occlusion
    tests tolerate none either)."""
    nd = lu.probe_nodes(case)
    assert nd["overflowed"] == 0
    hits = lu.node_receivers(case)
    r = rt_host.Renderer(nd["scene"], 0, lib)
    f = Fused(lib, hip, hits)
    try:
        f.reset()
        st = f.run(r, 1, 0.0, 1, want_stats=True)
        assert st.pixels == len(hits) and st.kernel_ms > 0
        diffuse, intensity, lit, rgba = f.read_all()
    finally:
        f.close()
        r.close()
    assert ocu.same_bits(intensity, nd["expected"]), int((lu.bits(intensity) != lu.bits(nd["expected"])).sum())
    mine = lu.jsmin1(diffuse) * nd["albedo1"]
    assert ocu.same_bits(mine, nd["diffuse"]), int((lu.bits(mine) != lu.bits(nd["diffuse"])).sum())
    # ... and the host form gives the device form's bytes
    got = rt_host.lighting(nd["scene"], hits, want=KEYS, lib=lib)
    same(tup(got), (diffuse, intensity, lit, rgba), (case, "host form"))
    n_lights = len(nd["scene"]["lights"])
    assert (rgba >> 24 == 255).all() and (lit * n_lights == np.rint(lit * n_lights)).all() and lit.min() >= 0.0 and lit.max() <= 1.0
    assert np.array_equal(rgba & 255, lu.to_byte(lu.jsmin1(diffuse)))


# ------------------------------------------------------------------ 2. the soft case: lights with a size
def test_soft_shadows_are_the_fold_of_occlusion_over_the_probes_segments(lib, hip):
    """A 96 x 54 pinhole view of default14 from the scene's camera; 16 samples, 64 offsets as four turned sets, stride 16, radius 1.0."""
    scene, hits = receivers(lib, "default14")
    n_samples, radius, stride = 16, 1.0, 16
    offs = lu.turned_sets(16, 4)
    assert offs.shape == (64, 3)
    want = lu.by_occlusion(scene, hits, offs, n_samples, radius, stride=stride, lib=lib)
    partly, penumbra, raised = lu.soft_counts(want, scene)
    print("LIGHTING default14 %dx%d, 16 samples (64 offsets, stride 16), light_radius 1.0: %d receivers with 0 < lit < 1, %d in a penumbra (samples that "
          "disagree), %d with an intensity above the scene's, largest %.4g; largest diffuse %.4g"
          % (W, H, partly, penumbra, raised, np.nanmax(want["intensity"]), np.nanmax(want["diffuse"])))
    assert partly >= 1 and penumbra >= 1 and raised >= 1                                    # a vacuous input fails
    v = lu.camera_view(scene)
    got = rt_host.lighting(scene, hits, n_samples, radius, offs=offs, stride=stride, want=KEYS, lib=lib)
    same(tup(got), tup(want), "lighting")
    got = rt_host.lighting_view(scene, v, W, H, n_samples, radius, offs=offs, stride=stride, want=KEYS, lib=lib)
    same(tup(got), tup(want), "lighting_view")
    # the resident forms: the list, and the view with a workspace of one row and of the whole view
    r = rt_host.Renderer(scene, 0, lib)
    f = Fused(lib, hip, hits, offs)
    try:
        f.reset()
        f.run(r, n_samples, radius, stride)
        same(f.read_all(), tup(want), "Renderer.lighting")
        for work_bytes in (128 * W, rt_host.lighting_view_work_bytes(W, H)):
            assert work_bytes >= 128 * W
            out = {k: Dev(lib, W * H * e) for k, (e, _) in Fused.EACH.items()}
            work = Dev(lib, work_bytes)
            try:
                st = r.lighting_view(v, W, H, f.d_offs, len(offs), n_samples, radius, out["diffuse"].p, out["intensity"].p, out["lit"].p, out["rgba"].p, work.p,
                                     work_bytes, stride=stride, want_stats=True)
                assert st.pixels == W * H
                work.read()                                                                 # (its canaries)
                same(tuple(out[k].read(Fused.EACH[k][1]) for k in KEYS), tup(want), ("Renderer.lighting_view", work_bytes))
            finally:
                work.close()
                for d in out.values():
                    d.close()
    finally:
        f.close()
        r.close()


# ------------------------------------------------------------------ 3. edges: list sizes, sample counts, strides, receivers no view gives
def test_list_sizes_sample_counts_and_strides(lib, hip):
    """1, 63, 64, 65 and 257 receivers (a wave less one, a wave, a wave and one, a second workgroup with one live lane), from a list
    that starts with the hand-built records (inside a sphere, a miss, a NaN, an Inf); 1, 2 and 3 samples; stride 0 (scalar loads of
    the table) and 1.  Receiver i's answer does not depend on the list's length, so one yardstick serves the five sizes."""
    scene, d14 = receivers(lib, "default14")
    mix = np.concatenate([lu.hand_built(), d14[W * 30:W * 30 + 251]])
    assert len(mix) == 257 and 0 < (~lu.scanned(mix)).sum() < 10
    offs = lu.turned_sets(3, 4)
    r = rt_host.Renderer(scene, 0, lib)
    f = Fused(lib, hip, mix, offs)
    try:
        for n_samples in (1, 2, 3):
            for stride in (0, 1):
                want = tup(lu.by_occlusion(scene, mix, offs, n_samples, 0.75, stride=stride, lib=lib))
                ok = lu.scanned(mix)
                assert np.isnan(want[0][~ok]).all() and np.isnan(want[1][~ok]).all() and (want[2][~ok] == 0.0).all() and (want[3][~ok] == 0xff000000).all()
                assert not np.isnan(want[0][ok]).any()
                for n in (1, 63, 64, 65, 257):
                    f.reset()
                    f.run(r, n_samples, 0.75, stride, n=n)
                    got = f.read_all()
                    same([g[:n] for g in got], [w[:n] for w in want], (n_samples, stride, n))
                    assert all((g[n:].view(np.uint8) == CANARY).all() for g in got), (n_samples, stride, n)      # nothing behind the list
        # each output asked for alone is itself asked for with the others; the others keep the sentinel
        for i, k in enumerate(KEYS):
            f.reset(); f.run(r, 3, 0.75, 1, want=(k,))
            got = f.read_all()
            same([got[i]], [want[i]], k + " alone")
            assert all((got[j].view(np.uint8) == CANARY).all() for j in range(4) if j != i), k
    finally:
        f.close()
        r.close()


@pytest.mark.parametrize("n_lights", [0, 16])
def test_a_scene_without_lights_and_one_with_sixteen(lib, hip, n_lights):
    base_scene, hits = receivers(lib, "default14")
    hits = np.concatenate([hits[W * 28:W * 28 + 300], lu.hand_built()])
    lights = [[5.0 - 0.9 * k, 10.0 - 0.3 * (k % 3), 5.0 - 0.7 * k] for k in range(n_lights)]
    scene = copy_of(base_scene, lights=lights)
    offs = lu.turned_sets(2, 2)
    want = lu.by_occlusion(scene, hits, offs, 2, 0.5, stride=2, lib=lib)
    ok = lu.scanned(hits)
    if n_lights == 0:
        assert (want["diffuse"][ok] == 0.0).all() and (want["intensity"][ok] == scene["light_intensity"]).all() and (want["lit"] == 0.0).all()
    else:
        assert len(np.unique(want["lit"])) > 4 and (want["contributed"].max(axis=0)[ok] <= 16).all()
    r = rt_host.Renderer(scene, 0, lib)
    f = Fused(lib, hip, hits, offs)
    try:
        f.reset()
        f.run(r, 2, 0.5, 2)
        same(f.read_all(), tup(want), n_lights)
    finally:
        f.close()
        r.close()
    same(tup(rt_host.lighting(scene, hits, 2, 0.5, offs=offs, stride=2, want=KEYS, lib=lib)), tup(want), (n_lights, "host form"))


def test_a_reversed_order_with_an_entry_that_names_no_receiver(lib, hip):
    scene, hits = receivers(lib, "default14")
    hits = np.concatenate([hits[W * 28:W * 28 + 700], lu.hand_built()])
    n = len(hits)
    offs = lu.turned_sets(3, 4)
    r = rt_host.Renderer(scene, 0, lib)
    f = Fused(lib, hip, hits, offs)
    try:
        f.reset(); f.run(r, 3, 0.5, 3)
        plain = f.read_all()
        same(plain, tup(lu.by_occlusion(scene, hits, offs, 3, 0.5, stride=3, lib=lib)), "the list's order")
        order = np.arange(n, dtype=np.uint32)[::-1].copy()
        named = np.ones(n, bool)
        for at, bad in ((5, n), (n // 2, 0xFFFFFFFF), (n - 1, n + 7)):
            named[order[at]] = False
            order[at] = bad
        f.extra.append(upload(lib, hip, order))
        f.reset(); f.run(r, 3, 0.5, 3, order_ptr=f.extra[-1])
        got = f.read_all()
        same([g[named] for g in got], [p[named] for p in plain], "reversed")
        assert (~named).sum() == 3
        assert all((g[~named].view(np.uint64) == SENTINEL_F64).all() for g in got[:3]) and (got[3][~named] == SENTINEL_U32).all()
    finally:
        f.close()
        r.close()


def test_the_host_form_passes_each_chunk_its_base(lib):
    """2^18 + 1 receivers, one sample, radius 0.25: the second chunk is one receiver, index 2^18, whose table entry differs from index
    0's (n_offs = 61 is prime)."""
    scene, base_list = receivers(lib, "default14")
    n, n_offs = 2 ** 18 + 1, 61
    assert lu.entry(0, 2 ** 18, 1, 0, n_offs) != lu.entry(0, 0, 1, 0, n_offs)
    hits = base_list[np.arange(n) % len(base_list)]
    offs = rt_host.lighting_offsets(n_offs)
    whole = rt_host.lighting(scene, hits, 1, 0.25, offs=offs, want=KEYS, lib=lib)
    a = rt_host.lighting(scene, hits[:2 ** 18], 1, 0.25, offs=offs, want=KEYS, lib=lib)
    b = rt_host.lighting(scene, hits[2 ** 18:], 1, 0.25, offs=offs, want=KEYS, base=2 ** 18, lib=lib)
    for k in KEYS:
        assert whole[k].tobytes() == np.concatenate([a[k], b[k]]).tobytes(), k
    # ... and the receiver behind the edge against the yardstick, with its base
    last = hits[2 ** 18:]
    assert lu.scanned(last).all()
    same(tuple(x[-1:] for x in tup(whole)), tup(lu.by_occlusion(scene, last, offs, 1, 0.25, base=2 ** 18, lib=lib)), "behind the chunk edge")
    # a window of the list against the yardstick: receiver i reads entry i % 61
    at = 2 ** 18 - 200
    same(tuple(x[at:at + 200] for x in tup(whole)), tup(lu.by_occlusion(scene, hits[at:at + 200], offs, 1, 0.25, base=at, lib=lib)), "before the chunk edge")


# ------------------------------------------------------------------ 4. edits of the resident scene
def test_moved_lights_and_a_new_intensity_are_seen(lib, hip):
    scene, hits = receivers(lib, "default14")
    scene = copy_of(scene)
    offs = lu.turned_sets(4, 4)
    r = rt_host.Renderer(scene, 0, lib)
    f = Fused(lib, hip, hits, offs)
    try:
        f.reset(); f.run(r, 4, 0.5, 4)
        before = f.read_all()
        scene["lights"] = [[-4.0, 9.0, 3.0], [2.5, 8.0, -1.0]]
        scene["light_intensity"] = 35.5
        r.set_lights(scene["lights"])
        r.set_light_intensity(scene["light_intensity"])
        f.reset(); f.run(r, 4, 0.5, 4)
        after = f.read_all()
        assert after[0].tobytes() != before[0].tobytes() and after[1].tobytes() != before[1].tobytes()
        same(after, tup(rt_host.lighting(scene, hits, 4, 0.5, offs=offs, stride=4, want=KEYS, lib=lib)), "the host form on the edited scene dict")
        same(after, tup(lu.by_occlusion(scene, hits, offs, 4, 0.5, stride=4, lib=lib)), "the yardstick on the edited scene dict")
    finally:
        f.close()
        r.close()


def test_a_moved_occluder_is_seen(lib, hip):
    scene, hits = receivers(lib, "h8")
    scene = copy_of(scene)
    offs = lu.turned_sets(4, 4)
    objs = scene["objects"]
    k = next(i for i, o in enumerate(objs) if o["r2"] == 1 and o["mtl"]["albedo"][4] == 0)
    r = rt_host.Renderer(scene, 0, lib)
    f = Fused(lib, hip, hits, offs)
    other = C.c_void_p()
    assert hip.hipStreamCreate(C.byref(other)) == 0
    try:
        f.reset(); f.run(r, 4, 0.5, 4)
        before = f.read_all()
        objs[k]["origin"] = [objs[k]["origin"][0] + 0.75, objs[k]["origin"][1] + 0.5, objs[k]["origin"][2] + 0.25]
        r.set_objects(objs[k:k + 1], k, stream=other.value)
        f.reset(); f.run(r, 4, 0.5, 4, stream=other.value)            # (behind the move on its stream; any other stream waits by event)
        assert hip.hipStreamSynchronize(other) == 0
        moved = f.read_all()
        assert moved[2].tobytes() != before[2].tobytes()                                       # the move shows
        same(moved, tup(rt_host.lighting(scene, hits, 4, 0.5, offs=offs, stride=4, want=KEYS, lib=lib)), "the host form on the edited scene dict")
        same(moved, tup(lu.by_occlusion(scene, hits, offs, 4, 0.5, stride=4, lib=lib)), "the yardstick on the edited scene dict")
    finally:
        assert hip.hipStreamDestroy(other) == 0
        f.close()
        r.close()
