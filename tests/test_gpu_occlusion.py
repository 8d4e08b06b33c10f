"""Occlusion queries on the GPU (include/rt_hip.h: rt_scene_occlusion_device, rt_occlusion, rt_occlusion_binned).  Every comparison is
exact - the kernel is the strict arithmetic: the expected intensity of a whole light loop is the C restatement's own (the probe's q[18]
for every lit node of the ray trees of tests/occlusion_util.py's cases), the expected intensity and blocker of a single segment the
scalar Python restatement's, which test_occlusion.py holds to q[18] on the CPU."""
import ctypes as C
import json

import numpy as np
import pytest

import occlusion_util as ocu
import rt_host
from objects_util import tlib  # noqa: F401  (fixture: the test library)

pytestmark = pytest.mark.gpu
CANARY = 0x5A
GPU_CASES = ("default14", "lcg64_ss1")
_hip = None


def hip():
    global _hip
    _hip = _hip or C.CDLL("libamdhip64.so")
    return _hip


@pytest.fixture(scope="module")
def lib(built):
    lib = rt_host.load_library()
    assert lib.rt_init(1) == 0, lib.rt_last_error()
    return lib


class DeviceSegments:
    """A segment list in device memory (the ABI has no upload helper: hosts hand over memory they filled themselves) and guard-framed
    device outputs for Renderer.occlusion."""
    PAD = 256
    EACH = {"intensity": (8, np.float64), "blocker": (4, np.int32)}

    def __init__(self, lib, rays, length=None, intensity=None, skip=None, order=None, have=("intensity", "blocker")):
        self.lib, self.n = lib, len(rays)
        self.d = {}
        for k, a, t in (("rays", rays, np.float64), ("length", length, np.float64), ("intensity_in", intensity, np.float64), ("skip", skip, np.int32),
                        ("order", order, np.uint32)):
            self.d[k] = self.upload(np.ascontiguousarray(a, t)) if a is not None else 0
        self.p = {}
        for k in have:
            nbytes = self.n * self.EACH[k][0] + 2 * self.PAD
            self.p[k] = lib.rt_alloc_device(0, nbytes)
            assert self.p[k], lib.rt_last_error()
        self.reset()

    def upload(self, src):
        p = self.lib.rt_alloc_device(0, max(src.nbytes, 4))
        assert p, self.lib.rt_last_error()
        assert hip().hipMemcpy(C.c_void_p(p), src.ctypes.data_as(C.c_void_p), C.c_size_t(src.nbytes), 1) == 0
        return p

    def reset(self):
        for k, p in self.p.items():
            assert self.lib.rt_memset_device(0, p, CANARY, self.n * self.EACH[k][0] + 2 * self.PAD) == 0

    def ptr(self, k):
        return self.p[k] + self.PAD if k in self.p else 0

    def run(self, r, want=("intensity", "blocker"), n=None, ordered=False, stream=None, want_stats=False, **override):
        d = dict(self.d, **override)
        return r.occlusion(self.n if n is None else n, d["rays"], d["length"], d["intensity_in"], d["skip"],
                           self.ptr("intensity") if "intensity" in want else 0, self.ptr("blocker") if "blocker" in want else 0,
                           order_ptr=d["order"] if ordered else 0, stream=stream, want_stats=want_stats)

    def raw(self, k):
        size, dtype = self.EACH[k]
        raw = np.empty(self.n * size + 2 * self.PAD, np.uint8)
        assert self.lib.rt_copy_to_host(0, raw.ctypes.data, self.p[k], raw.nbytes) == 0
        assert (raw[:self.PAD] == CANARY).all() and (raw[-self.PAD:] == CANARY).all(), k        # the guard words
        return raw[self.PAD:-self.PAD].view(dtype).copy()

    def read(self, n=None):
        """-> (intensity, blocker) of the first n rays; guards and everything past n intact."""
        out = []
        for k in ("intensity", "blocker"):
            a = self.raw(k)
            m = self.n if n is None else n
            assert (a[m:].view(np.uint8) == CANARY).all(), k
            out.append(a[:m])
        return out

    def close(self):
        for p in list(self.p.values()) + [p for p in self.d.values() if p]:
            self.lib.rt_free_device(0, p)
        self.p, self.d = {}, {}


SENTINEL_F64 = np.frombuffer(bytes([CANARY] * 8), np.float64)[0]
SENTINEL_I32 = np.frombuffer(bytes([CANARY] * 4), np.int32)[0]


def bits(a):
    return np.ascontiguousarray(a).tobytes()


def check(got, want_li, want_bl, what=""):
    li, bl = got
    assert np.array_equal(bl, want_bl), (what, int((bl != want_bl).sum()))
    assert bits(li) == bits(want_li), (what, int((li.view(np.uint64) != np.ascontiguousarray(want_li).view(np.uint64)).sum()))


_device_cases = {}


def device_case(lib, case):
    """Per case, once: the renderer, the segments in device memory and the device form's answer for them."""
    if case not in _device_cases:
        sg = ocu.segments(case)
        r = rt_host.Renderer(ocu.nodes(case)["scene"], 0, lib)
        d = DeviceSegments(lib, sg["rays"], sg["length"], sg["intensity"], sg["skip"])
        st = d.run(r, want_stats=True)
        assert st.pixels == len(sg["length"]) and st.kernel_ms > 0 and st.total_ms > 0
        _device_cases[case] = (r, d, d.read())
    return _device_cases[case]


# ------------------------------------------------------------------ 1. the nodes of the ray trees
@pytest.mark.parametrize("case", GPU_CASES)
def test_ray_tree_nodes(lib, case):
    """light_intensity_at through the GPU is q[18] of every lit node; every single segment's intensity and blocker are the restatement's."""
    nd, sg = ocu.nodes(case), ocu.segments(case)
    got = rt_host.light_intensity_at(nd["scene"], nd["point"], nd["facing"], nd["sphere"], lib=lib)
    diff = got.view(np.uint64) != nd["expected"].view(np.uint64)
    print("OCCLUSION %s: %d of %d nodes differ from q[18]" % (case, int(diff.sum()), len(diff)))
    assert not diff.any()
    _, _, first = device_case(lib, case)
    check(first, sg["want_intensity"], sg["want_blocker"], case)
    assert (sg["want_blocker"] >= 0).any() and (sg["want_intensity"] > sg["intensity"]).any() == (case == "default14")


# ------------------------------------------------------------------ 2. skip
@pytest.mark.parametrize("case", GPU_CASES)
def test_skip(lib, case):
    nd, sg = ocu.nodes(case), ocu.segments(case)
    scene = nd["scene"]
    r, d, first = device_case(lib, case)
    d.reset()
    d.run(r, skip=0)                                       # NULL: no sphere is left out
    none = d.read()
    check(none, *ocu.scan_list(scene, sg["rays"], sg["length"], sg["intensity"], None), "skip NULL")
    differs = int(((none[1] != first[1]) | (none[0].view(np.uint64) != first[0].view(np.uint64))).sum())
    print("OCCLUSION %s: %d of %d segments change without skip" % (case, differs, len(sg["skip"])))
    # the receiver matters where the segment starts INSIDE it - a glass sphere's far wall, which divides the intensity once more: the
    # restatement finds 491 such segments in default14 and none in lcg64_ss1, which has no glass (a convex opaque receiver that faces
    # the light is never met again: both its roots lie below epsilon)
    assert differs >= 1 or case != "default14"
    wrong = ((sg["skip"] + 1) % len(scene["objects"])).astype(np.int32)
    outside = np.where(np.arange(len(wrong)) % 2 == 0, -7, len(scene["objects"])).astype(np.int32)      # outside [0, n_objects): none
    for name, skip, want in (("wrong", wrong, ocu.scan_list(scene, sg["rays"], sg["length"], sg["intensity"], wrong)), ("outside", outside, none)):
        p = d.upload(skip)
        try:
            d.reset()
            d.run(r, skip=p)
            check(d.read(), want[0], want[1], name)
        finally:
            lib.rt_free_device(0, p)


# ------------------------------------------------------------------ 3. input defaults
def test_input_defaults(lib):
    case = "default14"
    nd, sg = ocu.nodes(case), ocu.segments(case)
    scene = nd["scene"]
    r, d, first = device_case(lib, case)
    n = len(sg["length"])
    # length NULL is +Infinity
    inf = d.upload(np.full(n, np.inf))
    nan = d.upload(np.full(n, np.nan))
    try:
        d.reset(); d.run(r, length=0); endless = d.read()
        d.reset(); d.run(r, length=inf)
        check(d.read(), *endless, "length NULL")
        want = ocu.scan_list(scene, sg["rays"], None, sg["intensity"], sg["skip"])
        assert (want[1] != sg["want_blocker"]).any()       # (the length matters: without it segments go on to the skybox)
        check(endless, *want, "length inf")
        # a NaN length occludes nothing
        d.reset(); d.run(r, length=nan)
        check(d.read(), sg["intensity"], np.full(n, -1, np.int32), "length NaN")
    finally:
        lib.rt_free_device(0, inf)
        lib.rt_free_device(0, nan)
    # intensity NULL is the scene's current light intensity
    try:
        for value in (float(scene.get("light_intensity", 50)), 12.5):
            r.set_light_intensity(value)
            d.reset(); d.run(r, intensity_in=0)
            check(d.read(), *ocu.scan_list(dict(scene, light_intensity=value), sg["rays"], sg["length"], None, sg["skip"]), "intensity NULL %r" % value)
    finally:
        r.set_light_intensity(float(scene.get("light_intensity", 50)))
    # a ray with a NaN or an infinity in any slot: NaN, -1, and its neighbours are untouched
    rays = sg["rays"][:200].copy()
    bad = {}
    for slot in range(6):
        for j, v in enumerate((np.nan, np.inf, -np.inf)):
            i = 7 + 9 * (3 * slot + j)
            rays[i, slot] = v
            bad[i] = v
    e = DeviceSegments(lib, rays, sg["length"][:200], sg["intensity"][:200], sg["skip"][:200])
    try:
        e.run(r)
        li, bl = e.read()
    finally:
        e.close()
    good = np.array([i not in bad for i in range(200)])
    assert np.isnan(li[~good]).all() and (bl[~good] == -1).all() and len(bad) == 18
    assert bits(li[good]) == bits(first[0][:200][good]) and np.array_equal(bl[good], first[1][:200][good])


# ------------------------------------------------------------------ 4. sizes and bounds
@pytest.mark.parametrize("n", [1, 63, 64, 257, 4097])
def test_sizes_and_bounds(lib, n):
    case = "lcg64_ss1"
    sg = ocu.segments(case)
    r, d, first = device_case(lib, case)
    assert n < d.n
    d.reset()
    d.run(r, n=n)
    li, bl = d.read(n)                                     # guards and every element past n keep their bytes
    assert bits(li) == bits(sg["want_intensity"][:n]) and np.array_equal(bl, sg["want_blocker"][:n])
    for only, other in (("intensity", "blocker"), ("blocker", "intensity")):
        d.reset()
        d.run(r, want=(only,), n=n)
        assert (d.raw(other).view(np.uint8) == CANARY).all(), other
        got = d.raw(only)
        assert bits(got[:n]) == bits((li if only == "intensity" else bl)) and (got[n:].view(np.uint8) == CANARY).all()


# ------------------------------------------------------------------ 5. orders
def test_orders(lib):
    case = "lcg64_ss1"
    sg = ocu.segments(case)
    r, d, first = device_case(lib, case)
    n = d.n
    work_bytes = rt_host.rays_order_work_bytes(n)
    d_order, d_work = lib.rt_alloc_device(0, 4 * n), lib.rt_alloc_device(0, work_bytes)
    assert d_order and d_work
    extra = []
    try:
        r.order_rays(n, d.d["rays"], d_order, d_work, work_bytes)
        order = np.empty(n, np.uint32)
        assert lib.rt_copy_to_host(0, order.ctypes.data, d_order, 4 * n) == 0
        assert np.array_equal(np.sort(order), np.arange(n, dtype=np.uint32)) and not np.array_equal(order, np.arange(n, dtype=np.uint32))
        d.reset(); d.run(r, ordered=True, order=d_order)
        check(d.read(), *first, "the library's order")
        perm = np.random.default_rng(21).permutation(n).astype(np.uint32)
        extra.append(d.upload(perm))
        d.reset(); d.run(r, ordered=True, order=extra[-1])
        check(d.read(), *first, "a random permutation")
        # entries >= n are skipped: the rays no entry names keep the sentinel
        holes = perm.copy()
        dropped = np.arange(n) % 3 == 0
        holes[dropped] = np.where(np.arange(int(dropped.sum())) % 2 == 0, n, 0xFFFFFFFF).astype(np.uint32)
        named = np.zeros(n, bool)
        named[perm[~dropped]] = True
        assert named.any() and not named.all()
        extra.append(d.upload(holes))
        d.reset(); d.run(r, ordered=True, order=extra[-1])
        li, bl = d.read()
        assert bits(li[named]) == bits(first[0][named]) and np.array_equal(bl[named], first[1][named])
        assert (li[~named].view(np.uint64) == SENTINEL_F64.view(np.uint64)).all() and (bl[~named] == SENTINEL_I32).all()
    finally:
        for p in [d_order, d_work] + extra:
            lib.rt_free_device(0, p)


# ------------------------------------------------------------------ 6. edits of the resident scene
def test_edits(lib):
    case = "default14"
    nd, sg = ocu.nodes(case), ocu.segments(case)
    scene = json.loads(json.dumps({k: v for k, v in nd["scene"].items() if k != "textures"}))
    scene["textures"] = nd["scene"]["textures"]
    objs = scene["objects"]
    take = slice(0, 600)
    rays, length, li_in, skip = sg["rays"][take], sg["length"][take], sg["intensity"][take], sg["skip"][take]
    # an opaque sphere of the scene proper and a free segment that is longer than its diameter and does not start on it
    k = next(i for i, o in enumerate(objs) if o["r2"] < 1e4 and o["mtl"]["albedo"][4] == 0)
    radius = objs[k]["r2"] ** 0.5
    s = next(i for i in range(len(length)) if sg["want_blocker"][i] < 0 and skip[i] != k and length[i] > 2 * radius + 1)
    home = list(objs[k]["origin"])
    onto = [float(rays[s, c] + rays[s, 3 + c] * (length[s] / 2)) for c in range(3)]
    r = rt_host.Renderer(scene, 0, lib)
    d = DeviceSegments(lib, rays, length, li_in, skip)
    other = C.c_void_p()
    assert hip().hipStreamCreate(C.byref(other)) == 0
    try:
        d.run(r)
        first = d.read()
        check(first, sg["want_intensity"][take], sg["want_blocker"][take], "before")
        objs[k]["origin"] = onto
        want = ocu.scan_list(scene, rays, length, li_in, skip)
        assert want[1][s] == k and first[1][s] == -1
        r.set_objects(objs[k:k + 1], k)
        d.reset(); d.run(r)                                # right behind the edit, on the library's stream
        check(d.read(), *want, "moved, same stream")
        r.set_objects(objs[k:k + 1], k, stream=other.value)
        d.reset(); d.run(r, stream=other.value)            # and on another stream
        assert hip().hipStreamSynchronize(other) == 0
        check(d.read(), *want, "moved, another stream")
        objs[k]["origin"] = home
        r.set_objects(objs[k:k + 1], k)
        d.reset(); d.run(r, stream=other.value)
        assert hip().hipStreamSynchronize(other) == 0
        check(d.read(), *first, "moved back")
        r.set_lights([[-3.0, 6.0, 2.0]], 1)                # the lights' positions play no part
        d.reset(); d.run(r)
        check(d.read(), *first, "after set_lights")
    finally:
        assert hip().hipStreamDestroy(other) == 0
        d.close()
        r.close()


# ------------------------------------------------------------------ 7. the host form
def test_host_form(tlib):  # noqa: F811
    case = "default14"
    nd, sg = ocu.nodes(case), ocu.segments(case)
    scene = nd["scene"]
    n = 2 ** 18 + 5                                        # two chunks, the second of 5 rays
    idx = np.arange(n) % len(sg["length"])
    rays, length, li_in, skip = sg["rays"][idx], sg["length"][idx], sg["intensity"][idx], sg["skip"][idx]
    want_li, want_bl = sg["want_intensity"][idx], sg["want_blocker"][idx]
    got = rt_host.occlusion(scene, rays, length, li_in, skip, want=("intensity", "blocker"), lib=tlib)
    check((got["intensity"], got["blocker"]), want_li, want_bl, "list")
    uploads = tlib.rt_test_upload_count()
    binned = rt_host.occlusion(scene, rays, length, li_in, skip, want=("intensity", "blocker"), lib=tlib, order="binned")
    check((binned["intensity"], binned["blocker"]), want_li, want_bl, "binned")
    alone = rt_host.occlusion(scene, rays[:300], length[:300], li_in[:300], skip[:300], want=("blocker",), lib=tlib)
    assert set(alone) == {"blocker"} and np.array_equal(alone["blocker"], want_bl[:300])
    # a blob that differs only in the camera is the resident scene
    moved = dict(scene, camera=dict(scene["camera"], origin=[1.0, 2.0, 9.0]))
    again = rt_host.occlusion(moved, rays[:300], length[:300], li_in[:300], skip[:300], want=("intensity",), lib=tlib)
    assert bits(again["intensity"]) == bits(want_li[:300])
    assert tlib.rt_test_upload_count() == uploads
