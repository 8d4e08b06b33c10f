"""Binned ray lists on the GPU (include/rt_hip.h: rt_scene_order_rays_device, rt_scene_trace_rays_ordered_device,
rt_trace_rays_binned).  Every comparison is exact: an order decides which rays share a wave and nothing a caller can read, so an
ordered trace is held to the plain one byte for byte (rgb, rgba, hit records), and - independently of the plain path - to the
unchanged C restatement through micro-cameras (tests/rays_util.py) on inputs for which the plain path's table in docs/EVIDENCE.md
shows no differing channel."""
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
from test_gpu_rays import SCENES, DeviceRays, hit_bytes

pytestmark = pytest.mark.gpu
ROOT = ou.ROOT
PKG = os.path.join(ROOT, "html5-canvas-raytracer_amd")


@pytest.fixture(scope="module")
def lib(built):
    lib = rt_host.load_library()
    assert lib.rt_init(1) == 0, lib.rt_last_error()
    return lib


_hip = None


def upload(lib, array):
    """A host array -> device memory holding its bytes (rt_alloc_device)."""
    global _hip
    _hip = _hip or C.CDLL("libamdhip64.so")
    src = np.ascontiguousarray(array)
    p = lib.rt_alloc_device(0, max(src.nbytes, 4))
    assert p, lib.rt_last_error()
    assert _hip.hipMemcpy(C.c_void_p(p), src.ctypes.data_as(C.c_void_p), C.c_size_t(src.nbytes), 1) == 0
    return p


def download(lib, p, count, dtype):
    out = np.empty(count, dtype)
    assert lib.rt_copy_to_host(0, out.ctypes.data, p, out.nbytes) == 0, lib.rt_last_error()
    return out


class Ordering:
    """Order buffer and workspace for n rays; the library's order of a device ray list."""

    def __init__(self, lib, n):
        self.lib, self.n = lib, n
        self.work_bytes = rt_host.rays_order_work_bytes(n)
        assert self.work_bytes > 0
        self.d_order = lib.rt_alloc_device(0, 4 * n)
        self.d_work = lib.rt_alloc_device(0, self.work_bytes)
        assert self.d_order and self.d_work, lib.rt_last_error()

    def run(self, r, d_rays):
        r.order_rays(self.n, d_rays, self.d_order, self.d_work, self.work_bytes)
        return download(self.lib, self.d_order, self.n, np.uint32)      # (rt_copy_to_host waits for the device)

    def close(self):
        self.lib.rt_free_device(0, self.d_order)
        self.lib.rt_free_device(0, self.d_work)


def order_of(lib, r, rays):
    d_rays = upload(lib, np.ascontiguousarray(rays, np.float64))
    o = Ordering(lib, len(rays))
    try:
        first = o.run(r, d_rays)
        again = o.run(r, d_rays)
        assert np.array_equal(first, again), "two calls, two orders"
        return first
    finally:
        o.close()
        lib.rt_free_device(0, d_rays)


def shuffled(rays, seed):
    return np.ascontiguousarray(rays[np.random.default_rng(seed).permutation(len(rays))])


def mixed_list(scene, w, h, cams_seed, shuffle_seed):
    """A frame's primary rays and 2000 micro-camera rays in one list, shuffled by a fixed permutation."""
    cams = ru.draw_cameras(scene, 500, cams_seed)
    rays = np.concatenate([rt_host.primary_rays(w, h, scene), ru.micro_rays(cams, float(scene.get("fovDeg", 60)))])
    return shuffled(rays, shuffle_seed)


# ------------------------------------------------------------------ 1. the order is a permutation, the same on every call
def test_order_is_a_permutation_of_a_shuffled_frame(lib):
    scene = rt_host.load_scene("h8")
    rays = shuffled(rt_host.primary_rays(200, 120, scene), 5)
    r = rt_host.Renderer(scene, 0, lib)
    try:
        order = order_of(lib, r, rays)
    finally:
        r.close()
    assert np.array_equal(np.sort(order), np.arange(len(rays), dtype=np.uint32))
    assert not np.array_equal(order, np.arange(len(rays), dtype=np.uint32))


@pytest.mark.parametrize("n", [1, 63, 65, 2 ** 18 + 5])
def test_order_is_a_permutation_at_any_size(lib, n):
    scene = rt_host.load_scene("h8")
    rays = shuffled(rt_host.primary_rays(640, 412, scene), 6)[:n]
    assert len(rays) == n
    r = rt_host.Renderer(scene, 0, lib)
    try:
        order = order_of(lib, r, rays)
    finally:
        r.close()
    assert np.array_equal(np.sort(order), np.arange(n, dtype=np.uint32))


def test_identical_rays_and_non_finite_rays(lib):
    scene = rt_host.load_scene("default14")
    r = rt_host.Renderer(scene, 0, lib)
    try:
        n = 5000
        same = np.tile(np.array([0.0, 1.5, 10.0, 0.0, 0.0, -1.0]), (n, 1))
        order = order_of(lib, r, same)
        assert np.array_equal(np.sort(order), np.arange(n, dtype=np.uint32))
        assert np.array_equal(order, np.arange(n, dtype=np.uint32))             # equal keys keep list order: the sort is stable
        rays = mixed_list(scene, 64, 40, 21, 22)
        bad = np.arange(7, len(rays), 41)
        for j, k in enumerate(bad):
            rays[k, j % 6] = (math.nan, math.inf, -math.inf)[j % 3]
        order = order_of(lib, r, rays)
        assert np.array_equal(np.sort(order), np.arange(len(rays), dtype=np.uint32))
        assert set(order[-len(bad):].tolist()) == set(bad.tolist())               # they end the order
        everything_bad = np.full((130, 6), math.nan)
        order = order_of(lib, r, everything_bad)
        assert np.array_equal(np.sort(order), np.arange(130, dtype=np.uint32))
    finally:
        r.close()


# ------------------------------------------------------------------ 1b. an exact yardstick for an order above 2^20 rays
# The bounds and key kernels run on a capped grid (csrc/rt_rays_order.h: rt_order_grid) and reach the rays beyond it with a grid-stride
# loop; rt_order_scan carries across chunks of 256 tiles.  The list below needs both; tests/test_rays_order.py holds its sizes against the
# library's own grid and tile count, without a GPU.  frame: w x h = m primary rays; extra: the displaced rays behind two copies of them.
ORDER_BEYOND = {"scene": "h8", "w": 1024, "h": 512, "extra": 4096 + 5}


def beyond_lists(scene):
    """-> (B, T, T'): the shuffled primary rays of the frame; `extra` more of them (another shuffle's first) with their origins
    displaced by 20..60 units along each axis, both signs on each; and the same without the displacement."""
    c = ORDER_BEYOND
    every = rt_host.primary_rays(c["w"], c["h"], scene)
    b = shuffled(every, 91)
    plain = shuffled(every, 92)[:c["extra"]].copy()
    rng = np.random.default_rng(93)
    moved = plain.copy()
    moved[:, 0:3] += rng.uniform(20.0, 60.0, (len(plain), 3)) * rng.choice([-1.0, 1.0], (len(plain), 3))
    return b, moved, plain


def test_order_beyond_one_turn_is_the_order_of_the_same_rays_in_one_turn(lib):
    """full = B ++ B ++ T, more than 2^20 rays and more than 256 tiles: every ray of T lies where only the second turn of rt_order_bounds
    and rt_order_keys reaches it, and T alone gives the origin coordinates an extent.  Y = B ++ T is the same set of rays - the same
    bounds, the same keys - in one turn and 130 tiles.  The order is the list sorted by (key, index), so full's order restricted to the
    first copy and T is Y's, element for element, and its second copy follows its first."""
    scene = rt_host.load_scene(ORDER_BEYOND["scene"])
    b, t, t_plain = beyond_lists(scene)
    m, k = len(b), len(t)
    full, y = np.concatenate([b, b, t]), np.concatenate([b, t])
    n = len(full)
    assert n == 2 * m + k > 2 ** 20 and 2 * m >= 2 ** 20 > m + k
    assert (np.abs(t[:, 0:3] - b[0, 0:3]) > 19.0).all() and (t[:, 0:3] > b[0, 0:3]).any(axis=0).all() and (t[:, 0:3] < b[0, 0:3]).any(axis=0).all()
    assert (b[:, 0:3] == b[0, 0:3]).all()                               # one origin: within B the origin decides nothing
    r = rt_host.Renderer(scene, 0, lib)
    try:
        o_full, o_y, o_plain = order_of(lib, r, full), order_of(lib, r, y), order_of(lib, r, np.concatenate([b, t_plain]))
        assert np.array_equal(np.sort(o_full), np.arange(n, dtype=np.uint32))
        assert np.array_equal(np.sort(o_y), np.arange(m + k, dtype=np.uint32))
        assert not np.array_equal(o_y, o_plain)                         # T moves the keys at all: bounds that never saw T would show
        first_and_t = o_full[(o_full < m) | (o_full >= 2 * m)].astype(np.int64)
        first_and_t = np.where(first_and_t >= 2 * m, first_and_t - m, first_and_t)
        differ = np.flatnonzero(first_and_t != o_y)
        assert differ.size == 0, ("entries that differ from the one-turn order", differ.size, differ[:8].tolist())
        second = o_full[(o_full >= m) & (o_full < 2 * m)].astype(np.int64) - m
        assert np.array_equal(second, o_full[o_full < m])
        plain, ordered = both_ways(lib, r, full)
    finally:
        r.close()
    assert_same(plain, ordered, "beyond one turn")
    assert len({bytes(p) for p in plain["rgba"][::997]}) > 50          # not all sky


# ------------------------------------------------------------------ 2. ordered results are the plain results
def both_ways(lib, r, rays, order=None):
    """-> (plain, ordered): {output: array} of rt_scene_trace_rays_device and of the ordered trace (the library's order, or `order`),
    both into canary-framed buffers prefilled with the canary."""
    n = len(rays)
    plain, ordered = DeviceRays(lib, rays), DeviceRays(lib, rays)
    o = Ordering(lib, n)
    d_given = upload(lib, np.ascontiguousarray(order, np.uint32)) if order is not None else None
    try:
        plain.run(r)
        if order is None:
            o.run(r, ordered.d_rays)
        r.trace_rays_ordered(n, ordered.d_rays, d_given or o.d_order, ordered.ptr("rgb"), ordered.ptr("rgba"), ordered.ptr("hits"))
        keys = ("rgb", "rgba", "hits")
        return {k: plain.read(k) for k in keys}, {k: ordered.read(k) for k in keys}
    finally:
        plain.close()
        ordered.close()
        o.close()
        if d_given:
            lib.rt_free_device(0, d_given)


def assert_same(a, b, what):
    for k in ("rgb", "rgba", "hits"):
        assert a[k].tobytes() == b[k].tobytes(), (what, k, int((a[k].reshape(len(a[k]), -1) != b[k].reshape(len(b[k]), -1)).any(axis=1).sum()))


@pytest.mark.parametrize("name,seed", [("h8", None), ("default14", None), ("cfg2", None), ("lcg64", None), ("default14_stars", 0), ("default14_stars", 7)])
def test_ordered_trace_is_the_plain_trace(lib, name, seed):
    scene = rt_host.load_scene(name)
    if seed is not None:
        scene = dict(scene, starsSeed=seed)
    rays = mixed_list(scene, 96, 54, 100 + len(name), 200 + len(name))
    r = rt_host.Renderer(scene, 0, lib)
    try:
        plain, ordered = both_ways(lib, r, rays)
    finally:
        r.close()
    assert_same(plain, ordered, (name, seed))
    assert len({bytes(p) for p in plain["rgba"]}) > 50                      # not all sky
    if name == "default14_stars":
        # the stars show, and they hang on a ray's index: the same rays at other indices draw another sky
        other = rt_host.trace_rays(scene, np.ascontiguousarray(rays[::-1]), want=("rgba",))["rgba"][::-1]
        assert (other != plain["rgba"]).any()


# ------------------------------------------------------------------ 3. ... and the restatement's, without the plain path in between
@pytest.mark.parametrize("name", ["default14", "random3"])
def test_binned_rays_match_the_restatement(lib, name):
    scene = SCENES[name]()
    cams = ru.draw_cameras(scene, 500, 1000 + len(name), outside_radius=5000.0 if name == "default14" else None)
    oracle = ru.MicroOracle(scene)
    rays = ru.micro_rays(cams, oracle.fov)
    want_rgba, roots = oracle.expected(cams)
    got = rt_host.trace_rays(scene, rays, want=("rgba", "hits"), order="binned")
    diff = got["rgba"] != want_rgba
    print("BINNED %s: %d rays, %d of %d channels differ from the restatement" % (name, len(rays), int(diff.sum()), diff.size))
    assert not diff.any(), (name, np.argwhere(diff)[:8].tolist())
    bad = [j for j in range(len(rays)) if not ru.hits_equal(got["hits"][j], oracle.hit_of(roots[j]))]
    assert not bad, (name, bad[:8])


# ------------------------------------------------------------------ 4. the caller's own orders
def test_caller_made_orders(lib):
    scene = rt_host.load_scene("default14")
    rays = mixed_list(scene, 64, 40, 31, 32)
    n = len(rays)
    r = rt_host.Renderer(scene, 0, lib)
    try:
        for what, order in (("identity", np.arange(n)), ("reversed", np.arange(n)[::-1]), ("random", np.random.default_rng(33).permutation(n))):
            plain, ordered = both_ways(lib, r, rays, order=order)
            assert_same(plain, ordered, what)
    finally:
        r.close()


def test_out_of_range_entries_are_skipped(lib):
    """Entries equal to n name no ray: exactly the rays no entry names keep the sentinel their outputs were prefilled with.  The ray
    list and the outputs are one record longer than n, so nothing here can touch memory outside an allocation whatever a kernel does."""
    scene = rt_host.load_scene("default14")
    rays = mixed_list(scene, 64, 40, 41, 42)
    n = len(rays) - 1                                                  # the list's last record is the spare one
    order = np.random.default_rng(43).permutation(n).astype(np.uint32)
    dropped = order[5::17].copy()                                      # the rays whose entries are replaced
    order[5::17] = n
    r = rt_host.Renderer(scene, 0, lib)
    plain, ordered = DeviceRays(lib, rays), DeviceRays(lib, rays)       # (n + 1 records each; prefilled with the canary byte)
    d_order = upload(lib, order)
    try:
        r.trace_rays(n, plain.d_rays, plain.ptr("rgb"), plain.ptr("rgba"), plain.ptr("hits"))
        r.trace_rays_ordered(n, ordered.d_rays, d_order, ordered.ptr("rgb"), ordered.ptr("rgba"), ordered.ptr("hits"))
        keep = np.ones(n + 1, bool)
        keep[dropped] = False
        keep[n] = False
        for k in ("rgb", "rgba", "hits"):
            a, b = plain.read(k), ordered.read(k)
            a, b = a.reshape(n + 1, -1).view(np.uint8), b.reshape(n + 1, -1).view(np.uint8)
            assert a[keep].tobytes() == b[keep].tobytes(), k
            assert (b[~keep] == 0x5A).all(), k                          # untouched: the prefill (test_gpu_rays.CANARY)
            assert (a[n] == 0x5A).all(), k
    finally:
        plain.close()
        ordered.close()
        lib.rt_free_device(0, d_order)
        r.close()


# ------------------------------------------------------------------ 5. an order outlives an edit of the scene
def test_an_order_is_reused_after_an_orbit_step(lib):
    scene = rt_host.load_scene("default14")
    textures = scene["textures"]
    scene = json.loads(json.dumps({k: v for k, v in scene.items() if k != "textures"}))       # (a copy this test may edit)
    scene["textures"] = textures
    rays = mixed_list(scene, 64, 40, 51, 52)
    n = len(rays)
    r = rt_host.Renderer(scene, 0, lib)
    plain, ordered = DeviceRays(lib, rays), DeviceRays(lib, rays)
    o = Ordering(lib, n)
    try:
        o.run(r, ordered.d_rays)
        plain.run(r)
        before = plain.read("rgba")
        i = next(i for i, ob in enumerate(scene["objects"]) if ob["r2"] < 1e4 and ob["mtl"]["albedo"][4] > 0)
        c0 = list(scene["objects"][i]["origin"])
        scene["objects"][i]["origin"] = [c0[0] + 0.5 * math.cos(0.4), c0[1], c0[2] + 0.5 * math.sin(0.4)]
        obu.set_objects(r, scene, i, i + 1)
        r.trace_rays_ordered(n, ordered.d_rays, o.d_order, ordered.ptr("rgb"), ordered.ptr("rgba"), ordered.ptr("hits"))
        plain.run(r)
        after = {k: plain.read(k) for k in ("rgb", "rgba", "hits")}
        assert (after["rgba"] != before).any()                            # the move shows
        assert_same(after, {k: ordered.read(k) for k in after}, "after the move")
    finally:
        plain.close()
        ordered.close()
        o.close()
        r.close()


# ------------------------------------------------------------------ 6. the host form, Node
def test_host_form_over_a_chunk_boundary(lib):
    """2^18 + 1000 shuffled rays of a stars scene (one chunk boundary), and 2^19 + 1000 (two, with a whole chunk in the middle whose
    sky is shown to hang on the global index)."""
    scene = rt_host.load_scene("default14_stars")
    every = shuffled(rt_host.primary_rays(1024, 600, scene), 61)
    for n in (2 ** 18 + 1000, 2 ** 19 + 1000):
        rays = every[:n]
        assert len(rays) == n
        listed = rt_host.trace_rays(scene, rays, want=("rgb", "rgba"), order="list")
        binned = rt_host.trace_rays(scene, rays, want=("rgb", "rgba"), order="binned")
        assert binned["rgba"].tobytes() == listed["rgba"].tobytes(), n
        assert binned["rgb"].tobytes() == listed["rgb"].tobytes(), n
    alone = rt_host.trace_rays(scene, rays[2 ** 18:2 ** 19], want=("rgba",))["rgba"]   # the middle chunk's rays at indices 0..: another sky
    assert (alone != listed["rgba"][2 ** 18:2 ** 19]).any()
    few = rt_host.trace_rays(scene, rays[:300], want=("rgba", "hits"), order="binned")
    assert few["rgba"].tobytes() == listed["rgba"][:300].tobytes()
    assert hit_bytes(few["hits"]).tobytes() == hit_bytes(rt_host.trace_rays(scene, rays[:300], want=("hits",))["hits"]).tobytes()


@pytest.mark.skipif(ou.node_path() is None, reason="node not installed")
def test_node_bin_option(lib):
    scene = rt_host.load_scene("default14")
    rays = mixed_list(scene, 32, 20, 71, 72)[:1500]
    out = subprocess.check_output([ou.node_path(), os.path.join(ROOT, "tests", "js_rays_bin_check.js"), PKG, "default14",
                                   base64.b64encode(np.ascontiguousarray(rays).tobytes()).decode()], text=True, timeout=300)
    res = json.loads(out.strip().splitlines()[-1])
    assert res["same"] is True, res
    want = rt_host.trace_rays(scene, rays, want=("rgba",))["rgba"]
    assert res["rgba"] == want.reshape(-1).tolist()


# ------------------------------------------------------------------ 7. the order is an order
def test_a_wave_of_the_order_is_a_small_patch_of_the_frame(lib):
    """The shuffled primary rays of a 256 x 256 frame: every run of 64 consecutive entries of the library's order names rays whose
    pixels fit a small box.  The median box area is held to 1024 pixels: an 8 x 8 block is 64, the row order the plain path is documented
    for 64 x 1, a key that ignores direction gives about the whole frame's 65 536 and one that resolves a single axis thousands - 16
    times the ideal is a cap against a degenerate key, not a tuning target."""
    w = h = 256
    scene = rt_host.load_scene("h8")
    perm = np.random.default_rng(81).permutation(w * h)
    rays = np.ascontiguousarray(rt_host.primary_rays(w, h, scene)[perm])
    r = rt_host.Renderer(scene, 0, lib)
    try:
        order = order_of(lib, r, rays)
    finally:
        r.close()
    assert np.array_equal(np.sort(order), np.arange(w * h, dtype=np.uint32))
    pixel = perm[order]                                                 # the frame pixel of the order's j-th ray
    x, y = (pixel % w).reshape(-1, 64), (pixel // w).reshape(-1, 64)
    area = (x.max(axis=1) - x.min(axis=1) + 1) * (y.max(axis=1) - y.min(axis=1) + 1)
    print("ORDER h8 256x256 shuffled: box area of 64 consecutive entries: median %d, mean %.1f, max %d pixels"
          % (int(np.median(area)), float(area.mean()), int(area.max())))
    assert np.median(area) <= 1024
