"""The soft trace in one launch on the GPU (include/rt_hip.h: rt_scene_trace_rays_soft_device, rt_scene_trace_view_soft_device,
rt_trace_rays_soft_recursive, rt_trace_view_soft).  The recursive kernel is held to code that exists without it: the wavefront loop
rt_trace_rays_soft (rt_host.trace_rays_soft, method "wavefront") and the strict recursive rt_trace_rays (rt_host.trace_rays).  Every
comparison is of bytes, rgb and rgba, on all rays: a node, its light terms and the fold are the wavefront kernels' own operations in
their own order, without FMA contraction.  No tolerance, no ray left out."""
import numpy as np
import pytest

import lighting_util as lu
import nodes_util as nu
import relight_util as rl
import rt_host
import views_util as vu
from test_gpu_views import Views, hip, lib  # noqa: F401  (fixtures; a view with its device twin)

pytestmark = pytest.mark.gpu
SCENES = ["default14", "h8"]
TABLE = lu.turned_sets(4, 2)                              # 8 entries on the unit sphere
RADIUS = 1.0
BASE = 2 ** 40 + 3
WANT = ("rgb", "rgba")


def primary(lib, name):
    """(scene, the 96 x 54 PINHOLE view's rays from the scene's camera), once per scene"""
    scene, rays, n_primary = rl.ray_list(lib, name)
    return scene, np.ascontiguousarray(rays[:n_primary])


def same(got, want, what):
    for k in WANT:
        g, w = got[k], want[k]
        if g.tobytes() != w.tobytes():
            bad = np.flatnonzero((np.ascontiguousarray(g).view(np.uint8).reshape(len(g), -1) != np.ascontiguousarray(w).view(np.uint8).reshape(len(w), -1)).any(axis=1))
            raise AssertionError((what, k, len(bad), int(bad[0]), g[bad[0]].tolist(), w[bad[0]].tolist()))


_cache = {}


def once(key, make):
    """a yardstick computed once, shared by the cases that need it and never written to"""
    if key not in _cache:
        out = make()
        for a in out.values():
            a.setflags(write=False)
        _cache[key] = out
    return _cache[key]


class Soft:
    """A ray list, canary-framed outputs and a table in device memory, and Renderer.trace_rays_soft on them."""

    def __init__(self, lib, r, rays, offs=None, order=None):
        self.lib, self.r, self.n = lib, r, len(rays)
        self.n_offs = 0 if offs is None else len(offs)
        self.d_rays = nu.Dev(lib, self.n * 48, np.asarray(rays, np.float64))
        self.d_rgb, self.d_rgba = nu.Dev(lib, self.n * 24), nu.Dev(lib, self.n * 4)
        self.d_offs = nu.Dev(lib, self.n_offs * 24, np.asarray(offs, np.float64)) if offs is not None else None
        self.d_order = nu.Dev(lib, len(order) * 4, np.asarray(order, np.uint32)) if order is not None else None

    def trace(self, n_samples, radius, first=0, n=None, **kw):
        """rays [first, first + n) of the list, written at their own places in the outputs"""
        n = self.n - first if n is None else n
        return self.r.trace_rays_soft(n, self.d_rays.ptr + 48 * first, self.d_rgb.ptr + 24 * first, self.d_rgba.ptr + 4 * first,
                                      self.d_offs.ptr if self.d_offs else 0, self.n_offs or n_samples, n_samples, radius,
                                      order_ptr=self.d_order.ptr if self.d_order else 0, **kw)

    def read(self):
        return {"rgb": self.d_rgb.read(np.float64).reshape(self.n, 3), "rgba": self.d_rgba.read().reshape(self.n, 4)}

    def close(self):
        for d in (self.d_rays, self.d_rgb, self.d_rgba, self.d_offs, self.d_order):
            if d:
                d.close()


def device_trace(lib, scene, rays, n_samples, radius, offs=None, order=None, **kw):
    r = rt_host.Renderer(scene, 0, lib)
    f = Soft(lib, r, rays, offs=offs, order=order)
    try:
        st = f.trace(n_samples, radius, want_stats=True, **kw)
        assert st.pixels == len(rays) and st.kernel_ms > 0
        return f.read()
    finally:
        f.close()
        r.close()


# ------------------------------------------------------------------ 1. levels and segs
@pytest.mark.parametrize("segs", [0, 1, 2])
@pytest.mark.parametrize("levels", ["0", "1", "depth", "depth+3"])
@pytest.mark.parametrize("name", SCENES)
def test_levels_and_segs(lib, name, levels, segs):
    scene, rays = primary(lib, name)
    depth = scene["segs"]
    assert 2 < depth <= 8
    lv = {"0": 0, "1": 1, "depth": depth, "depth+3": depth + 3}[levels]
    kw = dict(offs=TABLE, stride=1, levels=lv, segs=segs, want=WANT, lib=lib)
    want = once((name, "wavefront", lv, segs), lambda: rt_host.trace_rays_soft(scene, rays, 4, RADIUS, **kw))
    got = rt_host.trace_rays_soft(scene, rays, 4, RADIUS, method="recursive", **kw)
    same(got, want, (name, levels, segs))
    hard = once((name, "hard", segs), lambda: rt_host.trace_rays(scene, rays, segs=segs, want=WANT, method="recursive", lib=lib))
    if lv == 0:
        same(got, hard, (name, "levels 0 is the recursive trace", segs))
    else:
        assert got["rgba"].tobytes() != hard["rgba"].tobytes()                              # (the lights do have a size here)
    # one sample of point lights is the recursive trace at every `levels`
    point = rt_host.trace_rays_soft(scene, rays, 1, 0.0, levels=lv, segs=segs, want=WANT, method="recursive", lib=lib)
    same(point, hard, (name, "one sample, radius 0", levels, segs))


@pytest.mark.parametrize("name", SCENES)
def test_sixteen_samples_of_the_primary_hits(lib, name):
    """levels = 1 with 16 samples, every ray the same 16 entries (stride 0: the scalar-load branch of the table)"""
    scene, rays = primary(lib, name)
    want = rt_host.trace_rays_soft(scene, rays, 16, RADIUS, levels=1, want=WANT, lib=lib)
    got = rt_host.trace_rays_soft(scene, rays, 16, RADIUS, levels=1, want=WANT, method="recursive", lib=lib)
    same(got, want, (name, 16))
    same(rt_host.trace_rays_soft(scene, rays, 16, RADIUS, levels=1, want=WANT, method="recursive", order="binned", lib=lib), want, (name, 16, "binned"))
    hard = once((name, "hard", 0), lambda: rt_host.trace_rays(scene, rays, segs=0, want=WANT, method="recursive", lib=lib))
    differ = (got["rgba"] != hard["rgba"]).any(axis=1)
    print("SOFT %s: %d of %d pixels of the 16-sample frame differ from the hard frame" % (name, int(differ.sum()), len(rays)))
    assert differ.any()


# ------------------------------------------------------------------ 2. the table walk
@pytest.mark.parametrize("stride", [0, 1, 7])
@pytest.mark.parametrize("n_samples,n_offs", [(2, 2), (2, 8), (5, 5), (5, 8)])
@pytest.mark.parametrize("name", SCENES)
def test_the_table_walk(lib, name, n_samples, n_offs, stride):
    """a base no 32-bit index reaches; tables of n_samples and of 8 entries; two levels relit, so a child reads its ROOT ray's entries"""
    scene, rays = primary(lib, name)
    kw = dict(offs=TABLE[:n_offs], stride=stride, base=BASE, levels=2, want=WANT, lib=lib)
    want = rt_host.trace_rays_soft(scene, rays, n_samples, RADIUS, **kw)
    got = rt_host.trace_rays_soft(scene, rays, n_samples, RADIUS, method="recursive", **kw)
    same(got, want, (name, n_samples, n_offs, stride))
    if stride:
        assert len(np.unique(rl.entries(len(rays), n_offs, n_samples, stride, BASE)[:, 0])) == n_offs     # the walk reaches every entry


# ------------------------------------------------------------------ 3. chunk independence
def test_a_list_in_two_pieces_and_an_order(lib):
    """default14_stars: the stars sampler's pix and the table's entry are the ROOT ray's index pix_base + i"""
    scene = rt_host.load_scene("default14_stars")
    rays = rt_host.view_rays(lu.camera_view(scene), rl.W, rl.H, lib=lib).reshape(-1, 6)
    n, depth = len(rays), scene["segs"]
    kw = dict(stride=7, base=BASE, levels=depth)
    want = rt_host.trace_rays_soft(scene, rays, 3, RADIUS, offs=TABLE, want=WANT, lib=lib, **kw)
    whole = device_trace(lib, scene, rays, 3, RADIUS, offs=TABLE, **kw)
    same(whole, want, "one call")
    half = n // 2 + 1                                        # (odd: with stride 7 over 8 entries the second piece's own indices walk other entries)
    r = rt_host.Renderer(scene, 0, lib)
    f = Soft(lib, r, rays, offs=TABLE)
    try:
        f.trace(3, RADIUS, first=0, n=half, pix_base=0, **kw)
        f.trace(3, RADIUS, first=half, pix_base=half, **kw)
        same(f.read(), whole, "two pieces with pix_base")
        f.trace(3, RADIUS, first=half, pix_base=0, **kw)
        assert f.read()["rgba"].tobytes() != whole["rgba"].tobytes()                        # (pix_base does decide bytes)
    finally:
        f.close()
        r.close()
    perm = np.random.default_rng(3).permutation(n).astype(np.uint32)
    same(device_trace(lib, scene, rays, 3, RADIUS, offs=TABLE, order=perm, **kw), whole, "a permuted order")


# ------------------------------------------------------------------ 4. edges of the kernel
@pytest.mark.parametrize("n", [1, 63, 64, 65, 256, 257])
def test_edges_of_the_launch(lib, n):
    scene, all_rays = primary(lib, "default14")
    rays = np.ascontiguousarray(all_rays[1500::max(1, (len(all_rays) - 1500) // n)][:n])
    assert len(rays) == n
    kw = dict(stride=1, base=5, levels=2)
    want = rt_host.trace_rays_soft(scene, rays, 3, RADIUS, offs=TABLE[:4], want=WANT, lib=lib, **kw)
    got = device_trace(lib, scene, rays, 3, RADIUS, offs=TABLE[:4], **kw)                   # (read() checks the canaries around rgb and rgba)
    same(got, want, n)
    # an entry >= n names no ray: nothing is written for the ray it stands for
    perm = np.random.default_rng(n).permutation(n).astype(np.uint32)
    holed = perm.copy()
    holed[n // 2] = n + 5
    part = device_trace(lib, scene, rays, 3, RADIUS, offs=TABLE[:4], order=holed, **kw)
    skipped = int(perm[n // 2])
    keep = np.arange(n) != skipped
    assert part["rgba"][keep].tobytes() == want["rgba"][keep].tobytes() and part["rgb"][keep].tobytes() == want["rgb"][keep].tobytes()
    assert (part["rgba"][skipped] == nu.CANARY).all()


def test_rays_that_are_not_finite(lib):
    scene, all_rays = primary(lib, "default14")
    rays = all_rays[2000:2300].copy()
    rays[7, 4], rays[64, 0], rays[130, 5] = np.nan, np.inf, -np.inf
    kw = dict(stride=1, levels=2)
    want = rt_host.trace_rays_soft(scene, rays, 3, RADIUS, offs=TABLE[:4], want=WANT, lib=lib, **kw)
    got = device_trace(lib, scene, rays, 3, RADIUS, offs=TABLE[:4], **kw)
    same(got, want, "NaN and Inf rays")
    for i in (7, 64, 130):
        assert np.isnan(got["rgb"][i]).all() and got["rgba"][i].tolist() == [0, 0, 0, 255]


def test_a_ray_that_starts_inside_the_glass_sphere(lib):
    scene, _ = primary(lib, "default14")
    glass = [o for o in scene["objects"] if o["mtl"]["albedo"][4] > 0]
    assert glass
    c = np.array(glass[0]["origin"], np.float64)
    dirs = vu.unit_rows(np.random.default_rng(9).normal(size=(130, 3)))
    rays = np.concatenate([np.broadcast_to(c, dirs.shape) + 0.25 * float(np.sqrt(glass[0]["r2"])) * dirs[::-1], dirs], axis=1)
    kw = dict(stride=1, levels=scene["segs"])
    want = rt_host.trace_rays_soft(scene, rays, 3, RADIUS, offs=TABLE[:4], want=WANT, lib=lib, **kw)
    same(device_trace(lib, scene, rays, 3, RADIUS, offs=TABLE[:4], **kw), want, "from inside the glass")
    assert len(np.unique(want["rgba"], axis=0)) > 8


def _sixteen_lights():
    rng = np.random.default_rng(16)
    return np.concatenate([rng.uniform(-8, 8, (16, 1)), rng.uniform(3, 12, (16, 1)), rng.uniform(-8, 8, (16, 1))], axis=1).tolist()


EDGES = {
    "no lights": lambda s: rl.copy_of(s, lights=[]),
    "16 lights": lambda s: rl.copy_of(s, lights=_sixteen_lights(), light_intensity=9),
    "no skybox": lambda s: rl.copy_of(s, objects=rl.copy_of(s)["objects"][:-1]),
    "depth 0": lambda s: rl.copy_of(s, segs=0),
}


@pytest.mark.parametrize("edge", sorted(EDGES))
def test_edges_of_the_scene(lib, edge):
    base_scene, all_rays = primary(lib, "default14")
    rays = np.ascontiguousarray(all_rays[::3])
    scene = EDGES[edge](base_scene)
    kw = dict(stride=1, levels=2)
    want = rt_host.trace_rays_soft(scene, rays, 3, RADIUS, offs=TABLE[:4], want=WANT, lib=lib, **kw)
    same(device_trace(lib, scene, rays, 3, RADIUS, offs=TABLE[:4], **kw), want, edge)
    same(rt_host.trace_rays_soft(scene, rays, 3, RADIUS, offs=TABLE[:4], want=WANT, method="recursive", lib=lib, **kw), want, (edge, "host form"))
    if edge == "depth 0":
        assert not want["rgb"].any() and (want["rgba"] == [0, 0, 0, 255]).all()
    else:
        assert len(np.unique(want["rgba"], axis=0)) > 8


def test_edits_between_two_calls_take_effect(lib):
    scene, all_rays = primary(lib, "default14")
    rays = np.ascontiguousarray(all_rays[::3])
    edited = rl.copy_of(scene, lights=[[4.0, 9.0, 6.0], [-5.0, 8.0, 1.0]], light_intensity=30)
    kw = dict(stride=1, levels=2)
    before = rt_host.trace_rays_soft(scene, rays, 3, RADIUS, offs=TABLE[:4], want=WANT, lib=lib, **kw)
    after = rt_host.trace_rays_soft(edited, rays, 3, RADIUS, offs=TABLE[:4], want=WANT, lib=lib, **kw)
    assert before["rgba"].tobytes() != after["rgba"].tobytes()
    r = rt_host.Renderer(scene, 0, lib)
    f = Soft(lib, r, rays, offs=TABLE[:4])
    try:
        f.trace(3, RADIUS, **kw)
        same(f.read(), before, "before the edits")
        r.set_lights(edited["lights"])
        r.set_light_intensity(30)
        f.trace(3, RADIUS, **kw)
        same(f.read(), after, "after set_lights and set_light_intensity")
    finally:
        f.close()
        r.close()


# ------------------------------------------------------------------ 5. the view form
@pytest.mark.parametrize("model", [vu.PINHOLE, vu.EQUIRECT])
def test_the_view_form(lib, hip, model):  # noqa: F811
    scene = rt_host.load_scene("default14")
    w, h = rl.W, rl.H
    cam = scene["camera"]
    v = Views(lib, hip, model, w, h, cam=(cam["origin"], cam["axisX"], cam["axisY"], cam["axisZ"]), fov=scene["fovDeg"])
    kw = dict(stride=1, levels=2)
    try:
        want = rt_host.trace_view_soft(scene, v.host, w, h, 3, RADIUS, offs=TABLE, want=WANT, lib=lib, **kw)
        assert len(np.unique(want["rgba"], axis=0)) > 8
        same(rt_host.trace_view_soft(scene, v.host, w, h, 3, RADIUS, offs=TABLE, want=WANT, method="recursive", lib=lib, **kw), want, (model, "host form"))
        preferred = rt_host.soft_view_work_bytes(w, h, lib)
        assert preferred == 48 * w * h
        r = rt_host.Renderer(scene, 0, lib)
        d_offs = nu.Dev(lib, TABLE.nbytes, TABLE)
        try:
            for work_bytes in (48 * w, 3 * 48 * w, preferred):
                d_rgb, d_rgba, d_work = nu.Dev(lib, w * h * 24), nu.Dev(lib, w * h * 4), nu.Dev(lib, work_bytes)
                try:
                    st = r.trace_view_soft(v.dev, w, h, d_rgb.ptr, d_rgba.ptr, d_offs.ptr, len(TABLE), 3, RADIUS, d_work.ptr, work_bytes, want_stats=True, **kw)
                    assert st.pixels == w * h
                    d_work.read()                            # (its canaries)
                    got = {"rgb": d_rgb.read(np.float64).reshape(-1, 3), "rgba": d_rgba.read().reshape(-1, 4)}
                    same(got, want, (model, work_bytes))
                finally:
                    for d in (d_rgb, d_rgba, d_work):
                        d.close()
        finally:
            d_offs.close()
            r.close()
    finally:
        v.close()
