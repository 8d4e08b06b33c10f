"""Gathered light on the GPU (include/rt_hip.h: struct rt_gather).  The fused kernel is held to a value built only from calls that exist
without it (tests/gather_util.py): per sample the host probe's segments, traced by Renderer.trace_rays_soft at levels 0 with one sample
of point lights and pix_base = pix_base + s pix_stride, folded in numpy in the stated order, through the store rule.  Every comparison
is of bytes: the segment is rt_ambient.h's own source, a gathered ray's colour is the soft kernel's own walk, the fold is binary64
additions in a fixed order and one correctly rounded division.  No tolerance, no receiver left out.

Receivers: the hit records of a 96 x 54 pinhole at the reference's camera on default14, default14_stars, h8 and h8 without its skybox,
plus the hand-built records (inside a sphere, a miss, NaN records), as tests/test_gpu_ambient.py makes them."""
import json

import numpy as np
import pytest

import ambient_util as au
import gather_util as gu
import rt_host
import views_util as vu
from test_gpu_ambient import CONFIGS, H, SENTINEL_F64, SENTINEL_U32, W, receivers, the_scene
from test_gpu_views import CANARY, Dev, Views, hip, lib, upload  # noqa: F401  (lib and hip are fixtures)

pytestmark = pytest.mark.gpu
WALK = (16, 64, 7)                                             # the config the other scenes, depths and cases use: a walk that wraps
WANT = ("rgb", "rgba")


class Fused:
    """Receivers and a table in device memory, canary-framed outputs, and Renderer.gather on them."""

    def __init__(self, lib, hip, hits, dirs):
        self.lib, self.n, self.n_dirs = lib, len(hits), len(dirs)
        self.d_hits, self.d_dirs = upload(lib, hip, hits), upload(lib, hip, dirs)
        self.rgb, self.rgba = Dev(lib, self.n * 24), Dev(lib, self.n * 4)
        self.extra = []

    def reset(self):
        for d in (self.rgb, self.rgba):
            assert self.lib.rt_memset_device(0, d.p, CANARY, d.n) == 0

    def run(self, r, n_samples, stride, want=WANT, n=None, first=0, **kw):
        """receivers [first, first + n) of the list, written at their own places in the outputs"""
        n = self.n - first if n is None else n
        return r.gather(n, self.d_hits + 80 * first, self.d_dirs, self.n_dirs, n_samples, self.rgb.p + 24 * first if "rgb" in want else 0,
                        self.rgba.p + 4 * first if "rgba" in want else 0, stride=stride, **kw)

    def read(self):
        return self.rgb.read(np.float64).reshape(self.n, 3), self.rgba.read(np.uint32)

    def close(self):
        self.rgb.close(); self.rgba.close()
        for p in [self.d_hits, self.d_dirs] + self.extra:
            self.lib.rt_free_device(0, p)


def same(got, want, what):
    for g, w, k in zip(got, want, WANT):
        g, w = np.ascontiguousarray(g), np.ascontiguousarray(w)
        assert g.dtype == w.dtype and g.shape == w.shape, (what, k, g.dtype, w.dtype, g.shape, w.shape)
        diff = g.view(np.uint8).reshape(len(g), -1) != w.view(np.uint8).reshape(len(w), -1)
        if diff.any():
            bad = np.flatnonzero(diff.any(axis=1))
            raise AssertionError((what, k, len(bad), int(bad[0]), g[bad[0]].tolist(), w[bad[0]].tolist()))


def mixed_slice(lib):
    """Scanned receivers (glass among them), misses and records with a non-finite word, next to each other."""
    _, nosky = receivers(lib, "nosky")
    _, d14 = receivers(lib, "default14")
    mix = np.concatenate([au.hand_built(), nosky[W * 20:W * 20 + 150], d14[W * 30:W * 30 + 150]])
    ok = au.scanned(mix)
    assert 0 < ok.sum() < len(mix) and not ok[2:5].any() and ok[0:2].all() and ok[5] and (mix["object"][6:156] < 0).any() and len(mix) >= 259
    return mix


# ------------------------------------------------------------------ 0. what a CPU can say of the inputs
def test_the_inputs_are_what_the_cases_need(lib):
    """The record mix and the table walk's wrap, before anything is gathered."""
    mix = mixed_slice(lib)
    assert (mix["inside"] != 0).any()
    n_samples, n_dirs, stride = WALK
    e = [au.entry(0, i, stride, s, n_dirs) for i in range(W * H) for s in (0, n_samples - 1)]
    assert max(e) == n_dirs - 1 and min(e) == 0 and any((i * stride + n_samples - 1) >= n_dirs for i in range(W * H))      # the walk wraps
    big = 2 ** 40 + 3
    assert au.entry(big, 0, stride, 0, n_dirs) != au.entry(0, 0, stride, 0, n_dirs)


# ------------------------------------------------------------------ 1. the fused kernel against the fold of the soft trace over the probe's segments
CASES = [("default14", c, 0) for c in CONFIGS] + [("default14", WALK, 1), ("default14", WALK, 2)] + [(n, WALK, 0) for n in ("default14_stars", "h8", "nosky")]


@pytest.mark.parametrize("name,config,segs", CASES, ids=["%s-%d_%d_%d-segs%d" % ((n,) + c + (s,)) for n, c, s in CASES])
def test_fused_is_the_fold_of_the_soft_trace_over_the_probes_segments(lib, hip, name, config, segs):
    scene, hits = receivers(lib, name)
    n_samples, n_dirs, stride = config
    dirs = rt_host.ambient_dirs(n_dirs)
    r = rt_host.Renderer(scene, 0, lib)
    f = Fused(lib, hip, hits, dirs)
    try:
        rgb, rgba, c, obj = gu.by_soft(lib, hip, r, hits, dirs, n_samples, stride=stride, segs=segs, objects=True)
        f.reset()
        st = f.run(r, n_samples, stride, segs=segs, want_stats=True)
        assert st.pixels == len(hits) and st.kernel_ms > 0
        got = f.read()
        same(got, (rgb, rgba), (name, config, segs))
        ok = au.scanned(hits)
        assert np.isnan(rgb[~ok]).all() and (rgba[~ok] == 0xff000000).all() and (rgba >> 24 == 255).all()
        assert not np.isnan(rgb[ok]).any() and len(set(rgba.tolist())) > 16                    # a picture, not a constant
        # the host form gives the device form's bytes
        host = rt_host.gather(scene, hits, n_samples, dirs=dirs, stride=stride, segs=segs, want=WANT, lib=lib)
        same((host["rgb"], host["rgba"].view(np.uint32).reshape(-1)), got, (name, "host form", config, segs))
        # so that no case is vacuous: from the yardstick's side alone
        objs = scene["objects"]
        sky = next(i for i, o in enumerate(objs) if o["r2"] >= 1e7) if name != "nosky" else -2
        depth = segs or scene["segs"]
        if name == "default14" and config == WALK:
            glass = [i for i, o in enumerate(objs) if o["mtl"]["albedo"][3] > 0 and o["mtl"]["albedo"][4] > 0]
            n_glass = int(np.isin(obj, glass).sum())
            print("GATHER default14 %dx%d, %d samples, segs %d: %d gathered rays meet a sphere that reflects and refracts, %d the skybox"
                  % (W, H, n_samples, segs, n_glass, int((obj == sky).sum())))
            assert (obj == sky).any()
            if depth >= 2:
                assert glass and n_glass > 0                                                   # both children are visited: the stack is used
        if name == "default14_stars":
            stars = (obj == sky) & (c[:, :, 0] != 0.0)
            print("GATHER default14_stars: %d gathered rays meet a star" % int(stars.sum()))
            assert objs[sky]["mtl"]["sampler"]["kind"] == 3 and stars.any()
        if name == "nosky":
            assert ((obj < 0) & ok[None, :]).sum() > 1000                                      # gathered rays that miss
            assert (~ok).sum() > 100 and np.isnan(rgb[-4:-1]).all()                              # misses, and the hand-built NaN records
    finally:
        f.close()
        r.close()


# ------------------------------------------------------------------ 2. a base above 2^40; short lists; orders, NULL outputs, sentinels
def test_a_large_base_and_short_lists(lib, hip):
    """Lists of 1, 63, 64, 65, 256 and 257 receivers (a wave less one, a wave, a wave and one, a workgroup, a second workgroup with one
    live lane) from two places of the mixed slice, with base above 2^40."""
    scene = the_scene("default14")
    mix = mixed_slice(lib)
    n_samples, n_dirs, stride = 5, 64, 7
    base = 2 ** 40 + 3
    dirs = rt_host.ambient_dirs(n_dirs)
    r = rt_host.Renderer(scene, 0, lib)
    f = Fused(lib, hip, mix, dirs)
    try:
        first_rgb = {}
        for first in (0, 2):
            rgb, rgba, _ = gu.by_soft(lib, hip, r, mix[first:first + 257], dirs, n_samples, stride=stride, base=base, pix_stride=0)
            assert np.isnan(rgb).any() and not np.isnan(rgb).all()                             # the slice holds a receiver whose mean is NaN
            first_rgb[first] = rgb
            for n in (1, 63, 64, 65, 256, 257):
                f.reset(); f.run(r, n_samples, stride, n=n, first=first, base=base, pix_stride=0)
                got = f.read()
                same([g[first:first + n] for g in got], (rgb[:n], rgba[:n]), (first, n))
                assert (got[0].view(np.uint64)[:first] == SENTINEL_F64).all() and (got[0].view(np.uint64)[first + n:] == SENTINEL_F64).all()
                assert (got[1][:first] == SENTINEL_U32).all() and (got[1][first + n:] == SENTINEL_U32).all()
        no_base, _, _ = gu.by_soft(lib, hip, r, mix[:257], dirs, n_samples, stride=stride, pix_stride=0)
        assert au.bits(no_base).tobytes() != au.bits(first_rgb[0]).tobytes()                   # (the base does reach the table)
    finally:
        f.close()
        r.close()


def test_orders_and_null_outputs(lib, hip):
    scene = the_scene("default14")
    hits = mixed_slice(lib)
    n = len(hits)
    n_samples, n_dirs, stride = 5, 64, 7
    dirs = rt_host.ambient_dirs(n_dirs)
    r = rt_host.Renderer(scene, 0, lib)
    f = Fused(lib, hip, hits, dirs)
    try:
        want = gu.by_soft(lib, hip, r, hits, dirs, n_samples, stride=stride)[:2]
        f.reset(); f.run(r, n_samples, stride)
        same(f.read(), want, "the list's order")
        # reversed, with one entry >= n: the receiver it stood for keeps the sentinel
        order = np.arange(n, dtype=np.uint32)[::-1].copy()
        dropped = int(order[7])
        order[7] = n
        f.extra.append(upload(lib, hip, order))
        f.reset(); f.run(r, n_samples, stride, order_ptr=f.extra[-1])
        got = f.read()
        named = np.arange(n) != dropped
        same([g[named] for g in got], [w[named] for w in want], "reversed, one entry names no receiver")
        assert (got[0][dropped].view(np.uint64) == SENTINEL_F64).all() and got[1][dropped] == SENTINEL_U32
        # each output alone is itself with the other; the other keeps the sentinel
        for i, k in enumerate(WANT):
            f.reset(); f.run(r, n_samples, stride, want=(k,))
            got = f.read()
            same([got[i]], [want[i]], k + " alone")
            assert (got[1 - i].view(np.uint8) == CANARY).all(), k
    finally:
        f.close()
        r.close()


# ------------------------------------------------------------------ 3. the stars sampler's pix
def test_the_stars_pix_of_a_sample_and_a_list_in_pieces(lib, hip):
    scene, hits = receivers(lib, "default14_stars")
    n = len(hits)
    n_samples, n_dirs, stride = 5, 64, 7
    dirs = rt_host.ambient_dirs(n_dirs)
    r = rt_host.Renderer(scene, 0, lib)
    f = Fused(lib, hip, hits, dirs)
    try:
        f.reset(); f.run(r, n_samples, stride, pix_base=11)                     # pix_stride None: n
        whole = f.read()
        same(whole, gu.by_soft(lib, hip, r, hits, dirs, n_samples, stride=stride, pix_base=11)[:2], "pix_stride n")
        f.reset(); f.run(r, n_samples, stride, pix_base=11, pix_stride=0)
        flat = f.read()
        same(flat, gu.by_soft(lib, hip, r, hits, dirs, n_samples, stride=stride, pix_base=11, pix_stride=0)[:2], "pix_stride 0")
        assert whole[0].tobytes() != flat[0].tobytes()                          # every sample its own stars, or all the same ones
        # two pieces with base and pix_base advanced (and the whole list's pix_stride) are one call
        cut = 64 * 37 + 5
        f.reset()
        f.run(r, n_samples, stride, n=cut, pix_base=11, pix_stride=n)
        f.run(r, n_samples, stride, first=cut, base=cut, pix_base=11 + cut, pix_stride=n)
        same(f.read(), whole, "two pieces")
    finally:
        f.close()
        r.close()


# ------------------------------------------------------------------ 4. edits of the resident scene
def test_a_moved_sphere_a_moved_light_and_a_new_seed_take_effect(lib, hip):
    scene, hits = receivers(lib, "default14_stars")
    scene = dict(json.loads(json.dumps({k: v for k, v in scene.items() if k != "textures"})), textures=scene["textures"])      # (a copy to edit)
    n_samples, n_dirs, stride = 5, 64, 7
    dirs = rt_host.ambient_dirs(n_dirs)
    objs = scene["objects"]
    k = next(i for i, o in enumerate(objs) if o["r2"] == 1 and o["mtl"]["albedo"][4] == 0)
    r = rt_host.Renderer(scene, 0, lib)
    f = Fused(lib, hip, hits, dirs)
    try:
        f.reset(); f.run(r, n_samples, stride)
        last = f.read()
        same(last, gu.by_soft(lib, hip, r, hits, dirs, n_samples, stride=stride)[:2], "before")
        objs[k]["origin"] = [objs[k]["origin"][0] + 0.75, objs[k]["origin"][1] + 0.5, objs[k]["origin"][2] + 0.25]
        lights = [list(p) for p in scene["lights"]]
        lights[0] = [lights[0][0] - 3.0, lights[0][1], lights[0][2] + 1.0]
        for what, edit in (("a moved sphere", lambda: r.set_objects(objs[k:k + 1], k)), ("a moved light", lambda: r.set_lights(lights[:1], 0)),
                           ("a new seed", lambda: r.set_stars_seed(12345))):
            edit()
            f.reset(); f.run(r, n_samples, stride)
            got = f.read()
            assert got[0].tobytes() != last[0].tobytes(), what                   # the edit shows
            same(got, gu.by_soft(lib, hip, r, hits, dirs, n_samples, stride=stride)[:2], what)
            last = got
    finally:
        f.close()
        r.close()


# ------------------------------------------------------------------ 5. a whole view
@pytest.mark.parametrize("model", [vu.PINHOLE, vu.EQUIRECT])
def test_gather_view_is_gather_of_the_views_hit_records(lib, hip, model):
    w, h = 33, 17
    scene = the_scene("default14_stars")
    c = scene["camera"]
    views = Views(lib, hip, model, w, h, cam=(c["origin"], c["axisX"], c["axisY"], c["axisZ"]), fov=scene["fovDeg"])
    n_samples, n_dirs, stride = 5, 64, 7
    dirs = rt_host.ambient_dirs(n_dirs)
    try:
        hits = rt_host.view_hit_records(scene, views.host, w, h, lib=lib)
        assert (hits["object"] >= 0).any()
        want = rt_host.gather(scene, hits, n_samples, dirs=dirs, stride=stride, base=5, pix_base=3, want=WANT, lib=lib)      # pix_stride None: w h
        got = rt_host.gather_view(scene, views.host, w, h, n_samples, dirs=dirs, stride=stride, base=5, pix_base=3, want=WANT, lib=lib)
        for k in WANT:
            assert got[k].tobytes() == want[k].tobytes(), k
        assert len(set(got["rgba"].view(np.uint32).reshape(-1).tolist())) > 1                       # a picture, not a constant
        # the resident form: the least workspace (one row per band), a few rows and the whole view give the same bytes
        r = rt_host.Renderer(scene, 0, lib)
        d_dirs = upload(lib, hip, dirs)
        try:
            for work_bytes in (128 * w, 128 * w * 5, rt_host.gather_view_work_bytes(w, h)):
                rgb, rgba, work = Dev(lib, w * h * 24), Dev(lib, w * h * 4), Dev(lib, work_bytes)
                try:
                    st = r.gather_view(views.dev, w, h, d_dirs, n_dirs, n_samples, rgb.p, rgba.p, work.p, work_bytes, stride=stride, base=5, pix_base=3,
                                       want_stats=True)
                    assert st.pixels == w * h
                    work.read()                                                  # (its canaries)
                    assert rgb.read().tobytes() == want["rgb"].tobytes() and rgba.read().tobytes() == want["rgba"].tobytes(), work_bytes
                finally:
                    for d in (rgb, rgba, work):
                        d.close()
        finally:
            lib.rt_free_device(0, d_dirs)
            r.close()
    finally:
        views.close()


# ------------------------------------------------------------------ 6. the host form past its chunk edge
def test_the_host_form_passes_each_chunk_its_base_and_pix_base(lib, hip):
    """2^18 + 200 receivers (the 5 184 records tiled), one sample, depth 1: the second chunk's receivers take base and pix_base + 2^18 -
    the table entry (n_dirs = 61 is prime) and the stars differ from those of index 0."""
    scene, base_list = receivers(lib, "default14_stars")
    n, n_dirs, stride = 2 ** 18 + 200, 61, 7
    assert au.entry(0, 2 ** 18, stride, 0, n_dirs) != au.entry(0, 0, stride, 0, n_dirs)
    hits = base_list[np.arange(n) % len(base_list)]
    dirs = rt_host.ambient_dirs(n_dirs)
    whole = rt_host.gather(scene, hits, 1, dirs=dirs, stride=stride, segs=1, pix_stride=0, want=WANT, lib=lib)
    # the device form piecewise at the seam: 300 receivers on each side of it, as pieces of the whole list
    r = rt_host.Renderer(scene, 0, lib)
    seam = hits[2 ** 18 - 300:2 ** 18 + 200]
    f = Fused(lib, hip, seam, dirs)
    try:
        f.reset()
        f.run(r, 1, stride, n=300, segs=1, base=2 ** 18 - 300, pix_base=2 ** 18 - 300, pix_stride=0)
        f.run(r, 1, stride, first=300, segs=1, base=2 ** 18, pix_base=2 ** 18, pix_stride=0)
        got = f.read()
        same((whole["rgb"][2 ** 18 - 300:], whole["rgba"].view(np.uint32).reshape(-1)[2 ** 18 - 300:]), got, "the seam")
        same(got, gu.by_soft(lib, hip, r, seam, dirs, 1, stride=stride, segs=1, base=2 ** 18 - 300, pix_base=2 ** 18 - 300, pix_stride=0)[:2], "the seam, the yardstick")
        # without the advance the second chunk would be the first tile's answer again: it is not
        first = rt_host.gather(scene, hits[2 ** 18:], 1, dirs=dirs, stride=stride, segs=1, pix_stride=0, want=WANT, lib=lib)
        assert first["rgb"].tobytes() != whole["rgb"][2 ** 18:].tobytes()
    finally:
        f.close()
        r.close()
