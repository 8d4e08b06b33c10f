"""Sampled views on the GPU (include/rt_hip.h: rt_view_sample, rt_view_lens): the sample generator against the host probe, and the
sampled trace against values built from paths that exist without it - Renderer.trace_view for one zero sample, and for n samples
rt_host.trace_rays of the probe's rays of all samples in ONE list (ray s w h + i then draws the stated stars) folded in numpy in the
stated order.  Every comparison is byte for byte: the generator runs + - * / and sqrt without FMA contraction on the probe's own source,
the trace is the launch of a caller's ray list, and the fold is binary64 additions in a fixed order and one correctly rounded division."""
import ctypes as C

import numpy as np
import pytest

import rays_util
import rt_host
import view_samples_util as su
import views_util as vu
from test_gpu_views import CANARY, CAMS, Dev, hip, lib, one_sphere_scene, upload  # noqa: F401  (lib and hip are fixtures)

pytestmark = pytest.mark.gpu
MODELS = [vu.REFERENCE, vu.PINHOLE, vu.ORTHO, vu.EQUIRECT]
FOV, SCALE = 52.0, 0.037
INVALID = -1
W, H = 97, 33                # 3201 pixels: an odd count, so the accumulator's 9603 doubles end in the lane that takes one
THREE = [(0.25, -0.375, 0.5, -0.25), (-0.4, 0.1, -0.6, 0.3), (0.05, 0.45, 0.1, 0.9)]


def tup(s):
    return (s.dx, s.dy, s.lu, s.lv)


class SampledView:
    """A host view and its device twin at one size, for a list of samples: an EQUIRECT view carries one table per sample."""

    def __init__(self, lib, hip, model, w, h, samples, cam=None, fov=FOV, scale=SCALE):
        o, ax, ay, az = cam or vu.look_at(*vu.OBLIQUE)
        self.lib, self.ptrs = lib, []
        tables = rt_host.equirect_sample_tables(w, h, samples) if model == vu.EQUIRECT else None
        self.host = rt_host.view(model, o, ax, ay, az, fov, scale, tables=tables)
        if tables:
            self.ptrs = [upload(lib, hip, t) for t in tables]
        self.dev = rt_host.view(model, o, ax, ay, az, fov, scale, tables=tuple(self.ptrs) if tables else None)

    def close(self):
        for p in self.ptrs:
            self.lib.rt_free_device(0, p)


class Outputs:
    """Canary-framed rgb and rgba of n pixels, and a canary-framed workspace."""

    def __init__(self, lib, n, work_bytes):
        self.b = {"rgb": Dev(lib, n * 24), "rgba": Dev(lib, n * 4)}
        self.work = Dev(lib, work_bytes)
        self.work_bytes = work_bytes

    def trace(self, r, v, w, h, samples, lens=None, want=("rgb", "rgba"), **kw):
        return r.trace_view_samples(v, w, h, samples, lens, self.b["rgb"].p if "rgb" in want else 0, self.b["rgba"].p if "rgba" in want else 0,
                                    self.work.p, self.work_bytes, **kw)

    def read(self, k):
        self.work.read()                     # (its canaries; the body is scratch)
        return self.b[k].read()

    def close(self):
        for d in list(self.b.values()) + [self.work]:
            d.close()


# ------------------------------------------------------------------ the generator against the host probe
@pytest.mark.parametrize("model,lens", [(m, None) for m in MODELS] + [(vu.PINHOLE, su.LENS)])
def test_generated_sample_rays_are_the_probes(lib, hip, model, lens):
    """257 x 3: a second workgroup in x with one live lane.  1 x 65537: a second launch of the row loop.  An EQUIRECT view reads table 1
    of two tables: a generator that reads table 0 gives other rays."""
    samples = [(-0.125, 0.3, 0.2, 0.7), su.ARBITRARY]
    sample, table = samples[1], 1 if model == vu.EQUIRECT else 0
    L = rt_host.lens(*lens) if lens else None
    r = rt_host.Renderer(rt_host.load_scene("h8"), 0, lib)
    try:
        for w, h in [(257, 3), (1, 65537)]:
            v = SampledView(lib, hip, model, w, h, samples)
            d = Dev(lib, w * h * 48)
            try:
                r.view_sample_rays(v.dev, w, h, rt_host.view_sample(*sample), d.p, lens=L, table=table)
                got = d.read(np.uint64)                                             # nothing is written outside w * h records
                want = rt_host.view_sample_rays(v.host, w, h, sample, lens=L, table=table)
                assert (got == vu.bits(want).reshape(-1)).all(), (model, w, h)
                assert (vu.bits(want) != vu.bits(rt_host.view_sample_rays(v.host, w, h, samples[0], lens=L, table=0))).any()
                if h > 65535:
                    assert len({bytes(q) for q in want[65530:65537]}) == 7          # the rows differ where the launches meet
            finally:
                d.close()
                v.close()
    finally:
        r.close()


def test_generator_arguments(lib, hip):
    w, h = 8, 4
    v = SampledView(lib, hip, vu.PINHOLE, w, h, [su.ARBITRARY])
    d = Dev(lib, w * h * 48)
    s = rt_host.view_sample(*su.ARBITRARY)
    try:
        call = lambda first, rows, p, lens=None, sample=s: lib.rt_view_sample_rays_device(0, C.byref(v.dev), w, h, C.byref(lens) if lens is not None else None,
                                                                                          C.byref(sample) if sample is not None else None, 0, first, rows,
                                                                                          C.c_void_p(p), None)
        assert call(0, h + 1, d.p) == INVALID and "rows" in lib.rt_last_error().decode()
        assert call(0, h, 0) == INVALID and call(0, h, d.p + 8) == INVALID
        assert call(0, h, d.p, sample=None) == INVALID and call(0, h, d.p, lens=rt_host.lens(0.07, 0.0)) == INVALID
        assert call(2, 0, d.p) == 0                                                 # rows == 0: RT_OK, nothing written
        assert (d.read() == CANARY).all()
        assert call(1, 2, d.p) == 0
        got = d.read(np.uint64)
        assert (got[:2 * w * 6] == vu.bits(rt_host.view_sample_rays(v.host, w, h, s, first_row=1, rows=2)).reshape(-1)).all()
        assert (got[2 * w * 6:].view(np.uint8) == CANARY).all()
    finally:
        d.close()
        v.close()


# ------------------------------------------------------------------ one zero sample is the view
@pytest.mark.parametrize("name", ["h8", "default14_stars"])
def test_one_zero_sample_without_a_lens_is_trace_view(lib, hip, name):
    w, h = 96, 40
    scene = rt_host.load_scene(name)
    cam = scene["camera"]
    views = [rt_host.view(vu.REFERENCE, cam["origin"], cam["axisX"], cam["axisY"], cam["axisZ"], scene["fovDeg"]),
             rt_host.view(vu.PINHOLE, *vu.look_at(*vu.OBLIQUE), FOV)]
    r = rt_host.Renderer(scene, 0, lib)
    o = Outputs(lib, w * h, rt_host.view_samples_work_bytes(w, h))
    ref = {"rgb": Dev(lib, w * h * 24), "rgba": Dev(lib, w * h * 4)}
    work = Dev(lib, rt_host.view_work_bytes(w, h))
    try:
        seen = set()
        for v in views:
            r.trace_view(v, w, h, ref["rgb"].p, ref["rgba"].p, 0, work.p, work.n)
            st = o.trace(r, v, w, h, rt_host.view_samples_grid(1), want_stats=True)
            assert st.pixels == w * h and st.kernel_ms > 0
            for k in ("rgb", "rgba"):
                assert o.read(k).tobytes() == ref[k].read().tobytes(), (name, v.model, k)
            seen.add(o.read("rgba").tobytes())
            assert len({bytes(p) for p in o.read("rgba").reshape(-1, 4)}) > 20       # a picture, not a constant
        assert len(seen) == 2
    finally:
        for d in list(ref.values()) + [work]:
            d.close()
        o.close()
        r.close()


# ------------------------------------------------------------------ n samples against trace_rays of the probe's rays, folded in numpy
CASES = {"pinhole_lens": (vu.PINHOLE, su.LENS), "ortho": (vu.ORTHO, None), "equirect": (vu.EQUIRECT, None)}
_expected = {}


def sample_set(which):
    return [tup(s) for s in rt_host.view_samples_grid(2)] if which == "grid2" else THREE


def expected(lib, hip, name, case, which):
    """-> (rays of every sample (n, w h, 6), rgb per sample (n, w h, 3), the folded mean): computed once per case, from the probe's rays
    in sample-major order as ONE list through rt_host.trace_rays."""
    key = (name, case, which)
    if key not in _expected:
        model, lens = CASES[case]
        cam, scale = CAMS[model]
        samples = sample_set(which)
        v = SampledView(lib, hip, model, W, H, samples, cam, FOV, scale)
        L = rt_host.lens(*lens) if lens else None
        rays = np.stack([rt_host.view_sample_rays(v.host, W, H, s, lens=L, table=k) for k, s in enumerate(samples)])
        v.close()
        rgb = rt_host.trace_rays(rt_host.load_scene(name), rays.reshape(-1, 6), want=("rgb",))["rgb"].reshape(len(samples), W * H, 3)
        _expected[key] = (rays, rgb, su.fold(list(rgb)))
    return _expected[key]


@pytest.mark.parametrize("which", ["grid2", "three"])
@pytest.mark.parametrize("case", sorted(CASES))
@pytest.mark.parametrize("name", ["default14_stars", "h8"])
def test_a_sampled_trace_is_the_fold_of_trace_rays(lib, hip, name, case, which):
    model, lens = CASES[case]
    cam, scale = CAMS[model]
    samples = sample_set(which)
    _, per_sample, mean = expected(lib, hip, name, case, which)
    assert not np.isnan(mean).any() and len({bytes(p) for p in rays_util.store_rule(mean)}) > 20     # a picture, not a constant
    assert all((per_sample[0] != per_sample[k]).any() for k in range(1, len(samples)))               # the samples differ
    r = rt_host.Renderer(rt_host.load_scene(name), 0, lib)
    v = SampledView(lib, hip, model, W, H, samples, cam, FOV, scale)
    o = Outputs(lib, W * H, 96 * W * 5)                                                  # bands of 5 rows: 6 and a rest of 3 (485 and 291 pixels: odd)
    try:
        o.trace(r, v.dev, W, H, samples, rt_host.lens(*lens) if lens else None)
        assert (o.read("rgb").view(np.uint64) == vu.bits(mean).reshape(-1)).all(), (name, case, which)
        assert o.read("rgba").tobytes() == rays_util.store_rule(mean).tobytes()
    finally:
        o.close()
        v.close()
        r.close()


def test_each_sample_draws_its_own_stars(lib, hip):
    """Sample 1 of the list is traced with pix = w h + i: the same rays traced alone (pix = i) give another sky."""
    rays, per_sample, _ = expected(lib, hip, "default14_stars", "equirect", "three")
    alone = rt_host.trace_rays(rt_host.load_scene("default14_stars"), rays[1], want=("rgb",))["rgb"]
    assert (vu.bits(alone) != vu.bits(per_sample[1])).any()


# ------------------------------------------------------------------ bands
def test_no_result_depends_on_the_band_size(lib, hip):
    name, case, which = "default14_stars", "pinhole_lens", "grid2"
    model, lens = CASES[case]
    cam, scale = CAMS[model]
    samples = sample_set(which)
    _, _, mean = expected(lib, hip, name, case, which)
    r = rt_host.Renderer(rt_host.load_scene(name), 0, lib)
    v = SampledView(lib, hip, model, W, H, samples, cam, FOV, scale)
    assert rt_host.view_samples_work_bytes(W, H) == 96 * W * H
    outs = [Outputs(lib, W * H, 96 * W), Outputs(lib, W * H, 96 * W * 7), Outputs(lib, W * H, 96 * W * H)]     # one row, 7 rows (4 and a rest of 5), the view
    try:
        for o in outs:
            o.trace(r, v.dev, W, H, samples, rt_host.lens(*lens))
            assert (o.read("rgb").view(np.uint64) == vu.bits(mean).reshape(-1)).all(), o.work_bytes
            assert o.read("rgba").tobytes() == rays_util.store_rule(mean).tobytes(), o.work_bytes
    finally:
        for o in outs:
            o.close()
        v.close()
        r.close()


# ------------------------------------------------------------------ arguments, outputs, pending edits
def test_refusals_null_outputs_and_a_moved_sphere(lib, hip):
    w, h = 40, 24
    scene = rt_host.load_scene("default14")
    cam, _ = CAMS[vu.PINHOLE]
    samples = sample_set("grid2")
    arr, n = rt_host._samples_array(samples)
    L = rt_host.lens(*su.LENS)
    v = rt_host.view(vu.PINHOLE, *cam, FOV)
    r = rt_host.Renderer(scene, 0, lib)
    o = Outputs(lib, w * h, 96 * w * 5)
    hits = Dev(lib, w * h * 80)
    try:
        def call(scene_handle=r.handle, rgb=o.b["rgb"].p, rgba=o.b["rgba"].p, hits_p=0, work=o.work.p, work_bytes=o.work_bytes, segs=0, n=n, lens=L, view=v):
            out = rt_host.RtRayOutputs(rgb or None, rgba or None, hits_p or None)
            return lib.rt_scene_trace_view_samples_device(scene_handle, C.byref(view), w, h, C.byref(lens) if lens is not None else None, n, arr, segs,
                                                          C.byref(out), C.c_void_p(work), work_bytes, None, None)

        def refused(needle, **kw):
            assert call(**kw) == INVALID
            assert needle in lib.rt_last_error().decode(), lib.rt_last_error()

        assert call(scene_handle=None, n=0) == -5                                    # RT_ERR_STATE comes first
        refused("samples not in", n=0, work=0)                                       # ... then the validate function, then outputs and workspace
        refused("focus", lens=rt_host.lens(0.07, -1.0), rgb=0, rgba=0)
        refused("hits must be NULL", hits_p=hits.p)
        refused("every output is NULL", rgb=0, rgba=0)
        refused("misaligned output", rgba=o.b["rgba"].p + 2)
        refused("segs", segs=rt_host.RT_MAX_SEGS + 1)
        refused("workspace", work=0)
        refused("workspace", work=o.work.p + 8)
        refused("below one row", work_bytes=96 * w - 1)
        assert (o.read("rgb") == CANARY).all() and (o.read("rgba") == CANARY).all() and (o.work.read() == CANARY).all() and (hits.read() == CANARY).all()
        # an output that is not asked for is not touched
        assert call(rgb=0) == 0
        assert (o.read("rgb") == CANARY).all() and (o.read("rgba") != CANARY).any()
        before = o.read("rgba")
        # set_objects, then a sampled trace before anything else: it sees the moved sphere, as a freshly uploaded edited scene shows it
        i = next(i for i, ob in enumerate(scene["objects"]) if ob["r2"] < 1e4 and ob["mtl"]["albedo"][4] > 0)
        c0 = scene["objects"][i]["origin"]
        moved = dict(scene["objects"][i], origin=[c0[0] + 0.7, c0[1] + 0.3, c0[2] - 0.4])
        r.set_objects([moved], first=i)
        o.trace(r, v, w, h, samples, L)
        edited = dict(scene, objects=scene["objects"][:i] + [moved] + scene["objects"][i + 1:])
        fresh = rt_host.Renderer(edited, 0, lib)
        f = Outputs(lib, w * h, 96 * w * h)
        try:
            f.trace(fresh, v, w, h, samples, L)
            assert o.read("rgb").tobytes() == f.read("rgb").tobytes() and o.read("rgba").tobytes() == f.read("rgba").tobytes()
        finally:
            f.close()
            fresh.close()
        assert (o.read("rgba") != before).any()
    finally:
        hits.close()
        o.close()
        r.close()


# ------------------------------------------------------------------ the host form
def test_the_host_form_gives_the_device_forms_bytes(lib, hip):
    """520 x 520 = 270 400 pixels: 504 rows make the first chunk of 2^18 pixels, 16 rows the second.  One sphere, no lights: it takes no
    time.  n = 2."""
    w, h = 520, 520
    assert (1 << 18) // w == 504
    scene = one_sphere_scene()
    v = rt_host.view(vu.PINHOLE, *vu.look_at([0.8, 1.9, 1.6], [0.0, 2.0, 0.0], [0.0, 1.0, 0.0]), FOV)      # aimed above the ball: it lies across rows 503 / 504
    samples, L = THREE[:2], rt_host.lens(0.05, 2.0)
    got = rt_host.trace_view_samples(scene, v, w, h, samples, lens=L, want=("rgb", "rgba"))
    r = rt_host.Renderer(scene, 0, lib)
    o = Outputs(lib, w * h, rt_host.view_samples_work_bytes(w, h))
    try:
        o.trace(r, v, w, h, samples, L)
        assert o.read("rgba").tobytes() == got["rgba"].tobytes() and o.read("rgb").tobytes() == got["rgb"].tobytes()
        rows = got["rgba"].reshape(h, w, 4)
        assert len({bytes(p) for p in rows[503].reshape(-1, 4)}) > 1 and (rows[503] != rows[504]).any()     # the sphere crosses the chunks' seam
    finally:
        o.close()
        r.close()
    # an EQUIRECT view's tables of both samples are uploaded by the call
    e = SampledView(lib, hip, vu.EQUIRECT, 64, 32, samples, CAMS[vu.EQUIRECT][0])
    r = rt_host.Renderer(scene, 0, lib)
    o = Outputs(lib, 64 * 32, 96 * 64 * 32)
    try:
        o.trace(r, e.dev, 64, 32, samples)
        got = rt_host.trace_view_samples(scene, e.host, 64, 32, samples, want=("rgb", "rgba"))
        assert o.read("rgba").tobytes() == got["rgba"].tobytes() and o.read("rgb").tobytes() == got["rgb"].tobytes()
    finally:
        o.close()
        e.close()
        r.close()
