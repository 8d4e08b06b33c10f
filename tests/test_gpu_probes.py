"""Probes on the GPU (include/rt_hip.h: rt_probe_outputs, rt_scene_gather_probes_device): gathered light with a receiver's samples on
lanes.  The plain outputs are held to Renderer.gather - the receivers mapping, which this call must equal byte for byte - and to
tests/gather_util.py's by_soft, the yardstick that owes nothing to either gather kernel; the weighted sums to the numpy fold of by_soft's
per-sample colours in the header's order (numpy's *, + and / are separate IEEE operations).  Every comparison is of bytes, except the
coefficients of receivers that are not scanned: the sign of a NaN product is not stated, so there isnan is compared.

Inputs: tests/test_gpu_gather.py's - the 96 x 54 hit records per scene, and the mixed slice (glass, misses, NaN records side by side)."""
import base64
import json
import os
import subprocess

import numpy as np
import pytest

import ambient_util as au
import gather_util as gu
import oracle_util as ou
import rt_host
from test_gpu_ambient import SENTINEL_F64, SENTINEL_U32, receivers, the_scene
from test_gpu_gather import Fused, mixed_slice, same
from test_gpu_views import CANARY, Dev, hip, lib, upload  # noqa: F401  (lib and hip are fixtures)

pytestmark = pytest.mark.gpu
CAP = 1024                                                     # csrc/rt_probe.h RT_PROBE_CAP (tests/test_probe_resources.py reads it from the object)
N_DIRS, STRIDE = 1024, 7
SAMPLES = sorted({1, 3, 63, 64, 65, 255, 256, 257, 1024} | {q for q in (CAP - 1, CAP, CAP + 1) if q <= 1024})
WANT = ("rgb", "rgba")


class Probes:
    """Receivers, a table and (perhaps) weights in device memory, canary-framed outputs, and Renderer.gather_probes on them."""

    def __init__(self, lib, hip, hits, dirs, weights=None):
        self.lib, self.n, self.n_dirs = lib, len(hits), len(dirs)
        self.n_weights = 0 if weights is None else weights.shape[1]
        self.d_hits, self.d_dirs = upload(lib, hip, hits), upload(lib, hip, dirs)
        self.d_weights = upload(lib, hip, weights) if weights is not None else 0
        self.rgb, self.rgba, self.coef = Dev(lib, self.n * 24), Dev(lib, self.n * 4), Dev(lib, max(self.n * 24 * self.n_weights, 8))
        self.extra = []

    def reset(self):
        for d in (self.rgb, self.rgba, self.coef):
            assert self.lib.rt_memset_device(0, d.p, CANARY, d.n) == 0

    def run(self, r, n_samples, stride, want=WANT, n=None, first=0, **kw):
        """receivers [first, first + n) of the list, written at their own places in the outputs"""
        n = self.n - first if n is None else n
        coef = "coef" in want
        return r.gather_probes(n, self.d_hits + 80 * first, self.d_dirs, self.n_dirs, n_samples, self.rgb.p + 24 * first if "rgb" in want else 0,
                               self.rgba.p + 4 * first if "rgba" in want else 0, coef_ptr=self.coef.p + 24 * self.n_weights * first if coef else 0,
                               weights_ptr=self.d_weights if coef else 0, n_weights=self.n_weights if coef else 0, stride=stride, **kw)

    def read(self):
        return self.rgb.read(np.float64).reshape(self.n, 3), self.rgba.read(np.uint32)

    def read_coef(self):
        return self.coef.read(np.float64).reshape(self.n, self.n_weights, 3)

    def close(self):
        for d in (self.rgb, self.rgba, self.coef):
            d.close()
        for p in [self.d_hits, self.d_dirs] + ([self.d_weights] if self.d_weights else []) + self.extra:
            self.lib.rt_free_device(0, p)


def both(lib, hip, r, hits, dirs, n_samples, stride, what, **kw):
    """Renderer.gather and Renderer.gather_probes on the same inputs -> the parent's (rgb, rgba), after holding the probes' to them."""
    f, p = Fused(lib, hip, hits, dirs), Probes(lib, hip, hits, dirs)
    try:
        f.reset(); f.run(r, n_samples, stride, **kw)
        p.reset(); st = p.run(r, n_samples, stride, want_stats=True, **kw)
        assert st.pixels == len(hits) and st.kernel_ms > 0
        want = f.read()
        same(p.read(), want, what)
        return want
    finally:
        f.close()
        p.close()


def weighted_fold(c, weights, entries):
    """c (n_samples, n, 3), weights (n_dirs, n_weights), entries (n_samples, n) -> coef (n, n_weights, 3) in the header's order."""
    with np.errstate(invalid="ignore"):
        acc = weights[entries[0]][:, :, None] * c[0][:, None, :]
        for s in range(1, c.shape[0]):
            acc = acc + (weights[entries[s]][:, :, None] * c[s][:, None, :])
        return acc / float(c.shape[0])


def entries_of(n, n_samples, stride, n_dirs, base=0):
    return np.array([[au.entry(base, i, stride, s, n_dirs) for i in range(n)] for s in range(n_samples)], np.int64)


# ------------------------------------------------------------------ 1. against the parent's Renderer.gather
@pytest.mark.parametrize("n_samples", SAMPLES)
def test_the_samples_mapping_gives_the_receivers_mappings_bytes(lib, hip, n_samples):
    """One lane live, a wave less one, a wave, a second wave with one live lane, ..., every lane and every LDS slot (CAP = 1024: a lane
    has no second turn)."""
    scene = the_scene("default14")
    mix = mixed_slice(lib)
    dirs = rt_host.ambient_dirs(N_DIRS)
    r = rt_host.Renderer(scene, 0, lib)
    try:
        rgb, rgba = both(lib, hip, r, mix, dirs, n_samples, STRIDE, n_samples)
        nan = np.isnan(rgb).any(axis=1)
        assert nan.any() and not nan.all()                                                     # receivers whose mean is NaN, and others
        if n_samples >= 63:
            assert len(set(rgba.tolist())) > 16                                                # a picture, not a constant
    finally:
        r.close()


@pytest.mark.parametrize("name", ["default14_stars", "h8", "nosky"])
@pytest.mark.parametrize("stride", [0, 7])
def test_other_scenes_and_the_coherent_table(lib, hip, name, stride):
    scene = the_scene(name)
    mix = mixed_slice(lib)
    dirs = rt_host.ambient_dirs(N_DIRS)
    r = rt_host.Renderer(scene, 0, lib)
    try:
        rgb, rgba = both(lib, hip, r, mix, dirs, 65, stride, (name, stride))
        assert len(set(rgba.tolist())) > 16
        if name == "default14_stars":
            flat, _ = both(lib, hip, r, mix, dirs, 65, stride, (name, stride, "pix_stride 0"), pix_stride=0)
            assert (au.bits(flat) != au.bits(rgb)).any(axis=1).any()                         # the stars do see the sample's pix
    finally:
        r.close()


@pytest.mark.parametrize("segs", [1, 2])
def test_the_calls_depth(lib, hip, segs):
    scene = the_scene("default14")
    r = rt_host.Renderer(scene, 0, lib)
    try:
        deep = both(lib, hip, r, mixed_slice(lib), rt_host.ambient_dirs(N_DIRS), 65, STRIDE, ("segs", 0))
        got = both(lib, hip, r, mixed_slice(lib), rt_host.ambient_dirs(N_DIRS), 65, STRIDE, ("segs", segs), segs=segs)
        assert au.bits(got[0]).tobytes() != au.bits(deep[0]).tobytes()                         # (the depth does reach the walk)
    finally:
        r.close()


# ------------------------------------------------------------------ 2. against the yardstick that owes nothing to either gather kernel
@pytest.mark.parametrize("n_samples", [5, 65])
def test_against_the_fold_of_the_soft_trace(lib, hip, n_samples):
    scene = the_scene("default14")
    mix = mixed_slice(lib)
    dirs = rt_host.ambient_dirs(N_DIRS)
    base = 2 ** 40 + 3
    r = rt_host.Renderer(scene, 0, lib)
    p = Probes(lib, hip, mix, dirs)
    try:
        rgb, rgba, _ = gu.by_soft(lib, hip, r, mix, dirs, n_samples, stride=STRIDE, base=base, pix_base=11)
        assert np.isnan(rgb).any() and not np.isnan(rgb).all()
        p.reset(); p.run(r, n_samples, STRIDE, base=base, pix_base=11)
        same(p.read(), (rgb, rgba), n_samples)
        no_base, _, _ = gu.by_soft(lib, hip, r, mix, dirs, n_samples, stride=STRIDE, pix_base=11)
        assert au.bits(no_base).tobytes() != au.bits(rgb).tobytes()                            # (the base does reach the table)
    finally:
        p.close()
        r.close()


# ------------------------------------------------------------------ 3. short lists, orders, NULL outputs, sentinels
def test_short_lists_orders_and_null_outputs(lib, hip):
    scene = the_scene("default14")
    hits = mixed_slice(lib)
    n = len(hits)
    n_samples, n_dirs = 65, 128
    dirs = rt_host.ambient_dirs(n_dirs)
    weights = np.random.default_rng(3).uniform(-1.0, 1.0, (n_dirs, 2))
    r = rt_host.Renderer(scene, 0, lib)
    f, p = Fused(lib, hip, hits, dirs), Probes(lib, hip, hits, dirs, weights)
    try:
        for first in (0, 2):
            for m in (1, 2, 5):
                f.reset(); f.run(r, n_samples, STRIDE, n=m, first=first, pix_stride=0)
                want = f.read()
                p.reset(); p.run(r, n_samples, STRIDE, n=m, first=first, pix_stride=0)
                got = p.read()
                same([g[first:first + m] for g in got], [w[first:first + m] for w in want], (first, m))
                assert (got[0].view(np.uint64)[:first] == SENTINEL_F64).all() and (got[0].view(np.uint64)[first + m:] == SENTINEL_F64).all()
                assert (got[1][:first] == SENTINEL_U32).all() and (got[1][first + m:] == SENTINEL_U32).all()
        f.reset(); f.run(r, n_samples, STRIDE)
        want = f.read()
        # reversed, with one entry >= n: the receiver it stood for keeps the sentinel
        order = np.arange(n, dtype=np.uint32)[::-1].copy()
        dropped = int(order[7])
        order[7] = n
        p.extra.append(upload(lib, hip, order))
        p.reset(); p.run(r, n_samples, STRIDE, want=WANT + ("coef",), order_ptr=p.extra[-1])
        got, coef = p.read(), p.read_coef()
        named = np.arange(n) != dropped
        same([g[named] for g in got], [w[named] for w in want], "reversed, one entry names no receiver")
        assert (got[0][dropped].view(np.uint64) == SENTINEL_F64).all() and got[1][dropped] == SENTINEL_U32
        assert (coef[dropped].view(np.uint64) == SENTINEL_F64).all() and not (coef[named].view(np.uint64) == SENTINEL_F64).any()
        # each output alone is itself with the others; the others keep the sentinel
        bufs = {"rgb": p.rgb, "rgba": p.rgba, "coef": p.coef}
        for k in bufs:
            p.reset(); p.run(r, n_samples, STRIDE, want=(k,))
            if k == "coef":
                assert p.read_coef()[named].tobytes() == coef[named].tobytes()
            else:
                i = WANT.index(k)
                same([p.read()[i]], [want[i]], k + " alone")
            for o, d in bufs.items():
                if o != k:
                    assert (d.read() == CANARY).all(), (k, o)
    finally:
        f.close()
        p.close()
        r.close()


# ------------------------------------------------------------------ 4. weighted sums
def test_unit_weights_give_the_mean(lib, hip):
    scene = the_scene("default14")
    mix = mixed_slice(lib)
    dirs = rt_host.ambient_dirs(N_DIRS)
    r = rt_host.Renderer(scene, 0, lib)
    p = Probes(lib, hip, mix, dirs, np.ones((N_DIRS, 1)))
    try:
        p.reset(); p.run(r, 65, STRIDE, want=WANT + ("coef",))
        rgb, coef = p.read()[0], p.read_coef()
        assert np.isnan(rgb).any() and not np.isnan(rgb).all()
        assert au.bits(coef[:, 0]).tobytes() == au.bits(rgb).tobytes()                         # 1.0 * c is c
    finally:
        p.close()
        r.close()


_soft = {}


def soft_colours(lib, hip, r, mix, dirs, n_samples, stride):
    """by_soft's per-sample colours, once per (n_samples, stride), left unchanged"""
    if (n_samples, stride) not in _soft:
        c = gu.by_soft(lib, hip, r, mix, dirs, n_samples, stride=stride)[2]
        c.setflags(write=False)
        _soft[(n_samples, stride)] = c
    return _soft[(n_samples, stride)]


@pytest.mark.parametrize("n_samples", [65, 257])
@pytest.mark.parametrize("stride", [0, 7])
@pytest.mark.parametrize("n_weights", [9, 16])
def test_coefficients_are_the_numpy_fold_in_the_stated_order(lib, hip, n_weights, stride, n_samples):
    scene = the_scene("default14")
    mix = mixed_slice(lib)
    dirs = rt_host.ambient_dirs(N_DIRS)
    weights = rt_host.sh9_weights(dirs, lib=lib) if n_weights == 9 else np.random.default_rng(16).uniform(-2.0, 2.0, (N_DIRS, 16))
    r = rt_host.Renderer(scene, 0, lib)
    p = Probes(lib, hip, mix, dirs, weights)
    try:
        c = soft_colours(lib, hip, r, mix, dirs, n_samples, stride)
        entries = entries_of(len(mix), n_samples, stride, N_DIRS)
        want = weighted_fold(c, weights, entries)
        p.reset(); p.run(r, n_samples, stride, want=("coef",))
        got = p.read_coef()
        ok = au.scanned(mix)
        assert ok.any() and (~ok).any()
        assert not np.isnan(want[ok]).any() and au.bits(got[ok]).tobytes() == au.bits(want[ok]).tobytes()
        assert np.isnan(got[~ok]).all() and np.isnan(want[~ok]).all()
        # the coefficients depend on the table entry: with the rows permuted they change, and are again the fold
        perm = np.random.default_rng(5).permutation(N_DIRS)
        q = Probes(lib, hip, mix, dirs, weights[perm])
        try:
            q.reset(); q.run(r, n_samples, stride, want=("coef",))
            moved = q.read_coef()
        finally:
            q.close()
        assert (au.bits(moved[ok]) != au.bits(got[ok])).any()
        assert au.bits(moved[ok]).tobytes() == au.bits(weighted_fold(c, weights[perm], entries)[ok]).tobytes()
    finally:
        p.close()
        r.close()


# ------------------------------------------------------------------ 5. a list in two pieces
def test_a_list_in_two_pieces_is_one_call(lib, hip):
    scene = the_scene("default14_stars")
    mix = mixed_slice(lib)
    n = len(mix)
    dirs = rt_host.ambient_dirs(N_DIRS)
    weights = rt_host.sh9_weights(dirs, lib=lib)
    r = rt_host.Renderer(scene, 0, lib)
    p = Probes(lib, hip, mix, dirs, weights)
    all3 = WANT + ("coef",)
    try:
        p.reset(); p.run(r, 65, STRIDE, want=all3, pix_base=11)                   # pix_stride None: n
        whole, whole_coef = p.read(), p.read_coef()
        cut = 64 + 37
        p.reset()
        p.run(r, 65, STRIDE, want=all3, n=cut, pix_base=11, pix_stride=n)
        p.run(r, 65, STRIDE, want=all3, first=cut, base=cut, pix_base=11 + cut, pix_stride=n)
        same(p.read(), whole, "two pieces")
        assert p.read_coef().tobytes() == whole_coef.tobytes()
        p.reset()
        p.run(r, 65, STRIDE, want=all3, n=cut, pix_base=11, pix_stride=n)
        p.run(r, 65, STRIDE, want=all3, first=cut, pix_base=11, pix_stride=n)      # without the advance: another answer
        assert p.read()[0].tobytes() != whole[0].tobytes()
    finally:
        p.close()
        r.close()


# ------------------------------------------------------------------ 6. edits of the resident scene
def test_a_moved_sphere_a_moved_light_and_a_new_seed_take_effect(lib, hip):
    scene = the_scene("default14_stars")
    scene = dict(json.loads(json.dumps({k: v for k, v in scene.items() if k != "textures"})), textures=scene["textures"])      # (a copy to edit)
    mix = mixed_slice(lib)
    dirs = rt_host.ambient_dirs(N_DIRS)
    objs = scene["objects"]
    k = next(i for i, o in enumerate(objs) if o["r2"] == 1 and o["mtl"]["albedo"][4] == 0)
    r = rt_host.Renderer(scene, 0, lib)
    try:
        last = both(lib, hip, r, mix, dirs, 65, STRIDE, "before")
        objs[k]["origin"] = [objs[k]["origin"][0] + 0.75, objs[k]["origin"][1] + 0.5, objs[k]["origin"][2] + 0.25]
        lights = [list(q) for q in scene["lights"]]
        lights[0] = [lights[0][0] - 3.0, lights[0][1], lights[0][2] + 1.0]
        for what, edit in (("a moved sphere", lambda: r.set_objects(objs[k:k + 1], k)), ("a moved light", lambda: r.set_lights(lights[:1], 0)),
                           ("a new seed", lambda: r.set_stars_seed(12345))):
            edit()
            got = both(lib, hip, r, mix, dirs, 65, STRIDE, what)
            assert got[0].tobytes() != last[0].tobytes(), what                   # the edit shows
            last = got
    finally:
        r.close()


# ------------------------------------------------------------------ 7. the host forms, Python and Node
def test_host_forms_give_the_device_forms_bytes(lib, hip):
    scene = the_scene("default14")
    mix = mixed_slice(lib)
    dirs = rt_host.ambient_dirs(128)
    weights = rt_host.sh9_weights(dirs, lib=lib)
    all3 = WANT + ("coef",)
    r = rt_host.Renderer(scene, 0, lib)
    p = Probes(lib, hip, mix, dirs, weights)
    try:
        p.reset(); p.run(r, 65, STRIDE, want=all3, segs=2)
        dev, dev_coef = p.read(), p.read_coef()
    finally:
        p.close()
        r.close()
    host = rt_host.gather(scene, mix, 65, dirs=dirs, stride=STRIDE, segs=2, want=all3, lib=lib, mapping="samples", weights=weights)
    same((host["rgb"], host["rgba"].view(np.uint32).reshape(-1)), dev, "host form")
    assert host["coef"].tobytes() == dev_coef.tobytes()
    plain = rt_host.gather(scene, mix, 65, dirs=dirs, stride=STRIDE, segs=2, want=WANT, lib=lib, mapping="samples")
    parent = rt_host.gather(scene, mix, 65, dirs=dirs, stride=STRIDE, segs=2, want=WANT, lib=lib)
    assert all(plain[k].tobytes() == parent[k].tobytes() == host[k].tobytes() for k in WANT)
    # probes at three points: gather of the hand-made records, the sphere spiral as world directions
    points = [[0.0, 1.5, 0.0], [2.0, 0.5, -1.0], [-3.0, 2.0, 4.0]]
    sphere = rt_host.lighting_offsets(64, lib=lib)
    w9 = rt_host.sh9_weights(sphere, lib=lib)
    got = rt_host.probes(scene, points, 64, weights=w9, want=all3, lib=lib)
    recs = rt_host.hit_records(points, [[0.0, 0.0, 1.0]] * 3, [0, 0, 0])
    want = rt_host.gather(scene, recs, 64, dirs=sphere, stride=0, want=all3, lib=lib, mapping="samples", weights=w9)
    assert all(got[k].tobytes() == want[k].tobytes() for k in all3)
    assert not np.isnan(got["coef"]).any() and len({q.tobytes() for q in got["rgb"]}) == 3
    mean = rt_host.gather(scene, recs, 64, dirs=sphere, stride=0, want=("rgb",), lib=lib)
    assert mean["rgb"].tobytes() == got["rgb"].tobytes()


@pytest.mark.skipif(ou.node_path() is None, reason="node not installed")
def test_node_gives_pythons_bytes(lib, tmp_path):
    """RT.gather({mapping: 'samples', weights}), RT.probes and RT.sh9Weights (tests/js_probes_check.js) against the Python host forms'
    bytes, handed over in a file."""
    scene = the_scene("default14")
    mix = mixed_slice(lib)[:40]
    dirs = rt_host.ambient_dirs(128)
    weights = rt_host.sh9_weights(dirs, lib=lib)
    all3 = WANT + ("coef",)
    py = rt_host.gather(scene, mix, 65, dirs=dirs, stride=STRIDE, segs=2, want=all3, lib=lib, mapping="samples", weights=weights)
    points = [[0.0, 1.5, 0.0], [2.0, 0.5, -1.0], [-3.0, 2.0, 4.0]]
    sphere = rt_host.lighting_offsets(64, lib=lib)
    pr = rt_host.probes(scene, points, 64, weights=rt_host.sh9_weights(sphere, lib=lib), want=("rgb", "coef"), lib=lib)
    b64 = lambda a: base64.b64encode(np.ascontiguousarray(a).tobytes()).decode()
    ref = tmp_path / "probes.json"
    ref.write_text(json.dumps({"hits": b64(mix), "rgb": b64(py["rgb"]), "rgba": b64(py["rgba"]), "coef": b64(py["coef"]), "sh9": b64(weights),
                               "points": points, "probe_rgb": b64(pr["rgb"]), "probe_coef": b64(pr["coef"])}))
    pkg = os.path.join(ou.ROOT, "html5-canvas-raytracer_amd")
    done = subprocess.run([ou.node_path(), os.path.join(ou.ROOT, "tests", "js_probes_check.js"), pkg, str(ref)], stdout=subprocess.PIPE,
                          stderr=subprocess.PIPE, text=True, timeout=120)
    assert done.returncode == 0, done.stderr
    out = json.loads(done.stdout.strip().splitlines()[-1])
    assert out == {"rgb": True, "rgba": True, "coef": True, "sh9": True, "probe_rgb": True, "probe_coef": True, "refused": ["TypeError"] * 3}, out
