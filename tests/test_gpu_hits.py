"""Primary hits and picking on the GPU (include/rt_hip.h: rt_render_hits_device, rt_scene_pick, rt_render_hits, rt_pick), held to the
C restatement's per-sample probe (oracle/rt_oracle.c oracle_probe_sample) bit for bit: id, depth and normal of every sample, the whole
hit record of picked samples, after camera moves, in row tiles, beside colour frames, and through Node and the HTTP bridge."""
import json
import os
import subprocess

import numpy as np
import pytest

import hits_util as hu
import oracle_util as ou
import rt_host

pytestmark = pytest.mark.gpu
ROOT = ou.ROOT

SENTINEL = 0x5A


def _no_skybox_h8():
    s = rt_host.load_scene("h8")
    s["objects"] = [o for o in s["objects"] if o["r2"] < 1e6]        # without the enclosing sphere: rays that meet nothing
    return s


SCENES = {
    "h8_240x135": (lambda: rt_host.load_scene("h8"), 240, 135),
    "default14_160x90": (lambda: rt_host.load_scene("default14"), 160, 90),   # refraction, glass and bubble, skybox
    "cfg2_240x135": (lambda: rt_host.load_scene("cfg2"), 240, 135),           # textures
    "lcg64_ss2_128x128": (lambda: rt_host.load_scene("lcg64"), 128, 128),     # 64 spheres, supersample 2: 256 x 256 samples
    "h8_ss4_131x60": (lambda: rt_host.load_scene("h8_ss4"), 131, 60),
    "h8_no_skybox_240x135": (_no_skybox_h8, 240, 135),
}


class DeviceBuf:
    """Device memory from the library's allocator, pre-filled with a sentinel byte."""

    def __init__(self, nbytes, fill=SENTINEL):
        self.lib = rt_host.load_library()
        if self.lib.rt_device_count() < 0:
            assert self.lib.rt_init(0) == 0, self.lib.rt_last_error()
        self.n = nbytes
        self.p = self.lib.rt_alloc_device(0, nbytes)
        assert self.p, self.lib.rt_last_error()
        assert self.lib.rt_memset_device(0, self.p, fill, nbytes) == 0             # (synchronous)

    def host(self):
        out = np.empty(self.n, np.uint8)
        assert self.lib.rt_copy_to_host(0, out.ctypes.data, self.p, self.n) == 0   # (waits for the library's stream)
        return out

    def __del__(self):
        if self.p:
            self.lib.rt_free_device(0, self.p)
            self.p = None


class DeviceHits:
    """Device buffers for `band_rows` sample rows of k*w samples, pre-filled with a sentinel byte."""

    def __init__(self, band_rows, sw, which=(True, True, True)):
        self.shape = (band_rows, sw)
        self.t = [DeviceBuf(band_rows * sw * nb) for nb in (4, 8, 12)]
        self.which = which

    def ptrs(self):
        return [t.p if on else 0 for t, on in zip(self.t, self.which)]

    def host(self):
        b = [t.host() for t in self.t]
        r, c = self.shape
        return b[0].view(np.int32).reshape(r, c), b[1].view(np.float64).reshape(r, c), b[2].view(np.float32).reshape(r, c, 3), b


def _render_hits(r, w, h, k, tiles=None, band_rows=None, which=(True, True, True)):
    d = DeviceHits(band_rows or k * h, k * w, which)
    st = r.render_hits(w, h, *d.ptrs(), tiles=tiles, want_stats=True)
    assert st.kernel_ms > 0
    return d.host()


def _check_samples(probe, ids, depth, normal, samples):
    e_id, e_depth, e_normal = probe.expected(samples)
    ys, xs = np.array([s[1] for s in samples]), np.array([s[0] for s in samples])
    assert np.array_equal(ids[ys, xs], e_id)
    assert np.array_equal(depth[ys, xs].view(np.uint64), e_depth.view(np.uint64))               # bit for bit (inf on a miss)
    assert np.array_equal(normal[ys, xs].view(np.uint32), e_normal.view(np.uint32))
    miss = e_id == -1
    assert np.isinf(depth[ys, xs][miss]).all() and (normal[ys, xs][miss] == 0).all()
    return int(miss.sum())


@pytest.mark.parametrize("name", sorted(SCENES))
def test_hit_buffers_match_oracle_every_sample(name, built):
    make, w, h = SCENES[name]
    scene = make()
    k = scene.get("supersample", 1)
    r = rt_host.Renderer(scene)
    ids, depth, normal, _ = _render_hits(r, w, h, k)
    probe = hu.Probe(scene, w, h)
    samples = [(x, y) for y in range(k * h) for x in range(k * w)]
    misses = _check_samples(probe, ids, depth, normal, samples)
    assert (misses > 0) == (name == "h8_no_skybox_240x135"), misses
    if name == "default14_160x90":
        assert ((ids >> 16) == 1).any()                              # rays that start inside a sphere (the skybox) are flagged
    r.close()


def test_hit_buffers_large_frame(built):
    """H8 at 3840x2160: every buffer of the whole frame, a seeded sample of 20 000 samples against the oracle."""
    scene, w, h = rt_host.load_scene("h8"), 3840, 2160
    r = rt_host.Renderer(scene)
    ids, depth, normal, _ = _render_hits(r, w, h, 1)
    rng = np.random.default_rng(20261016)
    samples = list(zip(rng.integers(0, w, 20000).tolist(), rng.integers(0, h, 20000).tolist()))
    _check_samples(hu.Probe(scene, w, h), ids, depth, normal, samples)
    assert len(np.unique(ids)) >= 6
    r.close()


@pytest.mark.parametrize("name", sorted(SCENES))
def test_pick_matches_buffers_and_oracle(name, built):
    make, w, h = SCENES[name]
    scene = make()
    k = scene.get("supersample", 1)
    r = rt_host.Renderer(scene)
    ids, depth, normal, _ = _render_hits(r, w, h, k)
    rng = np.random.default_rng(7)
    pts = list(zip(rng.integers(0, k * w, 300).tolist(), rng.integers(0, k * h, 300).tolist()))
    got = r.pick(w, h, pts)
    probe = hu.Probe(scene, w, h)
    for (x, y), g in zip(pts, got):
        q = probe.root(x, y)
        if q[1] < 0:
            assert g is None and ids[y, x] == -1
            continue
        assert (g["object"], g["inside"]) == (int(q[1]) >> 1, bool(int(q[1]) & 1))
        assert ids[y, x] == g["object"] | (int(g["inside"]) << 16)
        assert g["t"] == q[2] == depth[y, x]
        assert g["point"] == list(q[3:6]) and g["normal"] == list(q[6:9])
        assert np.array_equal(np.float32(g["normal"]), normal[y, x])
        assert (g["u"], g["v"]) == probe.uv(q[6:9])
    r.close()


MOVES = [{"origin": [0.75, 2.0, 12.0], "axisX": [-1, 0, 0], "axisY": [0, 1, 0], "axisZ": [0, 0, -1]},
         {"origin": [-1.25, 1.0, 8.5], "axisX": [-1, 0, 0], "axisY": [0, 1, 0], "axisZ": [0, 0, -1]}]


def _moved(scene, cam):
    s = dict(scene)
    s["camera"] = cam
    return s


def test_camera_moves_device_forms_interleaved_with_colour(built):
    """rt_scene_set_camera, then colour frames and hits / picks on ONE stream: the hits follow the camera of each step."""
    scene, w, h = rt_host.load_scene("h8"), 240, 135
    r = rt_host.Renderer(scene)
    frame = DeviceBuf(w * h * 4)
    rng = np.random.default_rng(11)
    pts = list(zip(rng.integers(0, w, 100).tolist(), rng.integers(0, h, 100).tolist()))
    for cam in MOVES + [scene["camera"]]:
        d = DeviceHits(h, w)
        r.render_tiles(w, h, frame.p)                               # the previous camera's frame, still in flight
        r.set_camera(cam)
        r.render_tiles(w, h, frame.p)
        r.render_hits(w, h, *d.ptrs())                              # asynchronous, behind the colour frame
        r.render_tiles(w, h, frame.p)
        ids, depth, normal, _ = d.host()
        moved = _moved(scene, cam)
        probe = hu.Probe(moved, w, h)
        _check_samples(probe, ids, depth, normal, [(x, y) for y in range(h) for x in range(w)])
        for (x, y), g in zip(pts, r.pick(w, h, pts)):
            assert (g is None and ids[y, x] == -1) or (g["t"] == depth[y, x] and g["point"] == list(probe.root(x, y)[3:6]))
        got = frame.host()
        assert ou.max_lsb(got, ou.c_oracle_render(rt_host.flatten_scene(moved), w, h))[0] <= 1
    r.close()


def test_camera_moves_host_forms(built):
    """rt_render_hits / rt_pick on rt_render's resident scene: a blob that differs only in the camera moves it, and the hits follow."""
    scene, w, h = rt_host.load_scene("h8"), 240, 135
    rt_host.render(w, h, scene)
    for cam in MOVES:
        moved = _moved(scene, cam)
        out = rt_host.hits(w, h, moved)
        probe = hu.Probe(moved, w, h)
        _check_samples(probe, out["id"], out["depth"], out["normal"], [(x, y) for y in range(0, h, 3) for x in range(w)])
        pts = [(5, 7), (120, 60), (200, 130)]
        for (x, y), g in zip(pts, rt_host.pick(w, h, moved, pts)):
            q = probe.root(x, y)
            assert (g is None and q[1] < 0) or (g["t"] == q[2] and g["normal"] == list(q[6:9]))
        rgba, _ = rt_host.render(w, h, moved)
        assert ou.max_lsb(rgba, ou.c_oracle_render(rt_host.flatten_scene(moved), w, h))[0] <= 1


@pytest.mark.parametrize("name", ["h8_240x135", "lcg64_ss2_128x128", "h8_ss4_131x60"])
def test_row_tiles_reassemble_to_the_frame(name, built):
    """Interleaved 16-row tiles, stride 3 (the multi-GPU plan's shape): three calls' bands reassemble to the whole-frame buffers, byte
    for byte; the rows of a last tile that runs past the frame are left as they were."""
    make, w, h = SCENES[name]
    scene = make()
    k = scene.get("supersample", 1)
    r = rt_host.Renderer(scene)
    _, _, _, whole = _render_hits(r, w, h, k)
    tr, stride = 16, 3
    n_all = (h + tr - 1) // tr
    sw, rows_t = k * w, k * tr
    got = [np.full(k * h * sw * nb, SENTINEL, np.uint8) for nb in (4, 8, 12)]
    for g in range(stride):
        ts = list(range(g, n_all, stride))
        _, _, _, band = _render_hits(r, w, h, k, tiles=(tr, g, stride, len(ts)), band_rows=len(ts) * rows_t)
        for i, t in enumerate(ts):
            rows = min(rows_t, k * h - t * rows_t)
            for b, nb in enumerate((4, 8, 12)):
                src = band[b][i * rows_t * sw * nb:(i * rows_t + rows) * sw * nb]
                got[b][t * rows_t * sw * nb:(t * rows_t + rows) * sw * nb] = src
                if rows < rows_t:                                    # past the frame: untouched
                    assert (band[b][(i * rows_t + rows) * sw * nb:(i + 1) * rows_t * sw * nb] == SENTINEL).all()
    for b in range(3):
        assert np.array_equal(got[b], whole[b])
    r.close()


# ------------------------------------------------------------------ 65536 band rows: the one row grid y leaves to the loop's second turn
# rt_hits_kernel's grid y is capped at 65535 and `brow += gridDim.y` takes the rest: of the 65536 sample rows the ABI admits, band row
# 65535 alone belongs to a second turn.
TALL = [("h8", 8, 65536), ("h8_ss4", 2, 16384)]                      # both a sample grid of 8 x 65536


@pytest.mark.parametrize("name,w,h", TALL, ids=["%s_%dx%d" % c for c in TALL])
def test_65536_band_rows_match_the_oracle(name, w, h, built):
    scene = rt_host.load_scene(name)
    k = scene.get("supersample", 1)
    assert (k * w, k * h) == (8, 65536)
    r = rt_host.Renderer(scene)
    ids, depth, normal, raw = _render_hits(r, w, h, k)
    r.close()
    assert not any((b.reshape(k * h, -1) == SENTINEL).all(axis=1).any() for b in raw)      # no row of any buffer was left out
    rng = np.random.default_rng(20261018)
    samples = [(x, y) for y in (0, 1, 32767, 65534, 65535) for x in range(k * w)]
    samples += list(zip(rng.integers(0, k * w, 2000).tolist(), rng.integers(0, k * h, 2000).tolist()))
    _check_samples(hu.Probe(scene, w, h), ids, depth, normal, samples)
    assert len(np.unique(ids)) >= 2


def test_65536_band_rows_are_two_row_tiles_that_do_not_loop(built):
    """The same frame as two tiles of 32768 rows, one call each: neither call's band reaches the grid's cap, so neither loops; their
    bytes are the halves of the whole-frame call's."""
    scene, w, h = rt_host.load_scene("h8"), 8, 65536
    r = rt_host.Renderer(scene)
    _, _, _, whole = _render_hits(r, w, h, 1)
    halves = [_render_hits(r, w, h, 1, tiles=rt_host.RtTiles(32768, g, 1, 1), band_rows=32768)[3] for g in (0, 1)]
    r.close()
    for b, nb in enumerate((4, 8, 12)):
        cut = 32768 * w * nb
        assert np.array_equal(halves[0][b], whole[b][:cut]) and np.array_equal(halves[1][b], whole[b][cut:]), nb
        assert not np.array_equal(halves[0][b], halves[1][b])


def test_a_second_turn_row_past_the_frame_is_not_stored(built):
    """8 x 65530 in two tiles of 32768 rows is a band of 65536 rows whose last six lie past the frame - band row 65535, the second turn's
    only row, among them: they keep the sentinel in all three buffers, and the rows above are the frame's, rendered in tiles of 16384
    rows (four calls, none of which loops)."""
    scene, w, h = rt_host.load_scene("h8"), 8, 65530
    r = rt_host.Renderer(scene)
    _, _, _, band = _render_hits(r, w, h, 1, tiles=rt_host.RtTiles(32768, 0, 1, 2), band_rows=65536)
    parts = [_render_hits(r, w, h, 1, tiles=rt_host.RtTiles(16384, g, 1, 1), band_rows=16384)[3] for g in range(4)]
    r.close()
    for b, nb in enumerate((4, 8, 12)):
        cut = h * w * nb
        assert (band[b][cut:] == SENTINEL).all(), nb
        assert (parts[3][b][(h - 3 * 16384) * w * nb:] == SENTINEL).all(), nb
        assert np.array_equal(band[b][:cut], np.concatenate([p[b] for p in parts])[:cut]), nb
        assert not (band[b][:cut].reshape(h, -1) == SENTINEL).all(axis=1).any()


def test_hits_do_not_disturb_colour_frames_and_null_buffers_stay_untouched(built):
    scene, w, h = rt_host.load_scene("default14"), 160, 90
    r = rt_host.Renderer(scene)
    a, b = DeviceBuf(w * h * 4), DeviceBuf(w * h * 4)
    r.render_tiles(w, h, a.p)
    ids, depth, normal, full = _render_hits(r, w, h, 1)
    r.render_tiles(w, h, b.p)
    assert np.array_equal(a.host(), b.host())
    # each buffer alone: the others' memory keeps its sentinel, the one asked for equals the full call's
    for which in ((True, False, False), (False, True, False), (False, False, True)):
        _, _, _, part = _render_hits(r, w, h, 1, which=which)
        for on, p, f in zip(which, part, full):
            assert np.array_equal(p, f) if on else (p == SENTINEL).all()
    # nothing asked for: nothing launched, nothing written
    _, _, _, none = _render_hits(r, w, h, 1, which=(False, False, False))
    assert all((p == SENTINEL).all() for p in none)
    r.close()


def test_node_and_bridge_agree_with_python(built):
    if ou.node_path() is None:
        pytest.skip("node not installed")
    proc = subprocess.run([ou.node_path(), os.path.join(ROOT, "tests", "js_pick_check.js")], stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                          text=True, timeout=300)
    assert proc.returncode == 0, proc.stderr
    out = json.loads(proc.stdout.strip().splitlines()[-1])
    scene, w, h = rt_host.load_scene("default14"), 160, 90
    py = rt_host.hits(w, h, scene)
    import hashlib
    assert out["hits"] == {"id": hashlib.sha256(py["id"].tobytes()).hexdigest(), "depth": hashlib.sha256(py["depth"].tobytes()).hexdigest(),
                           "normal": hashlib.sha256(py["normal"].tobytes()).hexdigest(), "width": w, "height": h}
    assert out["idOnly"] == {"id": out["hits"]["id"], "depth": None, "normal": None}
    pts = [tuple(p) for p in out["pixels"]]
    ref = rt_host.pick(w, h, scene, pts)
    for (x, y), js, http, py_hit in zip(pts, out["picks"], out["http"], ref):
        if py_hit is None:
            assert js is None and http is None
            continue
        assert js["objectIsScene"] is True
        want = {"index": py_hit["object"], "inside": py_hit["inside"], "t": py_hit["t"], "point": py_hit["point"], "normal": py_hit["normal"],
                "u": py_hit["u"], "v": py_hit["v"]}
        assert {k: js[k] for k in want} == want
        assert http == want
    assert out["outside"] == {"pick": "RangeError", "status": 400}
