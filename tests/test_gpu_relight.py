"""Relit nodes on the GPU (include/rt_hip.h: rt_scene_relight_nodes_device, rt_relight_rays, rt_trace_rays_soft).  The kernel is held to
paths that exist without it: a relit node is the mean of the nodes rt_host.shade_rays writes for the same ray in scenes whose lights
were moved on the host (tests/relight_util.py: by_moved_lights), and a soft trace is the recursive rt_host.trace_rays of such a scene,
or the chain shade, relight, spawn, trace, fold.  Every comparison is of bytes: a displaced light is one multiply and one add in
binary64, the per-sample loop is the shade kernel's own, the fold is binary64 additions in a fixed order and one correctly rounded
division.  No tolerance, no node left out."""
import numpy as np
import pytest

import lighting_util as lu
import nodes_util as nu
import relight_util as rl
import rt_host
from test_gpu_views import lib  # noqa: F401  (a fixture; the canary-framed device arrays are nodes_util's Dev, which takes a source)

pytestmark = pytest.mark.gpu
SCENES = ["default14", "h8"]
TABLE = lu.turned_sets(4, 2)                              # 8 entries on the unit sphere
RADIUS = 1.0
BASE = 2 ** 40 + 3
ONE = np.array([[0.6, -0.48, 0.64]])                      # the one-entry table of the moved sample


def bytes_of(nodes):
    return np.ascontiguousarray(nodes).view(np.uint8).reshape(len(nodes), 200)


def relit(lib, scene, rays, n_samples, radius, offs=None, stride=1, base=0, pix=None, order=None, nodes=None):
    """-> (the shaded nodes, the same nodes after Renderer.relight_nodes), canaries checked."""
    r = rt_host.Renderer(scene, 0, lib)
    f = rl.Relit(lib, r, rays, offs=offs, pix=pix, order=order, nodes=nodes)
    try:
        before = f.nodes()
        st = f.relight(n_samples, radius, stride=stride, base=base, want_stats=True)
        assert st.pixels == len(rays) and st.kernel_ms > 0
        return before, f.nodes()
    finally:
        f.close()
        r.close()


# ------------------------------------------------------------------ 1. identity
@pytest.mark.parametrize("name", SCENES)
def test_one_sample_of_point_lights_is_the_shaded_node(lib, name):
    scene, rays, n_primary = rl.ray_list(lib, name)
    assert len(rays) > n_primary == rl.W * rl.H
    before, after = relit(lib, scene, rays, 1, 0.0)
    assert (before["inside"] != 0).any() and (before["specular"] > 0).any() and (before["object"] >= 0).all()
    rl.same_nodes(after, before, "one sample, radius 0")
    rl.same_nodes(before, rt_host.shade_rays(scene, rays, lib=lib), "the device's nodes are the host form's")
    # five equal samples: x + x + x + x + x, then / 5.  Binary64 gives x back for most x, not for all: where the stated fold of five
    # equal terms is not x, the node is held to that fold instead
    _, five = relit(lib, scene, rays, 5, 0.0, stride=3)
    want = before.copy()
    for k in ("diffuse", "specular"):
        want[k] = rl.fold(np.repeat(before[k][:, None], 5, axis=1))
    other = (lu.bits(want["diffuse"]) != lu.bits(before["diffuse"])) | (lu.bits(want["specular"]) != lu.bits(before["specular"]))
    print("RELIGHT %s: %d nodes, %d shading; five equal samples fold to something other than x for %d of them"
          % (name, len(rays), int(((before["diffuse"] != 0) | (before["specular"] != 0)).sum()), int(other.sum())))
    rl.same_nodes(five, want, "five equal samples")
    rl.same_nodes(five[~other], before[~other], "five equal samples give x back")


# ------------------------------------------------------------------ 2. one moved sample
@pytest.mark.parametrize("name", SCENES)
def test_one_moved_sample_is_the_scene_with_moved_lights(lib, name):
    scene, rays, n_primary = rl.ray_list(lib, name)
    moved = rl.moved_scene(scene, ONE[0], RADIUS)
    want = rt_host.shade_rays(moved, rays, lib=lib)
    before, after = relit(lib, scene, rays, 1, RADIUS, offs=ONE, stride=0)
    rl.same_nodes(after, want, "one moved sample")
    assert (bytes_of(after)[:, rl.RELIT] != bytes_of(before)[:, rl.RELIT]).any()
    # ... and every bounce relit is the recursive trace of that scene
    primary = rays[:n_primary]
    soft = rt_host.trace_rays_soft(scene, primary, 1, RADIUS, offs=ONE, stride=0, levels=scene["segs"], want=("rgb", "rgba"), lib=lib)
    ref = rt_host.trace_rays(moved, primary, want=("rgb", "rgba"), lib=lib)
    assert soft["rgb"].tobytes() == ref["rgb"].tobytes(), int((lu.bits(soft["rgb"]) != lu.bits(ref["rgb"])).any(axis=1).sum())
    assert soft["rgba"].tobytes() == ref["rgba"].tobytes()
    hard = rt_host.trace_rays(scene, primary, want=("rgba",), lib=lib)
    assert hard["rgba"].tobytes() != ref["rgba"].tobytes()


# ------------------------------------------------------------------ 3. samples and walks
_shaded = {}


@pytest.mark.parametrize("stride", [0, 1, 7])
@pytest.mark.parametrize("n_samples,n_offs", [(2, 2), (2, 8), (5, 5), (5, 8)])
@pytest.mark.parametrize("name", SCENES)
def test_samples_and_walks(lib, name, n_samples, n_offs, stride):
    """A nonzero base that no 32-bit index reaches, a pix array that is a permutation, tables of n_samples and of 8 entries (the first
    n_offs of one table, so the cases of a scene share their shade calls)."""
    scene, rays, _ = rl.ray_list(lib, name)
    pix = np.random.default_rng(5).permutation(len(rays)).astype(np.uint32)
    offs = TABLE[:n_offs]
    want, d, s = rl.by_moved_lights(scene, rays, offs, n_samples, RADIUS, stride, BASE, pix, lib=lib, shaded=_shaded.setdefault(name, {}))
    _, after = relit(lib, scene, rays, n_samples, RADIUS, offs=offs, stride=stride, base=BASE, pix=pix)
    rl.same_nodes(after, want, (name, n_samples, n_offs, stride))
    # a picture, not a constant: means that are not their first sample, and highlights
    assert (lu.bits(want["diffuse"]) != lu.bits(d[:, 0])).any() and (lu.bits(want["specular"]) != lu.bits(s[:, 0])).any()
    assert (want["specular"] > 0).any()
    if stride:
        assert len(np.unique(rl.entries(len(rays), n_offs, n_samples, stride, BASE, pix)[:, 0])) == n_offs        # the walk reaches every entry


# ------------------------------------------------------------------ 4. edges of the launch
@pytest.mark.parametrize("n", [1, 63, 64, 65, 256, 257])
def test_edges_of_the_launch(lib, n):
    scene, all_rays, _ = rl.ray_list(lib, "default14")
    rays = np.ascontiguousarray(all_rays[3000::max(1, (len(all_rays) - 3000) // n)][:n])     # across the spheres and the children
    assert len(rays) == n
    offs = TABLE[:4]
    want, _, _ = rl.by_moved_lights(scene, rays, offs, 3, RADIUS, 1, 5, lib=lib)
    before, after = relit(lib, scene, rays, 3, RADIUS, offs=offs, stride=1, base=5)
    rl.same_nodes(after, want, n)
    a, b = bytes_of(after), bytes_of(before)
    assert (a[:, :104] == b[:, :104]).all() and (a[:, 120:] == b[:, 120:]).all()            # nothing else of a node is written
    assert n < 60 or (a[:, rl.RELIT] != b[:, rl.RELIT]).any()
    # an order that is a permutation gives the plain call's bytes; an entry >= n names no node, and the node it stands for is untouched
    perm = np.random.default_rng(n).permutation(n).astype(np.uint32)
    _, ordered = relit(lib, scene, rays, 3, RADIUS, offs=offs, stride=1, base=5, order=perm, nodes=before)
    rl.same_nodes(ordered, after, (n, "a permutation"))
    skipped = int(perm[n // 2])
    holed = perm.copy()
    holed[n // 2] = n + 5
    _, part = relit(lib, scene, rays, 3, RADIUS, offs=offs, stride=1, base=5, order=holed, nodes=before)
    mixed = after.copy()
    mixed[skipped] = before[skipped]
    rl.same_nodes(part, mixed, (n, "an entry that names no node"))


# ------------------------------------------------------------------ 5. edges of the scene
def _sixteen_lights():
    rng = np.random.default_rng(16)
    return np.concatenate([rng.uniform(-8, 8, (16, 1)), rng.uniform(3, 12, (16, 1)), rng.uniform(-8, 8, (16, 1))], axis=1).tolist()


def _edit_albedo(scene, index, **albedo):
    s = rl.copy_of(scene)
    for k, v in albedo.items():
        s["objects"][index]["mtl"]["albedo"][int(k[1:])] = v
    return s


EDGES = {
    "no lights": lambda s: rl.copy_of(s, lights=[]),
    "16 lights": lambda s: rl.copy_of(s, lights=_sixteen_lights(), light_intensity=9),
    "no skybox": lambda s: rl.copy_of(s, objects=rl.copy_of(s)["objects"][:-1]),
    "neither diffuse nor specular": lambda s: _edit_albedo(s, 12, a1=0, a2=0),
    "diffuse alone": lambda s: _edit_albedo(s, 9, a2=0),
}


@pytest.mark.parametrize("edge", sorted(EDGES))
def test_edges_of_the_scene(lib, edge):
    base_scene, all_rays, _ = rl.ray_list(lib, "default14")
    rays = np.ascontiguousarray(all_rays[::3])
    scene = EDGES[edge](base_scene)
    offs = TABLE[:4]
    want, _, _ = rl.by_moved_lights(scene, rays, offs, 3, RADIUS, 1, 0, lib=lib)
    before, after = relit(lib, scene, rays, 3, RADIUS, offs=offs, stride=1)
    rl.same_nodes(after, want, edge)
    hit = before["object"] >= 0
    if edge == "no lights":
        assert hit.all() and not after["diffuse"].any() and not after["specular"].any()
    if edge == "no skybox":
        assert (~hit).any() and not after["diffuse"][~hit].any() and not after["specular"][~hit].any()
        assert (bytes_of(after)[~hit] == bytes_of(before)[~hit]).all()
    if edge == "neither diffuse nor specular":
        on = before["object"] == 12
        assert on.any() and not after["diffuse"][on].any() and not after["specular"][on].any()
    if edge == "diffuse alone":
        on = before["object"] == 9
        assert (after["diffuse"][on] > 0).any() and not after["specular"][on].any()
    if edge != "no lights":
        assert (bytes_of(after)[:, rl.RELIT] != bytes_of(before)[:, rl.RELIT]).any()


def test_a_ray_that_is_not_finite(lib):
    scene, all_rays, _ = rl.ray_list(lib, "default14")
    rays = np.ascontiguousarray(all_rays[2000:2300]).copy()
    rays[7, 4], rays[64, 0], rays[130, 5] = np.nan, np.inf, -np.inf
    want, _, _ = rl.by_moved_lights(scene, rays, TABLE[:4], 3, RADIUS, 1, 0, lib=lib)
    before, after = relit(lib, scene, rays, 3, RADIUS, offs=TABLE[:4], stride=1)
    rl.same_nodes(after, want, "NaN and Inf rays")
    for i in (7, 64, 130):
        assert after["object"][i] == -1 and after["diffuse"][i] == 0 and after["specular"][i] == 0 and np.isnan(after["sample"][i]).all()
        assert bytes_of(after)[i].tobytes() == bytes_of(before)[i].tobytes()


def test_edits_issued_just_before_the_call_are_seen(lib):
    """The nodes are shaded, THEN the lights move, the intensity changes and a glass sphere turns opaque: the relight reads the scene
    as it is at the call.  None of the three edits moves a hit, so the yardstick's bytes 104..119 - of the edited scene - belong to
    the same nodes, and every other byte stays the shade's."""
    scene, all_rays, _ = rl.ray_list(lib, "default14")
    rays = np.ascontiguousarray(all_rays[::3])
    offs = TABLE[:4]
    edited = rl.copy_of(scene, lights=[[4.0, 9.0, 6.0], [-5.0, 8.0, 1.0]], light_intensity=30)
    edited["objects"][6]["mtl"]["albedo"][4] = 0
    want, _, _ = rl.by_moved_lights(edited, rays, offs, 3, RADIUS, 1, 0, lib=lib)
    plain, _, _ = rl.by_moved_lights(scene, rays, offs, 3, RADIUS, 1, 0, lib=lib)
    r = rt_host.Renderer(scene, 0, lib)
    f = rl.Relit(lib, r, rays, offs=offs)
    try:
        before = f.nodes()
        r.set_lights(edited["lights"])
        r.set_light_intensity(30)
        r.set_objects([edited["objects"][6]], first=6)
        f.relight(3, RADIUS)
        after = f.nodes()
    finally:
        f.close()
        r.close()
    a, b, w, p = bytes_of(after), bytes_of(before), bytes_of(want), bytes_of(plain)
    assert (a[:, rl.RELIT] == w[:, rl.RELIT]).all(), int((a[:, rl.RELIT] != w[:, rl.RELIT]).any(axis=1).sum())
    assert (a[:, :104] == b[:, :104]).all() and (a[:, 120:] == b[:, 120:]).all()
    assert (w[:, :80] == b[:, :80]).all()                                                   # (the same hits in both scenes)
    assert (w[:, rl.RELIT] != p[:, rl.RELIT]).any()


# ------------------------------------------------------------------ 6. the loop
def test_no_level_relit_is_the_wavefront_trace(lib):
    scene, rays, n_primary = rl.ray_list(lib, "default14")
    primary = rays[:n_primary]
    want = rt_host.trace_rays(scene, primary, want=("rgb", "rgba", "level_counts"), method="wavefront", lib=lib)
    got = rt_host.trace_rays_soft(scene, primary, 4, RADIUS, offs=TABLE, stride=1, levels=0, want=("rgb", "rgba", "level_counts"), lib=lib)
    assert got["rgb"].tobytes() == want["rgb"].tobytes() and got["rgba"].tobytes() == want["rgba"].tobytes()
    assert got["level_counts"].tolist() == want["level_counts"].tolist() and want["level_counts"][1] > 0


@pytest.mark.parametrize("name", SCENES)
def test_one_level_relit_is_the_chain_of_device_calls(lib, name):
    """levels = 1 with 4 samples: Renderer.shade_rays, relight_nodes, spawn_rays, the recursive trace_rays of the children at segs - 1,
    and fold_nodes."""
    scene, rays, n_primary = rl.ray_list(lib, name)
    primary = np.ascontiguousarray(rays[:n_primary])
    segs = scene["segs"]
    got = rt_host.trace_rays_soft(scene, primary, 4, RADIUS, offs=TABLE, stride=1, levels=1, want=("rgb", "rgba", "level_counts"), lib=lib)
    _, nodes = relit(lib, scene, primary, 4, RADIUS, offs=TABLE, stride=1)
    r = rt_host.Renderer(scene, 0, lib)
    try:
        sp = nu.spawn(lib, r, nodes)
        assert sp["count"] == got["level_counts"][1] > 0
        child_rgb = rt_host.trace_rays(scene, sp["rays"], segs=segs - 1, want=("rgb",), lib=lib)["rgb"]
        rgb, rgba = nu.fold(lib, r, nodes, sp["links"], child_rgb)
    finally:
        r.close()
    assert got["rgb"].tobytes() == rgb.tobytes(), int((lu.bits(got["rgb"]) != lu.bits(rgb)).any(axis=1).sum())
    assert got["rgba"].tobytes() == rgba.tobytes()
    hard = rt_host.trace_rays(scene, primary, want=("rgba",), lib=lib)
    assert hard["rgba"].tobytes() != rgba.tobytes()
    # every bounce relit differs from the primary hits alone: the children's pix reach the kernel
    deep = rt_host.trace_rays_soft(scene, primary, 4, RADIUS, offs=TABLE, stride=1, levels=segs, want=("rgba",), lib=lib)
    assert name == "h8" or deep["rgba"].tobytes() != got["rgba"].tobytes()


def test_a_halved_chunk_gives_the_bytes_of_its_halves(lib):
    """90 000 rays of ~30 nodes each exceed one chunk's node budget (tests/test_gpu_nodes.py): the host form halves the chunk and starts
    it again.  Two levels relit, stride 1: the same bytes as the two halves of the list traced apart with base set."""
    from test_gpu_nodes import _four_spheres
    scene = _four_spheres()
    rays = rt_host.primary_rays(400, 225, scene)
    kw = dict(offs=TABLE, stride=1, levels=2, segs=16, lib=lib)
    whole = rt_host.trace_rays_soft(scene, rays, 2, RADIUS, want=("rgb", "rgba", "level_counts"), **kw)
    assert whole["level_counts"][0] == 90000 and whole["level_counts"].sum() > 2 ** 21
    half = 45001                                             # (not a multiple of the table's 8 entries: the second half's base decides bytes)
    a = rt_host.trace_rays_soft(scene, rays[:half], 2, RADIUS, want=("rgb", "rgba"), **kw)
    b = rt_host.trace_rays_soft(scene, rays[half:], 2, RADIUS, want=("rgb", "rgba"), base=half, **kw)
    for k in ("rgb", "rgba"):
        assert whole[k].tobytes() == a[k].tobytes() + b[k].tobytes(), k
    shifted = rt_host.trace_rays_soft(scene, rays[half:], 2, RADIUS, want=("rgba",), **kw)
    assert shifted["rgba"].tobytes() != b["rgba"].tobytes()                                 # (the base does decide bytes)


# ------------------------------------------------------------------ 7. the host form
@pytest.mark.parametrize("name", SCENES)
def test_the_host_form_is_the_device_entry(lib, name):
    scene, rays, _ = rl.ray_list(lib, name)
    _, want = relit(lib, scene, rays, 5, RADIUS, offs=TABLE, stride=7, base=BASE)
    got = rt_host.relight_rays(scene, rays, 5, RADIUS, offs=TABLE, stride=7, base=BASE, lib=lib)
    rl.same_nodes(got, want, "host form")
    rl.same_nodes(rt_host.relight_rays(scene, rays, 5, RADIUS, offs=TABLE, stride=7, base=BASE, order="binned", lib=lib), want, "host form, binned")
    # a list cut in two with pix set is the whole
    cut = (len(rays) // 3) | 1                               # (odd: with stride 7 over 8 entries the second piece's own indices walk other entries)
    pix = np.arange(len(rays), dtype=np.uint32)
    a = rt_host.relight_rays(scene, rays[:cut], 5, RADIUS, offs=TABLE, stride=7, base=BASE, pix=pix[:cut], lib=lib)
    b = rt_host.relight_rays(scene, rays[cut:], 5, RADIUS, offs=TABLE, stride=7, base=BASE, pix=pix[cut:], lib=lib)
    rl.same_nodes(np.concatenate([a, b]), want, "two pieces with pix")
    assert bytes_of(rt_host.relight_rays(scene, rays[cut:], 5, RADIUS, offs=TABLE, stride=7, base=BASE, lib=lib)).tobytes() != bytes_of(b).tobytes()
