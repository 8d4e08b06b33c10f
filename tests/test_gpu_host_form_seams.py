"""The chunk seams of the host forms that had no test of theirs (include/rt_hip.h: rt_ambient_view, rt_lighting_view,
rt_trace_view_soft, rt_trace_rays_soft_recursive): a host form pushes its work through device buffers in chunks of 2^18 elements - a
view in chunks of whole rows - and must give the bytes of a path that is cut elsewhere or not at all.  A 700 x 400 view is 374 rows
and then 26; one sphere and at most one light, so a pixel costs next to nothing.  Every comparison is of bytes, and every case asserts
that the picture differs across the seam rows: a constant image cannot pass."""
import numpy as np
import pytest

import nodes_util as nu
import rt_host
import views_util as vu

pytestmark = pytest.mark.gpu
FOV = 52.0
W, H = 700, 400
SEAM = (1 << 18) // W                                      # the first row of the second chunk
assert SEAM == 374 and H - SEAM == 26
N_SAMPLES, N_TABLE, STRIDE = 4, 61, 7                      # a prime table length: no two neighbours walk the same entries
CAM = ([0.8, 1.9, 1.6], [0.0, 1.5, 0.0], [0.0, 1.0, 0.0])  # the ball lies across rows 373 / 374 (tests/test_gpu_views.py)
# a panorama with the world's axes from above the ball: it lies 6 degrees wide around latitude -78, which is row 373.5 of 400
EQUIRECT_CAM = ([0.0, 1.5 + 0.978 * 4.78, -0.208 * 4.78], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0])


@pytest.fixture(scope="module")
def lib(built):
    lib = rt_host.load_library()
    assert lib.rt_init(1) == 0, lib.rt_last_error()
    return lib


def one_sphere_scene():
    s = rt_host.load_scene("h8")
    ball = next(o for o in s["objects"] if o["r2"] < 100)
    return dict(s, objects=[dict(ball, origin=[0.0, 1.5, 0.0])], lights=[], segs=1)


def lit_scene():
    return dict(one_sphere_scene(), lights=[[3.0, 6.0, 4.0]])


def pinhole():
    return rt_host.view(vu.PINHOLE, *vu.look_at(*CAM), FOV)


def crosses_the_seam(a):
    """(w h, ...) records in frame order: row 373 is not constant, and row 374 is another row"""
    rows = np.ascontiguousarray(a).view(np.uint8).reshape(H, W, -1)
    return len({bytes(p) for p in rows[SEAM - 1]}) > 1 and (rows[SEAM - 1] != rows[SEAM]).any()


def test_ambient_view_is_ambient_of_the_views_hit_records(lib):
    """rt_ambient_view cuts at row 374, rt_ambient of the same receivers at element 2^18 (row 374, column 344).  A lone sphere ends no
    scan of its own surface: what tells a hit from a miss is the intensity (1.0, and NaN for a miss)."""
    scene, v = one_sphere_scene(), pinhole()
    dirs = rt_host.ambient_dirs(N_TABLE, lib)
    want = ("open", "intensity", "rgba")
    got = rt_host.ambient_view(scene, v, W, H, N_SAMPLES, 2.0, dirs=dirs, stride=STRIDE, want=want, lib=lib)
    hits = rt_host.view_hit_records(scene, v, W, H, lib=lib)
    ref = rt_host.ambient(scene, hits, N_SAMPLES, 2.0, dirs=dirs, stride=STRIDE, want=want, lib=lib)
    for k in want:
        assert got[k].tobytes() == ref[k].tobytes(), k
    assert crosses_the_seam(got["intensity"])


def test_lighting_view_is_lighting_of_the_views_hit_records(lib):
    scene, v = lit_scene(), pinhole()
    offs = rt_host.lighting_offsets(N_TABLE, lib)
    want = rt_host.LIGHTING_OUTPUTS
    got = rt_host.lighting_view(scene, v, W, H, N_SAMPLES, 0.5, offs=offs, stride=STRIDE, want=want, lib=lib)
    hits = rt_host.view_hit_records(scene, v, W, H, lib=lib)
    ref = rt_host.lighting(scene, hits, N_SAMPLES, 0.5, offs=offs, stride=STRIDE, want=want, lib=lib)
    for k in want:
        assert got[k].tobytes() == ref[k].tobytes(), k
    assert crosses_the_seam(got["rgba"]) and crosses_the_seam(got["diffuse"])


@pytest.mark.parametrize("model", [vu.PINHOLE, vu.EQUIRECT])
def test_trace_view_soft_is_the_resident_form_in_one_band(lib, model):
    """EQUIRECT: a row behind the seam reads its entry of the latitude table by its row in the VIEW, not in the chunk."""
    scene = lit_scene()
    offs = rt_host.lighting_offsets(N_TABLE, lib)
    cam = vu.look_at(*CAM) if model == vu.PINHOLE else EQUIRECT_CAM
    tables = rt_host.equirect_tables(W, H) if model == vu.EQUIRECT else None
    host = rt_host.view(model, *cam, FOV, tables=tables)
    d_tables = [nu.Dev(lib, t.nbytes, t) for t in tables or ()]              # the device form's view: its tables in device memory
    assert all(t.ptr % 16 == 0 for t in d_tables)
    dev = rt_host.view(model, *cam, FOV, tables=tuple(t.ptr for t in d_tables) if tables else None)
    kw = dict(stride=STRIDE, levels=1)
    work_bytes = rt_host.soft_view_work_bytes(W, H, lib)
    r = rt_host.Renderer(scene, 0, lib)
    bufs = [nu.Dev(lib, W * H * 24), nu.Dev(lib, W * H * 4), nu.Dev(lib, work_bytes), nu.Dev(lib, offs.nbytes, offs)]
    try:
        got = rt_host.trace_view_soft(scene, host, W, H, N_SAMPLES, 0.5, offs=offs, want=("rgb", "rgba"), method="recursive", lib=lib, **kw)
        d_rgb, d_rgba, d_work, d_offs = bufs
        r.trace_view_soft(dev, W, H, d_rgb.ptr, d_rgba.ptr, d_offs.ptr, N_TABLE, N_SAMPLES, 0.5, d_work.ptr, work_bytes, **kw)
        assert d_rgb.read().tobytes() == got["rgb"].tobytes() and d_rgba.read().tobytes() == got["rgba"].tobytes()
        assert crosses_the_seam(got["rgba"]) and crosses_the_seam(got["rgb"])
    finally:
        for b in bufs + d_tables:
            b.close()
        r.close()


@pytest.mark.parametrize("order", ["list", "binned"])
def test_a_soft_ray_list_is_its_two_chunks_traced_apart(lib, order):
    """2^18 + 5 of the view's rays: the second chunk's five rays are rays 2^18 .. of the list to the table walk"""
    scene = lit_scene()
    n = (1 << 18) + 5
    rays = np.ascontiguousarray(rt_host.view_rays(pinhole(), W, H, lib=lib).reshape(-1, 6)[:n])
    offs = rt_host.lighting_offsets(N_TABLE, lib)
    kw = dict(stride=STRIDE, levels=1)
    got = rt_host.trace_rays_soft(scene, rays, N_SAMPLES, 0.5, offs=offs, want=("rgb", "rgba"), method="recursive", order=order, lib=lib, **kw)
    r = rt_host.Renderer(scene, 0, lib)
    bufs = [nu.Dev(lib, n * 48, rays), nu.Dev(lib, n * 24), nu.Dev(lib, n * 4), nu.Dev(lib, offs.nbytes, offs)]
    try:
        d_rays, d_rgb, d_rgba, d_offs = bufs
        for first, m in ((0, 1 << 18), (1 << 18, 5)):                     # each piece at its own place in the outputs, with its pix_base
            r.trace_rays_soft(m, d_rays.ptr + 48 * first, d_rgb.ptr + 24 * first, d_rgba.ptr + 4 * first, d_offs.ptr, N_TABLE, N_SAMPLES, 0.5,
                              pix_base=first, **kw)
        assert d_rgb.read().tobytes() == got["rgb"].tobytes() and d_rgba.read().tobytes() == got["rgba"].tobytes()
    finally:
        for b in bufs:
            b.close()
        r.close()
    # the picture around the seam: row 373 is whole and not constant, and the five rays behind the seam are not its first five
    row = got["rgba"][(SEAM - 1) * W:SEAM * W]
    assert len({bytes(p) for p in row}) > 1 and len({bytes(p) for p in got["rgba"]}) > 8
    assert got["rgb"][1 << 18:].tobytes() != got["rgb"][(SEAM - 1) * W:(SEAM - 1) * W + 5].tobytes()
