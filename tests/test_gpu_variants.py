"""Every kernel variant a colour launch can pick (csrc/rt_device.h: rt_trace_variant) still launches and still renders the frame.

Per scene - reflection-only with few spheres (h8), many spheres / the GRID kernels (lcg64_ss1), supersample 2 (lcg64), refracting
(cfg2) - and frame size one Renderer renders: the first frame from its camera (four-wave workgroups), a second frame of the same kind
(one-wave workgroups where the variant has them), a scatter render (the peer-store path: four-wave again at supersample 1), a counting
render and a strict render.  64x16 at supersample 1 is four launch-table entries, fewer than one group of eight: the one-wave grid's
padded slots run.  33x9 has the ragged edge and, being odd both ways, the centre lines: rt_retrace runs behind every product launch.
tests/test_variants.py holds the rule itself (no GPU)."""
import ctypes as C

import pytest

import oracle_util as ou
import rt_host

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib(built):
    lib = rt_host.load_library()
    assert lib.rt_init(1) == 0, lib.rt_last_error()
    return lib


@pytest.mark.parametrize("w,h", [(64, 16), (33, 9)])
@pytest.mark.parametrize("scene", ["h8", "lcg64_ss1", "lcg64", "cfg2"])
def test_every_variant_of_a_scene_launches_and_renders_the_same_frame(lib, scene, w, h):
    blob = rt_host.flatten_scene(rt_host.load_scene(scene))
    whole = rt_host.RtTiles(h, 0, 1, 1)
    n = w * h * 4
    d = lib.rt_alloc_device(0, n)
    assert d, lib.rt_last_error()
    r = rt_host.Renderer(blob, 0, lib)
    try:
        def read():
            host = C.create_string_buffer(n)
            assert lib.rt_copy_to_host(0, host, d, n) == 0, lib.rt_last_error()
            return host.raw

        def tiles(flags=0):
            assert lib.rt_memset_device(0, d, 0x5A, n) == 0
            st = r.render_tiles(w, h, d, whole, flags=flags, want_stats=True)
            return read(), st
        first, st1 = tiles()
        second, st2 = tiles()
        assert lib.rt_memset_device(0, d, 0x5A, n) == 0
        r.render_scatter(w, h, [d], whole, want_stats=True)
        scattered = read()
        counted, stc = tiles(rt_host.RT_FLAG_COUNT)
        strict, sts = tiles(rt_host.RT_FLAG_STRICT_FP)
    finally:
        r.close()
        lib.rt_free_device(0, d)
    # the product frames: byte for byte the same, whichever form of the kernel stored them
    assert first == second == scattered, scene
    for st in (st1, st2, stc, sts):
        assert st.pixels == w * h
    # ... and within 1 LSB of the strict kernel's (test_gpu_parity.py: test_strict_and_fma_kernels_agree_within_1_lsb_at_4k)
    assert ou.max_lsb(first, strict)[0] <= 1, scene
    # the counting variant: the C oracle's frame and counters (test_gpu_parity.py: test_counting_variant_matches_oracle_counters)
    cnt = [0, 0, 0]
    want = ou.c_oracle_render(blob, w, h, counters=cnt)
    assert ou.max_lsb(counted, want)[0] <= 1, scene
    assert [stc.rays, stc.shadow_rays, stc.sphere_tests] == cnt, scene
