"""CPU tests of binned ray lists (include/rt_hip.h: rt_rays_order_work_bytes, rt_scene_order_rays_device,
rt_scene_trace_rays_ordered_device, rt_trace_rays_binned; rt_host.trace_rays(order=...)): header and binding, the workspace
arithmetic, argument checks before any device is touched, the loud failure without a GPU, and the new kernels' resources."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import oracle_util as ou
import rt_host
from test_gpu_rays_order import ORDER_BEYOND                     # (a table only: importing the module needs no GPU)
from test_rays import RT_ERR_DEVICE, RT_ERR_INVALID, RT_ERR_STATE, TOOLS, _aligned, _blob, _resources

ROOT = ou.ROOT
NEW = ("rt_rays_order_work_bytes", "rt_scene_order_rays_device", "rt_scene_trace_rays_ordered_device", "rt_trace_rays_binned")


def test_header_and_binding_agree(built, tmp_path):
    """A C compiler takes the header and binds the four prototypes; rt_host.ABI has the same shapes; the blob's ABI and
    rt_ray_outputs are what they were."""
    cc = shutil.which("gcc") or shutil.which("cc")
    assert cc, "a C compiler is needed (the oracle is built with one)"
    proto = tmp_path / "proto.c"
    proto.write_text('#include "rt_hip.h"\n'
                     'size_t (*wb)(uint64_t) = rt_rays_order_work_bytes;\n'
                     'int (*ord)(rt_scene_dev *, uint64_t, const double *, uint32_t *, void *, size_t, void *) = rt_scene_order_rays_device;\n'
                     'int (*tro)(rt_scene_dev *, uint64_t, const double *, const uint32_t *, uint32_t, const rt_ray_outputs *, void *, rt_stats *) = '
                     'rt_scene_trace_rays_ordered_device;\n'
                     'int (*bin)(const void *, size_t, uint64_t, const double *, uint32_t, const rt_ray_outputs *, rt_stats *) = rt_trace_rays_binned;\n')
    subprocess.run([cc, "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", "-o", str(tmp_path / "proto.o"), str(proto)], check=True)
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include "rt_hip.h"\nint main(void) { printf("%zu %u\\n", sizeof(rt_ray_outputs), RT_ABI_VERSION); return 0; }\n')
    exe = tmp_path / "layout"
    subprocess.run([cc, "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)], check=True)
    assert [int(x) for x in subprocess.check_output([str(exe)], text=True).split()] == [24, 2]
    assert rt_host.RT_ABI_VERSION == 2 and C.sizeof(rt_host.RtRayOutputs) == 24
    lib = rt_host.load_library()
    for name in NEW:
        assert name in rt_host.ABI
        assert getattr(lib, name).argtypes == rt_host.ABI[name][1] and getattr(lib, name).restype == rt_host.ABI[name][0]
    P, U64, U32, SZ = C.c_void_p, C.c_uint64, C.c_uint32, C.c_size_t
    assert rt_host.ABI["rt_rays_order_work_bytes"] == (SZ, [U64])
    assert rt_host.ABI["rt_scene_order_rays_device"] == (C.c_int, [P, U64, P, P, P, SZ, P])
    assert rt_host.ABI["rt_scene_trace_rays_ordered_device"] == (C.c_int, [P, U64, P, P, U32, C.POINTER(rt_host.RtRayOutputs), P, C.POINTER(rt_host.RtStats)])
    assert rt_host.ABI["rt_trace_rays_binned"] == rt_host.ABI["rt_trace_rays"]
    exported = subprocess.check_output(["nm", "-D", rt_host.LIB_PATH], text=True)
    for name in NEW:
        assert " T %s\n" % name in exported, name


def test_work_bytes(built):
    """Host arithmetic: callable before rt_init, 0 outside 1..2^31 - 1, positive and non-decreasing inside."""
    lib = rt_host.load_library()
    assert lib.rt_rays_order_work_bytes(0) == 0 and lib.rt_rays_order_work_bytes(2 ** 31) == 0 and lib.rt_rays_order_work_bytes(2 ** 40) == 0
    ns = [1, 63, 64, 65, 2 ** 18, 2 ** 18 + 1, 2 ** 23]
    got = [lib.rt_rays_order_work_bytes(n) for n in ns]
    assert all(b > 0 for b in got) and got == sorted(got), got
    assert [rt_host.rays_order_work_bytes(n) for n in ns] == got
    assert lib.rt_rays_order_work_bytes(2 ** 31 - 1) >= got[-1]
    assert got[-1] >= 3 * 4 * 2 ** 23                      # two key arrays and an index array at least


@pytest.fixture(scope="module")
def tlib(built):
    """The test build: rt_order_grid and the sort's tile count (csrc/rt_rays_order.h) as host arithmetic."""
    lib = rt_host.load_library(rt_host.TEST_LIB_PATH)
    lib.rt_test_order_grid.restype = C.c_uint32
    lib.rt_test_order_grid.argtypes = [C.c_uint32]
    lib.rt_test_order_tiles.restype = C.c_uint32
    lib.rt_test_order_tiles.argtypes = [C.c_uint64]
    return lib


def test_order_grid(tlib):
    """rt_order_grid(n) = min(ceil(n / 256), 4096): small lists, lists at the cap, the cap plus or minus one workgroup - each as exactly
    that many workgroups' rays, one ray fewer and one more - and the longest list."""
    cap = 4096
    ns = [1, 2, 255, 256, 257, 511, 512, 513, 2 ** 18 + 5, 2 ** 23, 2 ** 31 - 1]
    for wgs in (cap - 1, cap, cap + 1):
        ns += [wgs * 256 - 1, wgs * 256, wgs * 256 + 1]
    got = {n: tlib.rt_test_order_grid(n) for n in ns}
    assert got == {n: min(-(-n // 256), cap) for n in ns}
    assert got[1] == 1 and got[257] == 2 and got[(cap - 1) * 256] == cap - 1 and got[(cap - 1) * 256 + 1] == cap and got[cap * 256 + 1] == cap
    for n in (1, 4096, 4097, 2 ** 20, 2 ** 20 + 1, 2 ** 31 - 1):
        assert tlib.rt_test_order_tiles(n) == -(-n // 4096)


def test_the_large_gpu_case_reaches_the_second_turn_and_the_second_scan_chunk(tlib):
    """What makes tests/test_gpu_rays_order.py's list B ++ B ++ T non-vacuous, against the library's own grid and layout: the list is
    longer than one turn of the bounds and key kernels, every ray of T lies past that turn, its tile count needs a second chunk of
    rt_order_scan - and the yardstick list B ++ T needs neither."""
    m, k = ORDER_BEYOND["w"] * ORDER_BEYOND["h"], ORDER_BEYOND["extra"]
    n = 2 * m + k
    turn = tlib.rt_test_order_grid(n) * 256
    assert n > turn and 2 * m >= turn
    assert tlib.rt_test_order_tiles(n) > 256
    assert tlib.rt_test_order_grid(m + k) * 256 >= m + k and tlib.rt_test_order_tiles(m + k) <= 256
    assert rt_host.rays_order_work_bytes(n, tlib) >= 3 * 4 * n + 256 * 4 * tlib.rt_test_order_tiles(n)


def test_bad_arguments_are_invalid(built):
    """Every bad argument is refused with a message that names it, before a device is touched (the same answers with and without a
    GPU), and the caller's buffers keep their bytes."""
    lib = rt_host.load_library()
    err = lambda: lib.rt_last_error().decode()
    rays = _aligned(12)
    rays[:] = [0, 1.5, 10, 0, 0, -1] * 2
    order = np.full(4, 7, np.uint32)
    work = np.full(1 << 16, 7, np.uint8)
    need = lib.rt_rays_order_work_bytes(2)
    assert 0 < need <= work.nbytes

    def order_call(n=2, p=rays.ctypes.data, o=order.ctypes.data, w=work.ctypes.data, wb=work.nbytes, scene=None):
        return lib.rt_scene_order_rays_device(scene, n, C.c_void_p(p), C.c_void_p(o), C.c_void_p(w), wb, None)

    assert order_call(p=0) == RT_ERR_INVALID and "NULL" in err()
    assert order_call(o=0) == RT_ERR_INVALID and "NULL" in err()
    assert order_call(w=0) == RT_ERR_INVALID and "NULL" in err()
    assert order_call(p=_aligned(12, 8).ctypes.data) == RT_ERR_INVALID and "16-byte aligned" in err()
    assert order_call(o=order.ctypes.data + 2) == RT_ERR_INVALID and "misaligned order" in err()
    assert order_call(wb=need - 1) == RT_ERR_INVALID and "work_bytes %d" % (need - 1) in err() and "rt_rays_order_work_bytes" in err()
    assert order_call(wb=0) == RT_ERR_INVALID and "work_bytes 0" in err()
    assert order_call(n=0) == RT_ERR_INVALID and "n 0" in err()
    assert order_call(n=2 ** 31) == RT_ERR_INVALID and "n 2147483648" in err()
    assert order_call() == RT_ERR_STATE and "NULL scene" in err()                                   # everything right but the scene

    rgb = np.full(6, 7.0)
    rgba = np.full(8, 7, np.uint8)
    out = rt_host.RtRayOutputs(rgb.ctypes.data, rgba.ctypes.data, None)

    def trace_call(n=2, p=rays.ctypes.data, o=order.ctypes.data, segs=0, bufs=out):
        return lib.rt_scene_trace_rays_ordered_device(None, n, C.c_void_p(p), C.c_void_p(o), segs, C.byref(bufs) if bufs is not None else None, None, None)

    assert trace_call(o=0) == RT_ERR_INVALID and "order" in err()
    assert trace_call(o=order.ctypes.data + 2) == RT_ERR_INVALID and "misaligned order" in err()
    assert trace_call(n=0) == RT_ERR_INVALID and "n 0" in err()
    assert trace_call(n=2 ** 31) == RT_ERR_INVALID and "n 2147483648" in err()
    assert trace_call(segs=17) == RT_ERR_INVALID and "segs 17" in err()
    assert trace_call(p=0) == RT_ERR_INVALID and "NULL" in err()
    assert trace_call(p=_aligned(12, 8).ctypes.data) == RT_ERR_INVALID and "16-byte aligned" in err()
    assert trace_call(bufs=rt_host.RtRayOutputs(None, None, None)) == RT_ERR_INVALID and "every output is NULL" in err()
    assert trace_call(bufs=rt_host.RtRayOutputs(rgb.ctypes.data + 4, None, None)) == RT_ERR_INVALID and "misaligned output" in err()
    assert trace_call(bufs=None) == RT_ERR_INVALID
    assert trace_call() == RT_ERR_STATE and "NULL scene" in err()

    # the host form: rt_trace_rays' rules under its own name
    blob, buf = _blob()
    binned = lambda n=2, p=rays.ctypes.data, segs=0, bufs=out, nb=len(blob): lib.rt_trace_rays_binned(
        buf, nb, n, C.c_void_p(p), segs, C.byref(bufs) if bufs is not None else None, None)
    assert binned(n=0) == RT_ERR_INVALID and "rt_trace_rays_binned: n 0" in err()
    assert binned(n=2 ** 31) == RT_ERR_INVALID and "n 2147483648" in err()
    assert binned(segs=17) == RT_ERR_INVALID and "segs 17" in err()
    assert binned(p=0) == RT_ERR_INVALID and "NULL" in err()
    assert binned(p=_aligned(12, 8).ctypes.data) == RT_ERR_INVALID and "16-byte aligned" in err()
    assert binned(bufs=rt_host.RtRayOutputs(None, None, None)) == RT_ERR_INVALID and "every output is NULL" in err()
    assert binned(bufs=None) == RT_ERR_INVALID
    assert binned(nb=len(blob) - 8) == RT_ERR_INVALID                                                  # a malformed blob

    assert (order == 7).all() and (work == 7).all() and (rgb == 7.0).all() and (rgba == 7).all()
    for bad in ("sorted", "", None, "BINNED"):
        with pytest.raises(ValueError):
            rt_host.trace_rays(blob, np.zeros((3, 6)), order=bad)


def test_no_gpu_means_loud_failure(built):
    """Without a GPU a valid binned call fails with RT_ERR_STATE (no rt_init) / RT_ERR_DEVICE (rt_init finds no device): never zeros."""
    lib = rt_host.load_library()
    blob, buf = _blob()
    rays = _aligned(6)
    rays[:] = [0, 1.5, 10, 0, 0, -1]
    rgba = np.full(4, 7, np.uint8)
    out = rt_host.RtRayOutputs(None, rgba.ctypes.data, None)
    if lib.rt_device_count() < 0:
        assert lib.rt_trace_rays_binned(buf, len(blob), 1, C.c_void_p(rays.ctypes.data), 0, C.byref(out), None) == RT_ERR_STATE
        assert "rt_init" in lib.rt_last_error().decode()
    if lib.rt_device_count() >= 0 or lib.rt_init(1) == 0:
        pytest.skip("a GPU is present")
    assert lib.rt_init(1) == RT_ERR_DEVICE
    with pytest.raises(rt_host.RtError, match="no HIP device visible"):
        rt_host.trace_rays(blob, rays.reshape(1, 6), want=("rgb", "rgba", "hits"), order="binned")
    assert (rgba == 7).all()


@pytest.mark.skipif(not all(os.path.exists(t) for t in TOOLS), reason="ROCm LLVM tools not installed")
def test_order_kernels_resources(built, tmp_path):
    """The bounds, key and sort kernels keep everything in registers and LDS: no scratch, no spills.  The ordered trace is the plain
    trace's kernel with one more argument (tests/test_rays.py holds it to rt_retrace's scratch), so this object holds exactly the five
    kernels of the ordering."""
    found = _resources("rt_rays_order.o", tmp_path)
    names = ("rt_order_bounds", "rt_order_keys", "rt_order_histogram", "rt_order_scan", "rt_order_scatter")
    assert len(found) == len(names) and all(any(n in k for k in found) for n in names), sorted(found)
    for k, v in found.items():
        assert v == {"vgpr_spill_count": 0, "sgpr_spill_count": 0, "private_segment_fixed_size": 0}, (k, v)
    # the ordered trace did not become kernels of its own anywhere
    strict = _resources("rt_kernel_strict.o", tmp_path)
    assert len([k for k in strict if "rt_trace_rays" in k]) == 2, sorted(strict)
    assert not [k for k in _resources("rt_kernel_fast.o", tmp_path) if "rays" in k or "order" in k]
