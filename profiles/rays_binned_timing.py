#!/usr/bin/env python3
"""What binning a ray list costs and saves (include/rt_hip.h: rt_scene_order_rays_device, rt_scene_trace_rays_ordered_device): the
primary rays of H8 and default14 at 3840x2160 as a list, in row order and under one fixed shuffle, `rgba` only.  Every figure is the
time between two HIP events recorded on the calls' stream around the call(s); median and min of `reps` repetitions after 10 warm-ups.
  (a) the shuffled list through the plain call of the PARENT commit's library (loaded beside this one, same process, same card)
  (b) the row-order list through the parent's plain call
  (c) the ordering alone (rt_scene_order_rays_device) of the shuffled list
  (d) the ordered trace alone, with that order computed beforehand
  (e) (c) + (d) enqueued back to back, timed as one interval
  (f) this commit's plain call on both lists: unchanged against (a) and (b)?
Written down before the first run (8 294 400 rays):
  (c)  176 bytes per ray (rt_rays_order.hip: bounds 48, keys 52, four histograms 16, four scatters 56) = 1.46 GB, 0.37 ms at 4 TB/s, plus
       14 launches of which four scans keep 256 workgroups busy: 0.45 - 0.6 ms.
  (d)  against (b): the rays of a wave are neighbours in space but their records lie anywhere in the list.  A 48-byte record at a
       random 16-byte-aligned address touches 1.25 lines of 128 bytes (160 bytes fetched for 48 used), and its 4-byte result is a
       partial write of a line of its own: about 240 bytes more per ray than the 52 of the row-order list, 2 GB, 0.4 - 0.5 ms on
       top of (b): 0.7 - 0.8 ms on H8, 1.2 - 1.3 ms on default14.
  (e)  their sum: 1.2 - 1.4 ms on H8 (no better than (a), 1.04 ms: a shuffled H8 list is cheap to trace as it is), 1.7 - 1.9 ms on
       default14 against 6.1 ms.
   python3 profiles/rays_binned_timing.py <parent librt_hip.so> [reps] [out.json]"""
import ctypes as C
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "html5-canvas-raytracer_amd"))
import numpy as np
import rt_host

parent_path = sys.argv[1]
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 200
w, h = 3840, 2160
n = w * h
lib = rt_host.load_library()
assert lib.rt_init(1) == 0
os.environ["RT_HIP_LIB_OLDER"] = "1"                   # (the parent exports none of the ordering entry points)
parent = rt_host.load_library(parent_path)
assert parent.rt_init(1) == 0
hip = C.CDLL("libamdhip64.so")
hip.hipEventElapsedTime.argtypes = [C.POINTER(C.c_float), C.c_void_p, C.c_void_p]
stream, ev_a, ev_b = C.c_void_p(), C.c_void_p(), C.c_void_p()
assert hip.hipStreamCreate(C.byref(stream)) == 0 and hip.hipEventCreate(C.byref(ev_a)) == 0 and hip.hipEventCreate(C.byref(ev_b)) == 0


def timed(call):
    def once():
        assert hip.hipEventRecord(ev_a, stream) == 0
        call()
        assert hip.hipEventRecord(ev_b, stream) == 0 and hip.hipEventSynchronize(ev_b) == 0
        ms = C.c_float()
        assert hip.hipEventElapsedTime(C.byref(ms), ev_a, ev_b) == 0
        return ms.value
    for _ in range(10):
        once()
    ms = [once() for _ in range(reps)]
    return {"median_ms": statistics.median(ms), "min_ms": min(ms)}


out = {"w": w, "h": h, "rays": n, "reps": reps, "order_work_bytes": rt_host.rays_order_work_bytes(n), "order_bytes_per_ray_model": 176, "scenes": {}}
for name in ("h8", "default14"):
    scene = rt_host.load_scene(name)
    rays = rt_host.primary_rays(w, h, scene)
    perm = np.random.default_rng(1).permutation(n)
    d_rows, d_shuffled = lib.rt_alloc_device(0, rays.nbytes), lib.rt_alloc_device(0, rays.nbytes)
    for dst, src in ((d_rows, rays), (d_shuffled, np.ascontiguousarray(rays[perm]))):
        assert hip.hipMemcpy(C.c_void_p(dst), src.ctypes.data_as(C.c_void_p), C.c_size_t(src.nbytes), 1) == 0
    work_bytes = rt_host.rays_order_work_bytes(n)
    rgba, rgba_ref, d_order, d_work = (lib.rt_alloc_device(0, b) for b in (4 * n, 4 * n, 4 * n, work_bytes))
    r, rp = rt_host.Renderer(scene, 0, lib), rt_host.Renderer(scene, 0, parent)
    s = stream.value
    res = {}
    res["(a) shuffled, plain call, parent library"] = timed(lambda: rp.trace_rays(n, d_shuffled, 0, rgba_ref, 0, stream=s))
    res["(b) row order, plain call, parent library"] = timed(lambda: rp.trace_rays(n, d_rows, 0, rgba, 0, stream=s))
    res["(c) ordering alone, shuffled"] = timed(lambda: r.order_rays(n, d_shuffled, d_order, d_work, work_bytes, stream=s))
    res["(d) ordered trace alone, shuffled"] = timed(lambda: r.trace_rays_ordered(n, d_shuffled, d_order, 0, rgba, 0, stream=s))

    def both():
        r.order_rays(n, d_shuffled, d_order, d_work, work_bytes, stream=s)
        r.trace_rays_ordered(n, d_shuffled, d_order, 0, rgba, 0, stream=s)
    res["(e) ordering + ordered trace, shuffled"] = timed(both)
    # the results the timed calls left: the binned list's bytes are the parent's plain bytes
    got, want = np.empty(n, np.uint32), np.empty(n, np.uint32)
    assert lib.rt_copy_to_host(0, got.ctypes.data, rgba, 4 * n) == 0 and lib.rt_copy_to_host(0, want.ctypes.data, rgba_ref, 4 * n) == 0
    res["binned bytes equal the parent's plain bytes"] = bool(np.array_equal(got, want))
    res["(f) shuffled, plain call, this library"] = timed(lambda: r.trace_rays(n, d_shuffled, 0, rgba, 0, stream=s))
    res["(f) row order, plain call, this library"] = timed(lambda: r.trace_rays(n, d_rows, 0, rgba, 0, stream=s))
    res["(c) achieved GB/s by the 176-byte model"] = 176.0 * n / (res["(c) ordering alone, shuffled"]["median_ms"] * 1e-3) / 1e9
    r.close()
    rp.close()
    out["scenes"][name] = res
    for p in (d_rows, d_shuffled, rgba, rgba_ref, d_order, d_work):
        lib.rt_free_device(0, p)
print(json.dumps(out, indent=1))
if len(sys.argv) > 3:
    with open(sys.argv[3], "w") as f:
        json.dump(out, f, indent=1)
