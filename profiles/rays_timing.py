#!/usr/bin/env python3
"""Kernel time of rt_scene_trace_rays_device (HIP events around the call's launches, rt_stats.kernel_ms): the primary rays of H8 and
default14 at 3840x2160 as a ray list with (a) rgba only, (b) rgb only, (c) rgb + rgba + hits, and one shuffled copy of the list (fixed
permutation, rgba only) - beside the RT_FLAG_STRICT_FP frame of the same scene and size, which is the same arithmetic without the
48 B read and 4 - 108 B write per ray and with the primary-ray cull.  Median and min of `reps` repetitions after 10 warm-ups.
   python3 profiles/rays_timing.py [reps] [out.json] [parent library: the strict frame is also timed with that librt_hip.so]"""
import json, os, statistics, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "html5-canvas-raytracer_amd"))
import ctypes
import numpy as np
import rt_host
reps = int(sys.argv[1]) if len(sys.argv) > 1 else 200
parent_path = sys.argv[3] if len(sys.argv) > 3 else None
w, h = 3840, 2160
n = w * h
lib = rt_host.load_library()
assert lib.rt_init(1) == 0
parent = None
if parent_path:
    os.environ["RT_HIP_LIB_OLDER"] = "1"               # (it does not export the ray entry points)
    parent = rt_host.load_library(parent_path)
    assert parent.rt_init(1) == 0


def timed(call):
    for _ in range(10):
        call()
    ms = [call().kernel_ms for _ in range(reps)]
    return {"median_ms": statistics.median(ms), "min_ms": min(ms)}


out = {"w": w, "h": h, "rays": n, "reps": reps, "scenes": {}}
for name in ("h8", "default14"):
    scene = rt_host.load_scene(name)
    rays = rt_host.primary_rays(w, h, scene)
    perm = np.random.default_rng(1).permutation(n)
    hip = ctypes.CDLL("libamdhip64.so")
    d_rays, d_shuffled = lib.rt_alloc_device(0, rays.nbytes), lib.rt_alloc_device(0, rays.nbytes)
    for dst, src in ((d_rays, rays), (d_shuffled, np.ascontiguousarray(rays[perm]))):
        assert hip.hipMemcpy(ctypes.c_void_p(dst), src.ctypes.data_as(ctypes.c_void_p), ctypes.c_size_t(src.nbytes), 1) == 0
    rgb, rgba, hits, frame = (lib.rt_alloc_device(0, n * b) for b in (24, 4, 80, 4))
    r = rt_host.Renderer(scene, 0, lib)
    res = {}
    cases = {"rgba only": (0, rgba, 0), "rgb only": (rgb, 0, 0), "rgb + rgba + hits": (rgb, rgba, hits)}
    for case, ptrs in cases.items():
        res[case] = timed(lambda: r.trace_rays(n, d_rays, *ptrs, want_stats=True))
        res[case]["bytes_per_ray"] = 48 + (24 if ptrs[0] else 0) + (4 if ptrs[1] else 0) + (80 if ptrs[2] else 0) + (48 if ptrs[2] else 0)   # (the hit kernel reads the list again)
    res["rgba only, shuffled list"] = timed(lambda: r.trace_rays(n, d_shuffled, 0, rgba, 0, want_stats=True))
    res["strict frame"] = timed(lambda: r.render_tiles(w, h, frame, flags=rt_host.RT_FLAG_STRICT_FP, want_stats=True))
    r.close()
    if parent is not None:
        rp = rt_host.Renderer(scene, 0, parent)
        res["strict frame, parent library"] = timed(lambda: rp.render_tiles(w, h, frame, flags=rt_host.RT_FLAG_STRICT_FP, want_stats=True))
        rp.close()
    yard = res.get("strict frame, parent library", res["strict frame"])["median_ms"]
    for case in list(cases) + ["rgba only, shuffled list"]:
        res[case]["ratio_to_strict_frame"] = res[case]["median_ms"] / yard
    out["scenes"][name] = res
    for p in (rgb, rgba, hits, frame, d_rays, d_shuffled):
        lib.rt_free_device(0, p)
print(json.dumps(out, indent=1))
if len(sys.argv) > 2:
    with open(sys.argv[2], "w") as f:
        json.dump(out, f, indent=1)
