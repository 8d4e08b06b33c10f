#!/usr/bin/env python3
"""Sampled views (rt_scene_trace_view_samples_device) at 3840x2160 on default14 and H8 (docs/EVIDENCE.md, "Sampled views"), a PINHOLE
view with the scene's camera, rgba out, the k x k grid pattern for k = 1..4:
 1. the sampled trace with the whole view as one band, rt_stats.kernel_ms, beside n = k k calls of Renderer.trace_view (the traces
    alone: what exists without the feature on the device; their kernel_ms added up).  k = 1 is the control: the same trace as
    trace_view plus one resolve launch;
 2. for k = 2, one band against bands of 2^20 pixels (273 rows);
 3. the host route that exists without the feature: per sample a host-made ray list (here the library's own probe, timed apart)
    through rt_trace_rays with rgb out, added up and divided in numpy - a host clock around trace and mean, `host_reps` passes.
Per configuration one warm-up pass, then `reps` passes in which the variants alternate; median, min and max.
   python3 profiles/view_samples_timing.py [reps] [out.json] [host_reps]
   python3 profiles/view_samples_timing.py kernels      five k = 2 sampled traces of default14 and nothing else: the process a kernel
                                                        trace is taken of, for the accumulate and resolve launches by themselves"""
import ctypes
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "html5-canvas-raytracer_amd"))
import numpy as np
import rt_host

kernels_only = len(sys.argv) > 1 and sys.argv[1] == "kernels"
reps = int(sys.argv[1]) if len(sys.argv) > 1 and not kernels_only else 7
host_reps = int(sys.argv[3]) if len(sys.argv) > 3 else 3
w, h = 3840, 2160
px = w * h
lib = rt_host.load_library()
assert lib.rt_init(1) == 0
hip = ctypes.CDLL("libamdhip64.so")


def alloc(nbytes):
    p = lib.rt_alloc_device(0, nbytes)
    assert p, lib.rt_last_error()
    return p


def spread(ms):
    return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4)}


def scene_view(name):
    scene = rt_host.load_scene(name)
    cam = scene["camera"]
    return scene, rt_host.view(rt_host.RT_VIEW_PINHOLE, cam["origin"], cam["axisX"], cam["axisY"], cam["axisZ"], scene["fovDeg"])


d_rgba, d_rgba_ref = alloc(px * 4), alloc(px * 4)
work_bytes = rt_host.view_samples_work_bytes(w, h)
d_work = alloc(work_bytes)

if kernels_only:
    scene, v = scene_view("default14")
    r = rt_host.Renderer(scene, 0, lib)
    for _ in range(5):
        r.trace_view_samples(v, w, h, rt_host.view_samples_grid(2), None, 0, d_rgba, d_work, work_bytes, want_stats=True)
    r.close()
    sys.exit(0)

out = {"w": w, "h": h, "pixels": px, "reps": reps, "host_reps": host_reps, "work_bytes_whole_view": work_bytes, "scenes": {}}
band_rows = (1 << 20) // w
for name in ("default14", "h8"):
    scene, v = scene_view(name)
    r = rt_host.Renderer(scene, 0, lib)
    res = {"device": {}, "bands_k2": {}, "host": {}}

    # 1. the sampled trace beside n calls of trace_view
    for k in (1, 2, 3, 4):
        samples = rt_host.view_samples_grid(k)
        sampled = lambda: r.trace_view_samples(v, w, h, samples, None, 0, d_rgba, d_work, work_bytes, want_stats=True).kernel_ms
        plain = lambda: sum(r.trace_view(v, w, h, 0, d_rgba_ref, 0, d_work, 48 * px, want_stats=True).kernel_ms for _ in range(k * k))
        sampled(), plain()
        ms = {"sampled": [], "n_trace_views": []}
        for _ in range(reps):
            ms["sampled"].append(sampled())
            ms["n_trace_views"].append(plain())
        res["device"]["k%d" % k] = {"samples": k * k, "trace_view_samples": spread(ms["sampled"]), "n_calls_of_trace_view": spread(ms["n_trace_views"]),
                                    "over_the_traces_ms": round(statistics.median(ms["sampled"]) - statistics.median(ms["n_trace_views"]), 4)}
        if k == 1:
            a, b = np.empty(px * 4, np.uint8), np.empty(px * 4, np.uint8)
            assert lib.rt_copy_to_host(0, a.ctypes.data, d_rgba, px * 4) == 0 and lib.rt_copy_to_host(0, b.ctypes.data, d_rgba_ref, px * 4) == 0
            res["device"]["k1"]["same_bytes_as_trace_view"] = bool((a == b).all())

    # 2. one band against bands of 2^20 pixels
    samples = rt_host.view_samples_grid(2)
    sizes = {"whole view": work_bytes, "2^20 pixels": 96 * w * band_rows}
    ms = {label: [] for label in sizes}
    for label, nbytes in sizes.items():
        r.trace_view_samples(v, w, h, samples, None, 0, d_rgba, d_work, nbytes, want_stats=True)
    for _ in range(reps):
        for label, nbytes in sizes.items():
            ms[label].append(r.trace_view_samples(v, w, h, samples, None, 0, d_rgba, d_work, nbytes, want_stats=True).kernel_ms)
    res["bands_k2"] = {label: dict(spread(ms[label]), work_bytes=sizes[label], rows_per_band=min(h, sizes[label] // (96 * w))) for label in sizes}
    frame = np.empty(px * 4, np.uint8)
    assert lib.rt_copy_to_host(0, frame.ctypes.data, d_rgba, px * 4) == 0
    r.close()

    # 3. the host route: n lists through rt_trace_rays, numpy's mean
    blob = rt_host.flatten_scene(scene)
    buf = ctypes.create_string_buffer(blob, len(blob))
    rays = rt_host._aligned_f64(px * 6)
    rgb, acc = np.empty((px, 3), np.float64), np.empty((px, 3), np.float64)
    bufs = rt_host.RtRayOutputs(rgb.ctypes.data, None, None)
    for k in (1, 2, 3, 4):
        samples = rt_host.view_samples_grid(k)
        build, route = [], []
        for rep in range(host_reps + 1):                       # (the first pass warms up)
            t_build = t_route = 0.0
            for i, s in enumerate(samples):
                t0 = time.perf_counter()
                assert lib.rt_view_sample_rays(ctypes.byref(v), w, h, None, ctypes.byref(s), 0, 0, h, ctypes.c_void_p(rays.ctypes.data)) == 0
                t1 = time.perf_counter()
                assert lib.rt_trace_rays(buf, len(blob), px, ctypes.c_void_p(rays.ctypes.data), 0, ctypes.byref(bufs), None) == 0, lib.rt_last_error()
                if i == 0:
                    acc[:] = rgb
                else:
                    np.add(acc, rgb, out=acc)
                t_build += t1 - t0
                t_route += time.perf_counter() - t1
            t0 = time.perf_counter()
            mean = acc / float(len(samples))
            t_route += time.perf_counter() - t0
            if rep:
                build.append(t_build * 1e3)
                route.append(t_route * 1e3)
        res["host"]["k%d" % k] = {"samples": k * k, "trace_rays_and_numpy_mean": spread(route), "building_the_lists": spread(build),
                                  "ray_bytes_shipped": 48 * px * k * k}
        if k == 2:
            # the same picture: sample s of the host route draws pix = i, not s w h + i, so only a scene without stars compares
            v8 = 255.0 * mean
            host_frame = np.full((px, 4), 255, np.uint8)
            host_frame[:, :3] = np.rint(np.clip(np.where(np.isnan(v8), 0.0, v8), 0.0, 255.0)).astype(np.uint8)
            res["host"]["k2"]["same_bytes_as_the_device_form"] = bool((host_frame.reshape(-1) == frame).all())
    out["scenes"][name] = res
print(json.dumps(out, indent=1))
if len(sys.argv) > 2:
    with open(sys.argv[2], "w") as f:
        json.dump(out, f, indent=1)
