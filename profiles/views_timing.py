#!/usr/bin/env python3
"""Views (rt_view_rays_device, rt_scene_trace_view_device, rt_trace_view) at 3840x2160 on default14 and H8 (docs/EVIDENCE.md, "Views"):
 1. the generator alone, per model: time per launch of the whole view and bytes written per second (48 bytes per ray);
 2. rt_scene_trace_view_device - a REFERENCE view with the scene's camera, rgba out - against rt_scene_trace_rays_device on the same
    rays already resident in device memory (made by the generator), for workspaces of 2^16, 2^18, 2^20 rays and the whole view; the
    difference is what generation and the band loop cost;
 3. rt_trace_view against rt_trace_rays with host-made rays (rt_host.primary_rays; the time to build them is reported apart).
Times: 1. a host clock around `launches` launches that end in a device synchronise; 2. rt_stats.kernel_ms (device events around the
call's launches); 3. a host clock around the synchronous call.  Per configuration one warm-up pass, then `reps` passes in which the
variants alternate; median, min and max.
   python3 profiles/views_timing.py [reps] [out.json]"""
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

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 7
w, h = 3840, 2160
n = w * h
launches = 20
lib = rt_host.load_library()
assert lib.rt_init(1) == 0
hip = ctypes.CDLL("libamdhip64.so")


def sync():
    assert hip.hipDeviceSynchronize() == 0


def alloc(nbytes):
    p = lib.rt_alloc_device(0, nbytes)
    assert p, lib.rt_last_error()
    return p


def upload(a):
    p = alloc(a.nbytes)
    assert hip.hipMemcpy(ctypes.c_void_p(p), a.ctypes.data_as(ctypes.c_void_p), ctypes.c_size_t(a.nbytes), 1) == 0
    return p


def spread(ms):
    return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4)}


out = {"w": w, "h": h, "rays": n, "reps": reps, "scenes": {}}
d_rays, d_rgba, d_rgba_ref = alloc(n * 48), alloc(n * 4), alloc(n * 4)
tables = rt_host.equirect_tables(w, h, lib)
d_tables = tuple(upload(t) for t in tables)
for name in ("default14", "h8"):
    scene = rt_host.load_scene(name)
    cam = scene["camera"]
    basis = (cam["origin"], cam["axisX"], cam["axisY"], cam["axisZ"])
    r = rt_host.Renderer(scene, 0, lib)
    res = {}

    # 1. the generator alone
    gen = {}
    for model, label in ((0, "reference"), (1, "pinhole"), (2, "ortho"), (3, "equirect")):
        v = rt_host.view(model, *basis, fov_deg=scene["fovDeg"], scale=0.01, tables=d_tables if model == 3 else None)
        r.view_rays(v, w, h, d_rays)
        sync()
        us = []
        for _ in range(reps):
            t0 = time.perf_counter()
            for _ in range(launches):
                r.view_rays(v, w, h, d_rays)
            sync()
            us.append((time.perf_counter() - t0) * 1e6 / launches)
        gen[label] = {"median_us": round(statistics.median(us), 1), "min_us": round(min(us), 1), "max_us": round(max(us), 1),
                      "gb_per_s_written": round(n * 48 / statistics.median(us) / 1e3, 1)}
    res["generator"] = gen

    # 2. the traced view against the trace of the same rays, resident
    v = rt_host.view(0, *basis, fov_deg=scene["fovDeg"])
    r.view_rays(v, w, h, d_rays)
    sync()
    bands = [("2^16", 1 << 16), ("2^18", 1 << 18), ("2^20", 1 << 20), ("whole view", n)]
    work = {label: 48 * w * max(1, min(h, rays // w)) for label, rays in bands}
    d_work = alloc(max(work.values()))
    r.trace_rays(n, d_rays, 0, d_rgba_ref, 0, want_stats=True)
    for label, _ in bands:
        r.trace_view(v, w, h, 0, d_rgba, 0, d_work, work[label], want_stats=True)
    ms = {label: [] for label, _ in bands}
    ms["trace_rays"] = []
    for _ in range(reps):
        ms["trace_rays"].append(r.trace_rays(n, d_rays, 0, d_rgba_ref, 0, want_stats=True).kernel_ms)
        for label, _ in bands:
            ms[label].append(r.trace_view(v, w, h, 0, d_rgba, 0, d_work, work[label], want_stats=True).kernel_ms)
    a, b = np.empty(n * 4, np.uint8), np.empty(n * 4, np.uint8)
    assert lib.rt_copy_to_host(0, a.ctypes.data, d_rgba, n * 4) == 0 and lib.rt_copy_to_host(0, b.ctypes.data, d_rgba_ref, n * 4) == 0
    res["device"] = {"trace_rays_resident": spread(ms["trace_rays"]), "same_bytes": bool((a == b).all()),
                     "trace_view": {label: dict(spread(ms[label]), rows_per_band=work[label] // (48 * w), work_bytes=work[label],
                                                over_trace_rays_ms=round(statistics.median(ms[label]) - statistics.median(ms["trace_rays"]), 4))
                                    for label, _ in bands}}
    lib.rt_free_device(0, d_work)
    r.close()

    # 3. the host forms, end to end
    t0 = time.perf_counter()
    rays = rt_host.primary_rays(w, h, scene)
    build_ms = (time.perf_counter() - t0) * 1e3
    aligned = np.empty(n * 6 + 2, np.float64)
    aligned = aligned[(aligned.ctypes.data >> 3) & 1:][:n * 6]
    aligned[:] = rays.reshape(-1)
    del rays
    blob = rt_host.flatten_scene(scene)
    buf = ctypes.create_string_buffer(blob, len(blob))
    rgba_a, rgba_b = np.empty((n, 4), np.uint8), np.empty((n, 4), np.uint8)
    oa, ob = rt_host.RtRayOutputs(None, rgba_a.ctypes.data, None), rt_host.RtRayOutputs(None, rgba_b.ctypes.data, None)
    calls = {"rt_trace_rays": lambda: lib.rt_trace_rays(buf, len(blob), n, ctypes.c_void_p(aligned.ctypes.data), 0, ctypes.byref(oa), None),
             "rt_trace_view": lambda: lib.rt_trace_view(buf, len(blob), ctypes.byref(v), w, h, 0, ctypes.byref(ob), None)}
    host = {k: [] for k in calls}
    for k, call in calls.items():
        assert call() == 0, lib.rt_last_error()
    for _ in range(reps):
        for k, call in calls.items():
            t0 = time.perf_counter()
            assert call() == 0
            host[k].append((time.perf_counter() - t0) * 1e3)
    res["host"] = {k: spread(t) for k, t in host.items()}
    res["host"]["same_bytes"] = bool((rgba_a == rgba_b).all())
    res["host"]["primary_rays_numpy_ms"] = round(build_ms, 1)
    res["host"]["ray_bytes_not_shipped"] = n * 48
    del aligned
    out["scenes"][name] = res
print(json.dumps(out, indent=1))
if len(sys.argv) > 2:
    with open(sys.argv[2], "w") as f:
        json.dump(out, f, indent=1)
