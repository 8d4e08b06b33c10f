#!/usr/bin/env python3
"""Relit nodes at 3840x2160 on default14 and H8 (docs/EVIDENCE.md, "Relit nodes").  The list is a PINHOLE view with the scene's camera,
generated once on the device (Renderer.view_rays) and left there with its nodes.
 1. the kernels on level 0 of that list (rt_stats.kernel_ms), alternating in one run:
      shade           rt_nodes_shade (rt_scene_shade_rays_device)
      relight_1       rt_relight_kernel, one sample, light_radius 0 (the shade's own light loop again)
      relight_4/16    4 / 16 samples, light_radius 1.0, 61 turned sets with stride n_samples (vector loads of the table)
      relight_16_same 16 samples, light_radius 1.0, 16 offsets with stride 0 (scalar loads of the table)
 2. the host forms end to end (a host clock; the rays cross the link in all three), alternating in one run:
      wavefront       rt_trace_rays_wavefront
      soft_1_level    rt_trace_rays_soft, levels 1, 16 samples, turned sets
      soft_all_levels rt_trace_rays_soft, levels = the scene's depth
    with the kernel time rt_stats reports for each.
Per configuration one warm-up pass, then `reps` passes in which the variants alternate; median, min and max.
   python3 profiles/relight_timing.py [reps] [out.json]"""
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "html5-canvas-raytracer_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np
import rt_host
from soft_shadows import COPIES, turned_copies

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 7
w, h, radius = 3840, 2160, 1.0
n = w * h
lib = rt_host.load_library()
assert lib.rt_init(1) == 0
hip = C.CDLL("libamdhip64.so")


def alloc(nbytes):
    p = lib.rt_alloc_device(0, nbytes)
    assert p, lib.rt_last_error()
    return p


def upload(a):
    a = np.ascontiguousarray(a)
    p = alloc(max(a.nbytes, 16))
    assert hip.hipMemcpy(C.c_void_p(p), a.ctypes.data_as(C.c_void_p), C.c_size_t(a.nbytes), 1) == 0
    return p


def spread(ms):
    return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4)}


d_rays, d_nodes = alloc(n * 48), alloc(n * 200)
tables = {k: turned_copies(rt_host.lighting_offsets(k), COPIES) for k in (4, 16)}
same = rt_host.lighting_offsets(16)
d_tables, d_same = {k: upload(t) for k, t in tables.items()}, upload(same)
out = {"w": w, "h": h, "nodes": n, "light_radius": radius, "reps": reps, "scenes": {}}
for name in ("default14", "h8"):
    scene = rt_host.load_scene(name)
    cam = scene["camera"]
    v = rt_host.view(rt_host.RT_VIEW_PINHOLE, cam["origin"], cam["axisX"], cam["axisY"], cam["axisZ"], scene["fovDeg"])
    r = rt_host.Renderer(scene, 0, lib)
    r.view_rays(v, w, h, d_rays)
    res = {}

    def relight(d_offs, n_offs, samples, rad, stride):
        return r.relight_nodes(n, d_rays, d_nodes, d_offs, n_offs, samples, rad, stride=stride, want_stats=True).kernel_ms

    variants = {"shade": lambda: r.shade_rays(n, d_rays, d_nodes, want_stats=True).kernel_ms,
                "relight_1": lambda: relight(0, 1, 1, 0.0, 1),
                "relight_4": lambda: relight(d_tables[4], len(tables[4]), 4, radius, 4),
                "relight_16": lambda: relight(d_tables[16], len(tables[16]), 16, radius, 16),
                "relight_16_same": lambda: relight(d_same, 16, 16, radius, 0)}
    for f in variants.values():
        f()
    ms = {k: [] for k in variants}
    for _ in range(reps):
        for k, f in variants.items():
            ms[k].append(f())
    for k, a in ms.items():
        res[k] = spread(a)
    res["relight_16_over_16_relight_1"] = round(statistics.median(ms["relight_16"]) / (16 * statistics.median(ms["relight_1"])), 3)
    res["relight_1_over_shade"] = round(statistics.median(ms["relight_1"]) / statistics.median(ms["shade"]), 3)
    print(name, json.dumps(res), flush=True)

    # 2. the host forms
    rays = rt_host.view_rays(v, w, h, lib=lib).reshape(-1, 6)
    aligned = rt_host._aligned_f64(n * 6)
    aligned[:] = rays.reshape(-1)
    blob = rt_host.flatten_scene(scene)
    buf = C.create_string_buffer(blob, len(blob))
    rgba = np.empty((n, 4), np.uint8)
    bufs = rt_host.RtRayOutputs(None, rgba.ctypes.data, None)
    a = rt_host.RtLighting(16, len(tables[16]), 16, 0, 0, radius)
    offs = np.ascontiguousarray(tables[16])

    def host(levels):
        st = rt_host.RtStats()
        t0 = time.perf_counter()
        if levels is None:
            rc = lib.rt_trace_rays_wavefront(buf, len(blob), n, C.c_void_p(aligned.ctypes.data), 0, 0, C.byref(bufs), C.byref(st), None)
        else:
            rc = lib.rt_trace_rays_soft(buf, len(blob), C.byref(a), C.c_void_p(offs.ctypes.data), levels, n, C.c_void_p(aligned.ctypes.data), 0, 0, C.byref(bufs),
                                        C.byref(st), None)
        assert rc == 0, lib.rt_last_error()
        return (time.perf_counter() - t0) * 1e3, st.kernel_ms

    forms = {"wavefront": None, "soft_1_level": 1, "soft_all_levels": scene["segs"]}
    for lv in forms.values():
        host(lv)
    ms = {k: ([], []) for k in forms}
    for _ in range(reps):
        for k, lv in forms.items():
            t, km = host(lv)
            ms[k][0].append(t)
            ms[k][1].append(km)
    res["host_forms"] = {k: {"end_to_end": spread(t), "kernel": spread(km)} for k, (t, km) in ms.items()}
    print(name, "host forms", json.dumps(res["host_forms"]), flush=True)
    out["scenes"][name] = res
    r.close()

if len(sys.argv) > 2:
    with open(sys.argv[2], "w") as f:
        json.dump(out, f, indent=1)
