#!/usr/bin/env python3
"""The soft trace in one launch at 3840x2160 on default14 and H8 (docs/EVIDENCE.md, "Soft trace in one launch").  The list is a PINHOLE
view with the scene's camera, generated once on the device (Renderer.view_rays) and left there.  Lights of radius 1.0, 61 turned sets
with stride n_samples, at 1, 4 and 16 samples and at levels 1 and the scene's depth.
 1. the kernels on that list (rt_stats.kernel_ms), alternating in one run:
      hard               the strict recursive rt_trace_rays (rt_scene_trace_rays_device)
      soft_<n>_<levels>  rt_soft_trace (rt_scene_trace_rays_soft_device): what the soft lights add to a hard frame
 2. the host forms end to end (a host clock) with the kernel time rt_stats reports, alternating in one run:
      view_<n>_<levels>       rt_trace_view_soft: the rays generated on the device, one launch per chunk of rows
      wavefront_<n>_<levels>  rt_trace_rays_soft with host-made rays: what it replaces
Per configuration one warm-up pass, then `reps` passes in which the variants alternate; median, min and max.
   python3 profiles/soft_timing.py [reps] [out.json]"""
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

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 5
w, h, radius = 3840, 2160, 1.0
n = w * h
SAMPLES = (1, 4, 16)
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


d_rays, d_rgba = alloc(n * 48), alloc(n * 4)
tables = {k: turned_copies(rt_host.lighting_offsets(k), COPIES) for k in SAMPLES}
d_tables = {k: upload(t) for k, t in tables.items()}
out = {"w": w, "h": h, "rays": n, "light_radius": radius, "reps": reps, "scenes": {}}
for name in ("default14", "h8"):
    scene = rt_host.load_scene(name)
    cam = scene["camera"]
    v = rt_host.view(rt_host.RT_VIEW_PINHOLE, cam["origin"], cam["axisX"], cam["axisY"], cam["axisZ"], scene["fovDeg"])
    r = rt_host.Renderer(scene, 0, lib)
    r.view_rays(v, w, h, d_rays)
    depth = scene["segs"]
    configs = [(k, lv) for k in SAMPLES for lv in (1, depth)]
    res = {"depth": depth}

    def soft(k, lv):
        return r.trace_rays_soft(n, d_rays, 0, d_rgba, d_tables[k], len(tables[k]), k, radius, stride=k, levels=lv, want_stats=True).kernel_ms

    variants = {"hard": lambda: r.trace_rays(n, d_rays, 0, d_rgba, 0, want_stats=True).kernel_ms}
    for k, lv in configs:
        variants["soft_%d_%d" % (k, lv)] = (lambda k=k, lv=lv: soft(k, lv))
    for f in variants.values():
        f()
    ms = {k: [] for k in variants}
    for _ in range(reps):
        for k, f in variants.items():
            ms[k].append(f())
    res["kernels"] = {k: spread(a) for k, a in ms.items()}
    for k in list(ms):
        if k != "hard":
            res["kernels"][k]["over_hard"] = round(statistics.median(ms[k]) / statistics.median(ms["hard"]), 3)
    print(name, "kernels", json.dumps(res["kernels"]), flush=True)
    r.close()

    # 2. the host forms
    rays = rt_host.view_rays(v, w, h, lib=lib).reshape(-1, 6)
    aligned = rt_host._aligned_f64(n * 6)
    aligned[:] = rays.reshape(-1)
    blob = rt_host.flatten_scene(scene)
    buf = C.create_string_buffer(blob, len(blob))
    rgba = np.empty((n, 4), np.uint8)
    bufs = rt_host.RtRayOutputs(None, rgba.ctypes.data, None)

    def host(form, k, lv):
        a = rt_host.RtLighting(k, len(tables[k]), k, 0, 0, radius)
        offs = np.ascontiguousarray(tables[k])
        st = rt_host.RtStats()
        t0 = time.perf_counter()
        if form == "view":
            rc = lib.rt_trace_view_soft(buf, len(blob), C.byref(v), w, h, C.byref(a), C.c_void_p(offs.ctypes.data), lv, 0, C.byref(bufs), C.byref(st))
        else:
            rc = lib.rt_trace_rays_soft(buf, len(blob), C.byref(a), C.c_void_p(offs.ctypes.data), lv, n, C.c_void_p(aligned.ctypes.data), 0, 0, C.byref(bufs),
                                        C.byref(st), None)
        assert rc == 0, lib.rt_last_error()
        return (time.perf_counter() - t0) * 1e3, st.kernel_ms

    forms = {"%s_%d_%d" % (form, k, lv): (form, k, lv) for k, lv in configs for form in ("view", "wavefront")}
    pictures = {}
    for key, args in forms.items():
        host(*args)
        pictures[key] = rgba.tobytes()
    res["same_bytes"] = all(pictures["view_%d_%d" % c] == pictures["wavefront_%d_%d" % c] for c in configs)
    ms = {k: ([], []) for k in forms}
    for _ in range(reps):
        for key, args in forms.items():
            t, km = host(*args)
            ms[key][0].append(t)
            ms[key][1].append(km)
    res["host_forms"] = {k: {"end_to_end": spread(t), "kernel": spread(km)} for k, (t, km) in ms.items()}
    print(name, "host forms", json.dumps(res["host_forms"]), "same bytes:", res["same_bytes"], flush=True)
    out["scenes"][name] = res

if len(sys.argv) > 2:
    with open(sys.argv[2], "w") as f:
        json.dump(out, f, indent=1)
