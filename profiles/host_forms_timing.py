#!/usr/bin/env python3
"""The host forms end to end (docs/EVIDENCE.md, "Host forms: one driver"): a host clock around one call of each, default14 at 3840 x 2160,
which is 32 chunks of 2^18 units.  What a call costs beside its kernels - the prologue, the allocations, the copies of each chunk,
the waits - is what a change of the host layer can move; the kernels and their launches are the same.
 lists:  rt_trace_rays (rgba), rt_ambient and rt_lighting of the view's hit records (16 samples; 1024 entries walked with stride 7),
         rt_trace_rays_soft_recursive (4 samples, one level; rgba), plain and binned
 views:  rt_trace_view (rgba), rt_ambient_view, rt_lighting_view (as the lists), rt_trace_view_soft (as the list)
One warm-up call of each, then `reps` passes in which the forms alternate; median, min and max per form, and a digest of every
form's bytes.  Two libraries are compared by running this script once per library (RT_HIP_LIB) and round, alternating.
   python3 profiles/host_forms_timing.py [reps] [out.json]"""
import hashlib
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "html5-canvas-raytracer_amd"))
import numpy as np
import rt_host

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 9
w, h = 3840, 2160
lib = rt_host.load_library()
assert lib.rt_init(1) == 0
scene = rt_host.flatten_scene(rt_host.load_scene("default14"))
s = rt_host.load_scene("default14")
cam = s["camera"]
v = rt_host.view(rt_host.RT_VIEW_PINHOLE, cam["origin"], cam["axisX"], cam["axisY"], cam["axisZ"], s["fovDeg"])
rays = rt_host.view_rays(v, w, h, lib=lib).reshape(-1, 6)
hits = rt_host.view_hit_records(scene, v, w, h, lib=lib)
dirs, offs = rt_host.ambient_dirs(1024, lib), rt_host.lighting_offsets(1024, lib)
soft = dict(offs=offs[:64], stride=7, levels=1, want=("rgba",), method="recursive", lib=lib)

FORMS = {
    "list_trace_rays": lambda: rt_host.trace_rays(scene, rays, want=("rgba",), lib=lib),
    "list_ambient": lambda: rt_host.ambient(scene, hits, 16, 2.0, dirs=dirs, stride=7, want=("rgba",), lib=lib),
    "list_lighting": lambda: rt_host.lighting(scene, hits, 16, 0.5, offs=offs, stride=7, want=("rgba",), lib=lib),
    "list_soft_recursive": lambda: rt_host.trace_rays_soft(scene, rays, 4, 0.5, **soft),
    "list_soft_recursive_binned": lambda: rt_host.trace_rays_soft(scene, rays, 4, 0.5, order="binned", **soft),
    "view_trace": lambda: rt_host.trace_view(scene, v, w, h, want=("rgba",), lib=lib),
    "view_ambient": lambda: rt_host.ambient_view(scene, v, w, h, 16, 2.0, dirs=dirs, stride=7, lib=lib),
    "view_lighting": lambda: rt_host.lighting_view(scene, v, w, h, 16, 0.5, offs=offs, stride=7, lib=lib),
    "view_soft": lambda: rt_host.trace_view_soft(scene, v, w, h, 4, 0.5, **soft),
}

digest = {k: hashlib.sha256(np.ascontiguousarray(f()["rgba"]).tobytes()).hexdigest()[:16] for k, f in FORMS.items()}   # (the warm-up)
ms = {k: [] for k in FORMS}
for _ in range(reps):
    for k, f in FORMS.items():
        t0 = time.perf_counter()
        f()
        ms[k].append((time.perf_counter() - t0) * 1e3)
out = {"w": w, "h": h, "reps": reps, "library": os.environ.get("RT_HIP_LIB", "product"),
       "forms": {k: {"median_ms": round(statistics.median(a), 3), "min_ms": round(min(a), 3), "max_ms": round(max(a), 3), "rgba_sha256_16": digest[k]}
                 for k, a in ms.items()}}
print(json.dumps(out), flush=True)
if len(sys.argv) > 2:
    with open(sys.argv[2], "w") as f:
        json.dump(out, f, indent=1)
