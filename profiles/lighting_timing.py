#!/usr/bin/env python3
"""Sampled lights at 3840x2160 on default14 and H8 (docs/EVIDENCE.md, "Sampled lights").  The receivers are the hit records of a
PINHOLE view with the scene's camera, written once by Renderer.trace_view and left in device memory.
 1. the fused kernel, rt_scene_lighting_device (rt_stats.kernel_ms, all four outputs):
      point_1         one sample, light_radius 0: the reference's own light loop
      soft_16_same    16 samples, light_radius 1.0, 16 offsets with stride 0 (every receiver the same 16: scalar loads of the table)
      soft_16_sets    16 samples, light_radius 1.0, 61 turned sets of 16 offsets with stride 16 (vector loads of the table)
 2. beside them, the existing parts at 960x540, the most the host probe builds quickly: rt_scene_occlusion_device over device copies of
    the host-built segments of ONE light (the receivers that face it: rays, lengths, skips; the scene's intensity), rt_stats.kernel_ms,
    and the fused kernel's point_1 on the same receivers - each divided by the number of scans it makes (the fused kernel's: the
    facing (receiver, light) pairs of both lights).  The parts' figure leaves out what they cost beyond the scan: building the segments
    on the host, 48 + 16 + 4 bytes per segment over the link per light, the masked subset, the chaining of the intensity.
 3. the host form rt_lighting_view end to end (rgba out; 16 samples, radius 1.0, turned sets): a host clock around rt_host.lighting_view.
Per configuration one warm-up pass, then `reps` passes in which the variants alternate; median, min and max.
   python3 profiles/lighting_timing.py [reps] [out.json]"""
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
w, h, n_samples, radius = 3840, 2160, 16, 1.0
sw, sh = 960, 540
n, sn = w * h, sw * sh
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


d_hits, d_work = alloc(n * 80), alloc(n * 48)
d_diffuse, d_li, d_lit, d_rgba = alloc(n * 8), alloc(n * 8), alloc(n * 8), alloc(n * 4)
same = rt_host.lighting_offsets(n_samples)
sets = turned_copies(same, COPIES)
d_same, d_sets = upload(same), upload(sets)
out = {"w": w, "h": h, "receivers": n, "n_samples": n_samples, "light_radius": radius, "reps": reps, "scenes": {}}
for name in ("default14", "h8"):
    scene = rt_host.load_scene(name)
    cam = scene["camera"]
    v = rt_host.view(rt_host.RT_VIEW_PINHOLE, cam["origin"], cam["axisX"], cam["axisY"], cam["axisZ"], scene["fovDeg"])
    r = rt_host.Renderer(scene, 0, lib)
    res = {}

    def fused(count, d_offs, n_offs, samples, rad, stride):
        return r.lighting(count, d_hits, d_offs, n_offs, samples, rad, d_diffuse, d_li, d_lit, d_rgba, stride=stride, want_stats=True).kernel_ms

    # 2. first, while d_hits holds the small view: the parts and the fused kernel per scan at 960x540
    r.trace_view(v, sw, sh, 0, 0, d_hits, d_work, 48 * sn, want_stats=True)
    hits = np.zeros(sn, np.dtype(rt_host.HIT_FIELDS))
    assert lib.rt_copy_to_host(0, hits.ctypes.data, d_hits, sn * 80) == 0
    n_lights = len(scene["lights"])
    segs = [rt_host.lighting_segments(scene, hits, 0, k, 1, 0.0, lib=lib) for k in range(n_lights)]
    m = segs[0]["mask"]
    scans_one, scans_all = int(m.sum()), int(sum(int(s["mask"].sum()) for s in segs))
    aligned = np.empty(scans_one * 6 + 2, np.float64)
    aligned = aligned[(aligned.ctypes.data >> 3) & 1:][:scans_one * 6]
    aligned[:] = segs[0]["rays"][m].reshape(-1)
    d_rays, d_len, d_skip, d_out = upload(aligned), upload(segs[0]["length"][m]), upload(segs[0]["skip"][m]), alloc(scans_one * 8)
    assert d_rays % 16 == 0

    def parts():
        return r.occlusion(scans_one, d_rays, d_len, 0, d_skip, d_out, 0, want_stats=True).kernel_ms

    parts(), fused(sn, 0, 1, 1, 0.0, 1)
    ms = {"occlusion_one_light": [], "fused_point_1": []}
    for _ in range(reps):
        ms["occlusion_one_light"].append(parts())
        ms["fused_point_1"].append(fused(sn, 0, 1, 1, 0.0, 1))
    res["at_960x540"] = {k: spread(a) for k, a in ms.items()}
    res["at_960x540"].update({"receivers": sn, "scans_one_light": scans_one, "scans_all_lights": scans_all,
                              "occlusion_ns_per_scan": round(statistics.median(ms["occlusion_one_light"]) * 1e6 / scans_one, 4),
                              "fused_ns_per_scan": round(statistics.median(ms["fused_point_1"]) * 1e6 / scans_all, 4)})
    # ... the two routes agree on the first light's receivers that the second light does not face (their intensity is the first scan's)
    li_parts, li_fused = np.empty(scans_one), np.empty(sn)
    assert lib.rt_copy_to_host(0, li_parts.ctypes.data, d_out, scans_one * 8) == 0
    assert lib.rt_copy_to_host(0, li_fused.ctypes.data, d_li, sn * 8) == 0
    only = m & ~np.any([s["mask"] for s in segs[1:]], axis=0) if n_lights > 1 else m
    res["at_960x540"]["same_bytes"] = bool(li_fused[only].tobytes() == li_parts[only[m]].tobytes())
    for p in (d_rays, d_len, d_skip, d_out):
        lib.rt_free_device(0, p)
    print(name, "960x540", json.dumps(res["at_960x540"]), flush=True)

    # 1. the fused kernel at 3840x2160
    r.trace_view(v, w, h, 0, 0, d_hits, d_work, 48 * n, want_stats=True)
    variants = {"point_1": (0, 1, 1, 0.0, 1), "soft_16_same": (d_same, len(same), n_samples, radius, 0), "soft_16_sets": (d_sets, len(sets), n_samples, radius, n_samples)}
    for a in variants.values():
        fused(n, *a)
    ms = {k: [] for k in variants}
    for _ in range(reps):
        for k, a in variants.items():
            ms[k].append(fused(n, *a))
    for k, a in ms.items():
        res[k] = spread(a)
    res["soft_16_sets_over_16_point_1"] = round(statistics.median(ms["soft_16_sets"]) / (16 * statistics.median(ms["point_1"])), 3)
    print(name, json.dumps({k: res[k] for k in list(variants) + ["soft_16_sets_over_16_point_1"]}), flush=True)

    # 3. the host form, end to end
    rt_host.lighting_view(scene, v, w, h, n_samples, radius, offs=sets, stride=n_samples, lib=lib)
    host = []
    for _ in range(reps):
        t0 = time.perf_counter()
        rt_host.lighting_view(scene, v, w, h, n_samples, radius, offs=sets, stride=n_samples, lib=lib)
        host.append((time.perf_counter() - t0) * 1e3)
    res["host_form_lighting_view_rgba"] = spread(host)
    print(name, "host form", json.dumps(res["host_form_lighting_view_rgba"]), flush=True)
    out["scenes"][name] = res
    r.close()

if len(sys.argv) > 2:
    with open(sys.argv[2], "w") as f:
        json.dump(out, f, indent=1)
