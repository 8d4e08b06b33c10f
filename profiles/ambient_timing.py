#!/usr/bin/env python3
"""Ambient occlusion at 3840x2160, 16 samples per receiver, radius 2.0, on default14 and H8 (docs/EVIDENCE.md, "Ambient occlusion").
The receivers are the hit records of a PINHOLE view with the scene's camera, written once by Renderer.trace_view and left in device
memory.  Two tables: 1024 directions walked with stride 7, and 16 directions with stride 0 (every receiver the
same 16: the fused kernel's scalar-load branch).
 1. the fused kernel, rt_scene_ambient_device: rt_stats.kernel_ms, with the intensity output alone (what the composition below
    computes) and with all three outputs;
 2. the unfused composition on the same receivers, per sample: rt_ambient_segments_device (rays and skips into device memory; a host
    clock around the launch and a synchronise, the entry point reports no stats), rt_scene_occlusion_device (length = 2.0 and intensity =
    1.0 from device arrays, the generator's skips; intensity out; rt_stats.kernel_ms), and for samples 1..15 one addition of the sample's
    intensities into an accumulator - the library's own accumulate kernel (rt_view_samples.hip), timed with device events.  No count of
    open scans and no division: less than the fused kernel does;
 3. the host form rt_ambient_view end to end (rgba out): a host clock around rt_host.ambient_view.
Per configuration one warm-up pass, then `reps` passes in which the variants alternate; median, min and max.
   python3 profiles/ambient_timing.py [reps] [out.json]"""
import ctypes as C
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
w, h, n_samples, radius = 3840, 2160, 16, 2.0
n = w * h
assert n % 3 == 0                                     # (the accumulate kernel adds 3 doubles per "pixel")
lib = rt_host.load_library()
assert lib.rt_init(1) == 0
hip = C.CDLL("libamdhip64.so")
lib.rt_launch_view_accumulate.restype = C.c_int
lib.rt_launch_view_accumulate.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p]


def alloc(nbytes):
    p = lib.rt_alloc_device(0, nbytes)
    assert p, lib.rt_last_error()
    return p


def upload(a):
    a = np.ascontiguousarray(a)
    p = alloc(a.nbytes)
    assert hip.hipMemcpy(C.c_void_p(p), a.ctypes.data_as(C.c_void_p), C.c_size_t(a.nbytes), 1) == 0
    return p


def spread(ms):
    return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4)}


ev = [C.c_void_p(), C.c_void_p()]
for e in ev:
    assert hip.hipEventCreate(C.byref(e)) == 0


def add_ms(d_acc, d_li):
    """acc += li over n doubles on the NULL stream, by device events"""
    assert hip.hipEventRecord(ev[0], None) == 0
    assert lib.rt_launch_view_accumulate(d_acc, d_li, n // 3, None) == 0
    assert hip.hipEventRecord(ev[1], None) == 0
    assert hip.hipEventSynchronize(ev[1]) == 0
    ms = C.c_float()
    assert hip.hipEventElapsedTime(C.byref(ms), ev[0], ev[1]) == 0
    return ms.value


d_hits, d_rays, d_skip = alloc(n * 80), alloc(n * 48), alloc(n * 4)
d_open, d_li, d_acc, d_rgba = alloc(n * 8), alloc(n * 8), alloc(n * 8), alloc(n * 4)
d_length, d_one = upload(np.full(n, radius)), upload(np.ones(n))
out = {"w": w, "h": h, "receivers": n, "n_samples": n_samples, "radius": radius, "reps": reps, "scenes": {}}
for name in ("default14", "h8"):
    scene = rt_host.load_scene(name)
    cam = scene["camera"]
    v = rt_host.view(rt_host.RT_VIEW_PINHOLE, cam["origin"], cam["axisX"], cam["axisY"], cam["axisZ"], scene["fovDeg"])
    r = rt_host.Renderer(scene, 0, lib)
    r.trace_view(v, w, h, 0, 0, d_hits, d_rays, 48 * n, want_stats=True)           # the receivers (d_rays is the workspace here)
    res = {}
    for label, n_dirs, stride in (("walk_1024_stride_7", 1024, 7), ("same_16_stride_0", 16, 0)):
        dirs = rt_host.ambient_dirs(n_dirs)
        d_dirs = upload(dirs)

        def fused(all_outputs):
            return r.ambient(n, d_hits, d_dirs, n_dirs, n_samples, radius, d_open if all_outputs else 0, d_li, d_rgba if all_outputs else 0, stride=stride,
                             want_stats=True).kernel_ms

        def unfused():
            parts = {"segments": 0.0, "occlusion": 0.0, "add": 0.0}
            for s in range(n_samples):
                assert hip.hipDeviceSynchronize() == 0
                t0 = time.perf_counter()
                r.ambient_segments(n, d_hits, d_dirs, n_dirs, s, d_rays, d_skip, n_samples=n_samples, stride=stride)
                assert hip.hipDeviceSynchronize() == 0
                parts["segments"] += (time.perf_counter() - t0) * 1e3
                parts["occlusion"] += r.occlusion(n, d_rays, d_length, d_one, d_skip, d_acc if s == 0 else d_li, 0, want_stats=True).kernel_ms
                if s:
                    parts["add"] += add_ms(d_acc, d_li)
            return parts

        fused(False), fused(True), unfused()
        ms = {"fused_intensity": [], "fused_all": [], "unfused": [], "segments": [], "occlusion": [], "add": []}
        for _ in range(reps):
            ms["fused_intensity"].append(fused(False))
            p = unfused()
            ms["unfused"].append(sum(p.values()))
            for k in p:
                ms[k].append(p[k])
            ms["fused_all"].append(fused(True))
        res[label] = {k: spread(a) for k, a in ms.items()}
        res[label]["unfused_over_fused_intensity"] = round(statistics.median(ms["unfused"]) / statistics.median(ms["fused_intensity"]), 3)
        # the two routes agree: the accumulator over n_samples is the fused intensity
        acc, li = np.empty(n), np.empty(n)
        assert lib.rt_copy_to_host(0, acc.ctypes.data, d_acc, n * 8) == 0
        fused(False)
        assert lib.rt_copy_to_host(0, li.ctypes.data, d_li, n * 8) == 0
        res[label]["same_bytes"] = bool((acc / float(n_samples)).tobytes() == li.tobytes())
        lib.rt_free_device(0, d_dirs)
        print(name, label, json.dumps(res[label]), flush=True)
    # 3. the host form, end to end
    dirs = rt_host.ambient_dirs(1024)
    rt_host.ambient_view(scene, v, w, h, n_samples, radius, dirs=dirs, stride=7, lib=lib)
    host = []
    for _ in range(reps):
        t0 = time.perf_counter()
        rt_host.ambient_view(scene, v, w, h, n_samples, radius, dirs=dirs, stride=7, lib=lib)
        host.append((time.perf_counter() - t0) * 1e3)
    res["host_form_ambient_view_rgba"] = spread(host)
    print(name, "host form", json.dumps(res["host_form_ambient_view_rgba"]), flush=True)
    out["scenes"][name] = res
    r.close()

if len(sys.argv) > 2:
    with open(sys.argv[2], "w") as f:
        json.dump(out, f, indent=1)
