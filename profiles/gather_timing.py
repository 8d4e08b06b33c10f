#!/usr/bin/env python3
"""Gathered light at 3840x2160, 16 samples per receiver, on default14 and H8 (docs/EVIDENCE.md, "Gathered light").  The receivers are
the hit records of a PINHOLE view with the scene's camera, written once by Renderer.trace_view and left in device memory.  Two tables:
16 directions with stride 0 (every receiver the same 16: the fused kernel's scalar-load branch, and the coherent case), and the 61
turned copies of the 16-point spiral with stride 16 that tools/bleed.py uses (each receiver one whole set, neighbours different ones).
Two depths: segs 1 (a gathered ray is shaded where it lands) and segs 0 (the scene's depth).
 1. the fused kernel, rt_scene_gather_device, rgb out: rt_stats.kernel_ms;
 2. its parts on the same receivers, per sample: rt_ambient_segments_device (rays into device memory; a host clock around the launch and
    a synchronise, the entry point reports no stats) and rt_scene_trace_rays_soft_device with levels 0, one sample, light_radius 0 and
    pix_base = s n (rgb out; rt_stats.kernel_ms) - and, reported beside them, for samples 1..15 one addition of the sample's colours
    into an accumulator (the library's accumulate kernel, device events).  No division: less than the fused kernel does;
 3. the host form rt_gather_view end to end (rgb out): a host clock around rt_host.gather_view; and, ONCE per scene (it takes tens of
    seconds), the composed host path: rt_host.view_hit_records, then per sample rt_host.ambient_segments,
    rt_host.trace_rays_soft(method="recursive", levels 0) and one numpy addition, then the division.
Per configuration one warm-up pass, then `reps` passes in which the variants alternate; median, min and max.
   python3 profiles/gather_timing.py [reps] [out.json] [kernel]      ("kernel": parts 1 and 2 only)"""
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
from ambient import COPIES, turned_copies

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 5
kernel_only = len(sys.argv) > 3 and sys.argv[3] == "kernel"
w, h, n_samples = 3840, 2160, 16
n = w * h
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


def add_ms(d_acc, d_c):
    """acc += c over 3 n doubles on the NULL stream, by device events"""
    assert hip.hipEventRecord(ev[0], None) == 0
    assert lib.rt_launch_view_accumulate(d_acc, d_c, n, None) == 0
    assert hip.hipEventRecord(ev[1], None) == 0
    assert hip.hipEventSynchronize(ev[1]) == 0
    ms = C.c_float()
    assert hip.hipEventElapsedTime(C.byref(ms), ev[0], ev[1]) == 0
    return ms.value


TABLES = (("same_16_stride_0", lambda: rt_host.ambient_dirs(16, lib), 0), ("sets_61x16_stride_16", lambda: turned_copies(rt_host.ambient_dirs(16, lib), COPIES), 16))
d_hits, d_rays = alloc(n * 80), alloc(n * 48)
d_rgb, d_c, d_acc = alloc(n * 24), alloc(n * 24), alloc(n * 24)
out = {"w": w, "h": h, "receivers": n, "n_samples": n_samples, "reps": reps, "library": os.path.basename(rt_host.LIB_PATH), "scenes": {}}
for name in ("default14", "h8"):
    scene = rt_host.load_scene(name)
    cam = scene["camera"]
    v = rt_host.view(rt_host.RT_VIEW_PINHOLE, cam["origin"], cam["axisX"], cam["axisY"], cam["axisZ"], scene["fovDeg"])
    r = rt_host.Renderer(scene, 0, lib)
    r.trace_view(v, w, h, 0, 0, d_hits, d_rays, 48 * n, want_stats=True)           # the receivers (d_rays is the workspace here)
    res = {"depth": scene["segs"]}
    for label, table, stride in TABLES:
        dirs = table()
        n_dirs = len(dirs)
        d_dirs = upload(dirs)
        for segs in (1, 0):

            def fused():
                return r.gather(n, d_hits, d_dirs, n_dirs, n_samples, d_rgb, 0, stride=stride, segs=segs, want_stats=True).kernel_ms

            def parts():
                p = {"segments": 0.0, "trace": 0.0, "add": 0.0}
                for s in range(n_samples):
                    assert hip.hipDeviceSynchronize() == 0
                    t0 = time.perf_counter()
                    r.ambient_segments(n, d_hits, d_dirs, n_dirs, s, d_rays, 0, n_samples=n_samples, stride=stride)
                    assert hip.hipDeviceSynchronize() == 0
                    p["segments"] += (time.perf_counter() - t0) * 1e3
                    p["trace"] += r.trace_rays_soft(n, d_rays, d_acc if s == 0 else d_c, 0, 0, 1, 1, 0.0, levels=0, segs=segs, pix_base=s * n,
                                                    want_stats=True).kernel_ms
                    if s:
                        p["add"] += add_ms(d_acc, d_c)
                return p

            fused(), parts()
            ms = {"fused": [], "parts": [], "segments": [], "trace": [], "add": []}
            for _ in range(reps):
                ms["fused"].append(fused())
                p = parts()
                ms["parts"].append(p["segments"] + p["trace"])
                for k in p:
                    ms[k].append(p[k])
            key = "%s_segs_%d" % (label, segs)
            res[key] = {k: spread(a) for k, a in ms.items()}
            res[key]["parts_over_fused"] = round(statistics.median(ms["parts"]) / statistics.median(ms["fused"]), 3)
            # the two routes agree: the accumulator over n_samples is the fused rgb
            acc, rgb = np.empty(3 * n), np.empty(3 * n)
            assert lib.rt_copy_to_host(0, acc.ctypes.data, d_acc, n * 24) == 0
            fused()
            assert lib.rt_copy_to_host(0, rgb.ctypes.data, d_rgb, n * 24) == 0
            res[key]["same_bytes"] = bool((acc / float(n_samples)).tobytes() == rgb.tobytes())
            print(name, key, json.dumps(res[key]), flush=True)
        lib.rt_free_device(0, d_dirs)
    r.close()
    if not kernel_only:
        # 3. the host forms, end to end: 61 sets of 16 with stride 16, the scene's depth
        dirs = turned_copies(rt_host.ambient_dirs(16, lib), COPIES)
        rt_host.gather_view(scene, v, w, h, n_samples, dirs=dirs, stride=16, lib=lib)
        host = []
        for _ in range(reps):
            t0 = time.perf_counter()
            got = rt_host.gather_view(scene, v, w, h, n_samples, dirs=dirs, stride=16, want=("rgb",), lib=lib)
            host.append((time.perf_counter() - t0) * 1e3)
        res["host_form_gather_view_rgb"] = spread(host)
        print(name, "host form", json.dumps(res["host_form_gather_view_rgb"]), flush=True)
        t0 = time.perf_counter()
        hits = rt_host.view_hit_records(scene, v, w, h, lib=lib)
        t_hits = (time.perf_counter() - t0) * 1e3
        acc = None
        for s in range(n_samples):
            rays, _ = rt_host.ambient_segments(hits, s, n_samples, dirs=dirs, stride=16, lib=lib)
            c = rt_host.trace_rays_soft(scene, rays, 1, 0.0, levels=0, want=("rgb",), method="recursive", lib=lib)["rgb"]
            acc = c if acc is None else acc + c
            print(name, "composed host path, sample", s, round((time.perf_counter() - t0) * 1e3), "ms", flush=True)
        with np.errstate(invalid="ignore"):
            mean = acc / float(n_samples)
        res["composed_host_path_once_ms"] = {"total": round((time.perf_counter() - t0) * 1e3, 1), "view_hit_records": round(t_hits, 1)}
        # (the stars sampler's pix differs - the composed path has no pix_base - but neither scene has stars)
        res["composed_same_bytes"] = bool(mean.tobytes() == got["rgb"].tobytes())
        print(name, "composed host path", json.dumps(res["composed_host_path_once_ms"]), res["composed_same_bytes"], flush=True)
    out["scenes"][name] = res

if len(sys.argv) > 2:
    with open(sys.argv[2], "w") as f:
        json.dump(out, f, indent=1)
