#!/usr/bin/env python3
"""Gathered light for short receiver lists, by both mappings (docs/EVIDENCE.md, "Probes"): rt_scene_gather_device (one lane per receiver)
against rt_scene_gather_probes_device (one workgroup per receiver, its samples on lanes), on default14 at the scene's depth.  The
receivers are n hit records spread evenly over the 192 x 108 pinhole view of the scene's camera (repeated where n is larger), n in
1 .. 16384 and, to find where the receivers mapping overtakes, 65536 .. 1048576; the table is the sphere spiral
(rt_lighting_sphere_offsets) of n_samples entries with stride 0, n_samples 64, 256 and 1024; rgb out.  Per (n_samples, n) one
warm-up pass, then `reps` passes in which the two mappings alternate; median, min and max of rt_stats.kernel_ms (device events around the
launch), and whether both gave the same bytes.  With weights: the samples mapping again with the nine spherical-harmonics weights and
coef as its only output.
   python3 profiles/probe_timing.py [reps] [out.json]"""
import ctypes as C
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "html5-canvas-raytracer_amd"))
import numpy as np
import rt_host

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 5
W, H = 192, 108
COUNTS = (1, 16, 64, 256, 1024, 4096, 16384, 65536, 262144, 1048576)
SAMPLES = (64, 256, 1024)
lib = rt_host.load_library()
assert lib.rt_init(1) == 0
hip = C.CDLL("libamdhip64.so")


def upload(a):
    a = np.ascontiguousarray(a)
    p = lib.rt_alloc_device(0, a.nbytes)
    assert p, lib.rt_last_error()
    assert hip.hipMemcpy(C.c_void_p(p), a.ctypes.data_as(C.c_void_p), C.c_size_t(a.nbytes), 1) == 0
    return p


def spread(ms):
    return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4)}


scene = rt_host.load_scene("default14")
cam = scene["camera"]
v = rt_host.view(rt_host.RT_VIEW_PINHOLE, cam["origin"], cam["axisX"], cam["axisY"], cam["axisZ"], scene["fovDeg"])
every = rt_host.view_hit_records(scene, v, W, H, lib=lib)
r = rt_host.Renderer(scene, 0, lib)
n_max = max(COUNTS)
d_rgb, d_rgb2, d_coef = (lib.rt_alloc_device(0, q) for q in (n_max * 24, n_max * 24, n_max * 24 * 9))
out = {"scene": "default14", "depth": scene["segs"], "view": [W, H], "reps": reps, "library": os.path.basename(rt_host.LIB_PATH), "table": "sphere spiral, stride 0",
       "rows": []}
for n_samples in SAMPLES:
    dirs = rt_host.lighting_offsets(n_samples, lib)
    d_dirs, d_w = upload(dirs), upload(rt_host.sh9_weights(dirs, lib=lib))
    for n in COUNTS:
        hits = every[(np.arange(n, dtype=np.int64) * len(every)) // n]
        d_hits = upload(hits)

        def receivers():
            return r.gather(n, d_hits, d_dirs, n_samples, n_samples, d_rgb, 0, stride=0, want_stats=True).kernel_ms

        def samples():
            return r.gather_probes(n, d_hits, d_dirs, n_samples, n_samples, d_rgb2, 0, stride=0, want_stats=True).kernel_ms

        def weighted():
            return r.gather_probes(n, d_hits, d_dirs, n_samples, n_samples, 0, 0, coef_ptr=d_coef, weights_ptr=d_w, n_weights=9, stride=0, want_stats=True).kernel_ms

        receivers(), samples(), weighted()
        ms = {"receivers": [], "samples": [], "samples_sh9": []}
        for _ in range(reps):
            ms["receivers"].append(receivers())
            ms["samples"].append(samples())
            ms["samples_sh9"].append(weighted())
        a, b = np.empty(3 * n), np.empty(3 * n)
        assert lib.rt_copy_to_host(0, a.ctypes.data, d_rgb, n * 24) == 0 and lib.rt_copy_to_host(0, b.ctypes.data, d_rgb2, n * 24) == 0
        row = {"n_samples": n_samples, "n": n, "scanned": int((hits["object"] >= 0).sum())}
        row.update({k: spread(q) for k, q in ms.items()})
        row["receivers_over_samples"] = round(statistics.median(ms["receivers"]) / statistics.median(ms["samples"]), 3)
        row["same_bytes"] = bool(a.tobytes() == b.tobytes())
        out["rows"].append(row)
        print(json.dumps(row), flush=True)
        lib.rt_free_device(0, d_hits)
    lib.rt_free_device(0, d_dirs)
    lib.rt_free_device(0, d_w)
r.close()

if len(sys.argv) > 2:
    with open(sys.argv[2], "w") as f:
        json.dump(out, f, indent=1)
