#!/usr/bin/env python3
"""Kernel time of rt_render_hits_device (HIP events around the one launch, rt_stats.kernel_ms) for H8 at 3840x2160: all three buffers
and the id buffer alone, beside the colour frame of the same scene and size.
   python3 profiles/hits_timing.py [reps] [out.json]"""
import json, os, statistics, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "html5-canvas-raytracer_amd"))
import rt_host
reps = int(sys.argv[1]) if len(sys.argv) > 1 else 200
w, h = 3840, 2160
lib = rt_host.load_library()
assert lib.rt_init(1) == 0
r = rt_host.Renderer(rt_host.load_scene("h8"), 0, lib)
n = w * h
bufs = {"id": lib.rt_alloc_device(0, n * 4), "depth": lib.rt_alloc_device(0, n * 8), "normal": lib.rt_alloc_device(0, n * 12)}
frame = lib.rt_alloc_device(0, n * 4)
cases = {"id+depth+normal": (bufs["id"], bufs["depth"], bufs["normal"]), "id only": (bufs["id"], 0, 0)}
out = {"scene": "h8", "w": w, "h": h, "reps": reps}
for name, ptrs in cases.items():
    for _ in range(10):
        r.render_hits(w, h, *ptrs)
    ms = [r.render_hits(w, h, *ptrs, want_stats=True).kernel_ms for _ in range(reps)]
    stored = n * (4 + (8 if ptrs[1] else 0) + (12 if ptrs[2] else 0))
    out[name] = {"median_ms": statistics.median(ms), "min_ms": min(ms), "stored_bytes": stored,
                 "store_TBps_at_median": stored / (statistics.median(ms) * 1e-3) / 1e12}
for _ in range(10):
    r.render_tiles(w, h, frame)
ms = [r.render_tiles(w, h, frame, want_stats=True).kernel_ms for _ in range(reps)]
out["colour frame"] = {"median_ms": statistics.median(ms), "min_ms": min(ms)}
print(json.dumps(out, indent=1))
if len(sys.argv) > 2:
    with open(sys.argv[2], "w") as f:
        json.dump(out, f, indent=1)
for p in list(bufs.values()) + [frame]:
    lib.rt_free_device(0, p)
r.close()
