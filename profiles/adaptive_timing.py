#!/usr/bin/env python3
"""Adaptive supersampling (rt_render_adaptive_device) beside the frames it sits between: the supersample-1 frame alone and the full
supersample-k frame through the existing path, for H8 and default14.
  time     3840x2160, k = 2 and 4, T = 16 and 32 (and T = 256: the base frame plus the criterion, nothing refined): the refined share,
           and per frame two figures - `stats_ms`, the median of rt_stats.kernel_ms (HIP events around one call's launches, the call
           waited for), and `stream_ms`, HIP events around `reps` calls issued back to back on one stream without a host wait between
           them, divided by reps (the full supersample-3/4 path waits and allocates inside every call: that is part of what it costs)
  picture  1920x1080, the same settings: the adaptive frame against the full supersample-k frame - the share of pixels that differ by
           more than 1 LSB in some channel, and the largest difference
   python3 profiles/adaptive_timing.py [reps] [out.json]"""
import ctypes as C
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "html5-canvas-raytracer_amd"))
import rt_host

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 30
WARM = 10
lib = rt_host.load_library()
assert lib.rt_init(1) == 0, lib.rt_last_error()
hip = C.CDLL("libamdhip64.so")


def ok(e):
    assert e == 0, "HIP error %d" % e


stream, ev0, ev1 = C.c_void_p(), C.c_void_p(), C.c_void_p()
ok(hip.hipStreamCreate(C.byref(stream)))
ok(hip.hipEventCreate(C.byref(ev0)))
ok(hip.hipEventCreate(C.byref(ev1)))


def timed(call):
    """{stats_ms, stream_ms} of call(want_stats) on `stream`"""
    for _ in range(WARM):
        call(False)
    ok(hip.hipStreamSynchronize(stream))
    ms = [call(True).kernel_ms for _ in range(reps)]
    ok(hip.hipEventRecord(ev0, stream))
    for _ in range(reps):
        call(False)
    ok(hip.hipEventRecord(ev1, stream))
    ok(hip.hipEventSynchronize(ev1))
    t = C.c_float()
    ok(hip.hipEventElapsedTime(C.byref(t), ev0, ev1))
    return {"stats_ms": round(statistics.median(ms), 4), "stats_min_ms": round(min(ms), 4), "stream_ms": round(t.value / reps, 4)}


def host(ptr, n, dtype=np.uint8):
    a = np.empty(n, np.uint8)
    ok(hip.hipStreamSynchronize(stream))
    assert lib.rt_copy_to_host(0, a.ctypes.data, ptr, n) == 0, lib.rt_last_error()
    return a.view(dtype)


out = {"reps": reps, "warmup": WARM, "time": [], "picture": []}
for name in ("h8", "default14"):
    scene = rt_host.load_scene(name)
    assert scene.get("supersample", 1) == 1
    base_r = rt_host.Renderer(scene, 0, lib)
    full_r = {k: rt_host.Renderer(dict(scene, supersample=k), 0, lib) for k in (2, 4)}
    for what, (w, h) in (("time", (3840, 2160)), ("picture", (1920, 1080))):
        n = w * h
        wb = rt_host.adaptive_work_bytes(w, h, lib)
        frame, full, work = lib.rt_alloc_device(0, n * 4), lib.rt_alloc_device(0, n * 4), lib.rt_alloc_device(0, wb)
        assert frame and full and work, lib.rt_last_error()
        if what == "time":
            row = {"scene": name, "w": w, "h": h, "base": timed(lambda s: base_r.render_tiles(w, h, frame, stream=stream.value, want_stats=s))}
            for k in (2, 4):
                row["full_k%d" % k] = timed(lambda s: full_r[k].render_tiles(w, h, full, stream=stream.value, want_stats=s))
            out["time"].append(row)
            print(json.dumps(row), flush=True)
        for k in (2, 4):
            if what == "picture":
                full_r[k].render_tiles(w, h, full, stream=stream.value)
                want = host(full, n * 4).reshape(h, w, 4).astype(np.int16)
            for t in ((16, 32, 256) if what == "time" else (16, 32)):
                call = lambda s: base_r.render_adaptive(w, h, frame, k, t, work, wb, stream=stream.value, want_stats=s)
                row = {"scene": name, "w": w, "h": h, "k": k, "threshold": t}
                if what == "time":
                    row.update(timed(call))
                else:
                    call(False)
                    d = np.abs(host(frame, n * 4).reshape(h, w, 4).astype(np.int16) - want).max(axis=2)
                    row.update({"pixels_off_by_more_than_1_lsb": round(float((d > 1).mean()), 6), "largest_difference": int(d.max())})
                row["refined_share"] = round(int(host(work, 4, np.uint32)[0]) / n, 5)
                out[what].append(row)
                print(json.dumps(row), flush=True)
        for p in (frame, full, work):
            lib.rt_free_device(0, p)
    base_r.close()
    for r in full_r.values():
        r.close()
if len(sys.argv) > 2:
    with open(sys.argv[2], "w") as f:
        json.dump(out, f, indent=1)
