#!/usr/bin/env python3
"""Small-frame call rate, where the host cost of a launch shows: h8 at a few hundred pixels per side, N frames back to back with stats
off.  Prints, per frame size, the microseconds per call of the enqueue loop alone and of the loop with the queue drained.
  RT_HIP_LIB=<library> python3 profiles/call_rate.py [N]      (A/B: run the libraries alternately, several times each)"""
import ctypes as C
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "html5-canvas-raytracer_amd"))
import rt_host

N = int(sys.argv[1]) if len(sys.argv) > 1 else 20000
lib = rt_host.load_library()
assert lib.rt_init(1) == 0, lib.rt_last_error()
r = rt_host.Renderer(rt_host.flatten_scene(rt_host.load_scene("h8")), 0, lib)
out = []
for w, h in ((256, 256), (255, 255), (64, 64)):        # (255: odd both ways, rt_retrace runs behind every frame)
    d = lib.rt_alloc_device(0, w * h * 4)
    host = C.create_string_buffer(4)
    whole = rt_host.RtTiles(h, 0, 1, 1)
    for _ in range(300):
        r.render_tiles(w, h, d, whole)
    lib.rt_copy_to_host(0, host, d, 4)
    t0 = time.perf_counter()
    for _ in range(N):
        r.render_tiles(w, h, d, whole)
    t1 = time.perf_counter()
    lib.rt_copy_to_host(0, host, d, 4)
    t2 = time.perf_counter()
    out.append("%dx%d enqueue %.2f us/call, drained %.2f us/call" % (w, h, (t1 - t0) / N * 1e6, (t2 - t0) / N * 1e6))
    lib.rt_free_device(0, d)
r.close()
print(" | ".join(out), flush=True)
