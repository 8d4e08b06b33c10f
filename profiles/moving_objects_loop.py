#!/usr/bin/env python3
"""The moving-objects loop (for rocprofv3 --kernel-trace --stats): one sphere orbits, per step rt_scene_set_objects + render; then the
same scene with a still picture and with the camera loop of moving_camera_loop.py, for comparison.
   python3 profiles/moving_objects_loop.py [scene] [w] [h] [steps]"""
import math, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "html5-canvas-raytracer_amd")); sys.path.insert(0, ROOT)
import rt_host
import bench
scene_name = sys.argv[1] if len(sys.argv) > 1 else "h8"
w, h = (int(sys.argv[2]), int(sys.argv[3])) if len(sys.argv) > 3 else (3840, 2160)
steps = int(sys.argv[4]) if len(sys.argv) > 4 else 256
scene = rt_host.load_scene(scene_name)
lib = rt_host.load_library()
assert lib.rt_init(1) == 0
r = rt_host.Renderer(scene, 0, lib)
d = lib.rt_alloc_device(0, w * h * 4)
i = next(i for i, o in enumerate(scene["objects"]) if o["r2"] < 1e4)          # the first sphere that is neither skybox nor ground
o = scene["objects"][i]
c0, rad = list(o["origin"]), 0.5 * math.sqrt(o["r2"]) + 0.2
recs = []
for k in range(64):
    a = 2 * math.pi * k / 64
    o["origin"] = [c0[0] + rad * math.cos(a), c0[1], c0[2] + rad * math.sin(a)]
    recs.append(rt_host.sphere_records([o]))
cams = [bench.moving_camera(scene, k, 64) for k in range(64)]
whole = rt_host.RtTiles(h, 0, 1, 1)


def loop(step):
    for k in range(8):
        step(k); r.render_tiles(w, h, d, whole)
    r.render_tiles(w, h, d, whole, want_stats=True)
    t0 = time.perf_counter()
    for k in range(steps):
        step(k); r.render_tiles(w, h, d, whole)
    r.render_tiles(w, h, d, whole, want_stats=True)
    return (time.perf_counter() - t0) / steps


for what, step in (("still", lambda k: None), ("objects", lambda k: r.set_objects(recs[k % 64], i)), ("camera", lambda k: r.set_camera(cams[k % 64]))):
    dt = loop(step)
    print("%s %dx%d %-8s %.4f ms per step (%d steps), %.1f Gpixel/s" % (scene_name, w, h, what, dt * 1e3, steps, w * h / dt / 1e9))
lib.rt_free_device(0, d); r.close()
