#!/usr/bin/env python3
"""The moving-lights loop: one light orbits, per frame rt_scene_set_lights + render - beside the same blob sequence uploaded afresh
per frame by a library built from the parent commit (what rt_render did for a moved light before rt_scene_set_lights), and beside the
object move of moving_objects_loop.py.  Steady state, one stream, no host wait inside loops (a) and (c); a frame's time is the
interval between the device events recorded behind consecutive frames, and a run's figure the median over its frames.
   python3 profiles/moving_lights_loop.py [out.json] [parent librt_hip.so] [w] [h] [frames] [repeats]     the comparison: per scene
        and repeat one fresh process per loop, the loops alternating; prints the medians and their spread
   python3 profiles/moving_lights_loop.py --one a|b|c scene w h frames                                     one loop (RT_HIP_LIB selects
        the library; under rocprofv3 --kernel-trace --stats this form shows a light move's kernels)
     a  set_lights of one light on an orbit, then render_tiles
     b  the same blobs, each through rt_scene_upload, render_tiles, rt_scene_free
     c  set_objects of one sphere on an orbit, then render_tiles"""
import ctypes as C
import json
import math
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "html5-canvas-raytracer_amd"))
SCENES = ("h8", "default14", "lcg64")
WARMUP = 16


def one(mode, scene_name, w, h, frames):
    import rt_host
    scene = rt_host.load_scene(scene_name)
    lib = rt_host.load_library()
    assert lib.rt_init(1) == 0
    hip = C.CDLL("libamdhip64.so")
    stream = C.c_void_p()
    assert hip.hipStreamCreate(C.byref(stream)) == 0
    events = [C.c_void_p() for _ in range(frames + 1)]
    for e in events:
        assert hip.hipEventCreate(C.byref(e)) == 0
    d = lib.rt_alloc_device(0, w * h * 4)
    whole = rt_host.RtTiles(h, 0, 1, 1)
    l0 = list(scene["lights"][0])
    orbit = [[l0[0] + 3.0 * math.cos(2 * math.pi * k / 64), l0[1], l0[2] + 3.0 * math.sin(2 * math.pi * k / 64)] for k in range(64)]
    r = None
    if mode == "b":
        blobs = [rt_host.flatten_scene(dict(scene, lights=[p] + scene["lights"][1:])) for p in orbit]

        def frame(k):
            x = rt_host.Renderer(blobs[k % 64], 0, lib)
            x.render_tiles(w, h, d, whole, stream=stream.value)
            assert hip.hipEventRecord(events[max(k - WARMUP + 1, 0)], stream) == 0
            x.close()
    else:
        r = rt_host.Renderer(scene, 0, lib)
        i = next(i for i, o in enumerate(scene["objects"]) if o["r2"] < 1e4)      # the first sphere that is neither skybox nor ground
        o = dict(scene["objects"][i])
        c0, rad = list(o["origin"]), 0.5 * math.sqrt(o["r2"]) + 0.2
        recs = [rt_host.sphere_records([dict(o, origin=[c0[0] + rad * math.cos(2 * math.pi * k / 64), c0[1], c0[2] + rad * math.sin(2 * math.pi * k / 64)])]) for k in range(64)]

        def frame(k):
            if mode == "a":
                r.set_lights([orbit[k % 64]])
            else:
                r.set_objects(recs[k % 64], i)
            r.render_tiles(w, h, d, whole, stream=stream.value)
            assert hip.hipEventRecord(events[max(k - WARMUP + 1, 0)], stream) == 0
    for k in range(WARMUP + frames):              # (event 0 is recorded again by every warm-up frame: its last record opens the window)
        frame(k)
    assert hip.hipStreamSynchronize(stream) == 0
    ms = []
    for k in range(frames):
        t = C.c_float()
        assert hip.hipEventElapsedTime(C.byref(t), events[k], events[k + 1]) == 0
        ms.append(t.value)
    if r is not None:
        r.close()
    lib.rt_free_device(0, d)
    print(json.dumps({"mode": mode, "scene": scene_name, "w": w, "h": h, "frames": frames, "median_ms": statistics.median(ms),
                      "mean_ms": sum(ms) / len(ms), "p10_ms": sorted(ms)[len(ms) // 10], "p90_ms": sorted(ms)[(9 * len(ms)) // 10]}))


def compare(out, parent_lib, w, h, frames, repeats):
    rows = []
    for scene in SCENES:
        for rep in range(repeats):
            for mode in ("a", "b", "c"):
                env = dict(os.environ)
                if mode == "b":
                    env["RT_HIP_LIB"], env["RT_HIP_LIB_OLDER"] = parent_lib, "1"
                p = subprocess.run([sys.executable, os.path.abspath(__file__), "--one", mode, scene, str(w), str(h), str(frames)], env=env,
                                   stdout=subprocess.PIPE, text=True, timeout=300)
                if p.returncode != 0:               # (a loop that failed ends the comparison: nothing more is started on the GPU)
                    sys.exit("loop %s of %s failed (exit status %d)" % (mode, scene, p.returncode))
                row = json.loads(p.stdout.strip().splitlines()[-1])
                row["repeat"] = rep
                rows.append(row)
                print(json.dumps(row), flush=True)
    summary = {}
    for scene in SCENES:
        med = {m: [x["median_ms"] for x in rows if x["scene"] == scene and x["mode"] == m] for m in "abc"}
        summary[scene] = {m: {"medians_ms": med[m], "median_ms": statistics.median(med[m]), "spread_ms": max(med[m]) - min(med[m])} for m in "abc"}
        s = summary[scene]
        print("%-10s %dx%d  (a) set_lights %.4f ms   (b) parent, upload per frame %.4f ms (spread %.4f)   (c) set_objects %.4f ms (spread %.4f)"
              % (scene, w, h, s["a"]["median_ms"], s["b"]["median_ms"], s["b"]["spread_ms"], s["c"]["median_ms"], s["c"]["spread_ms"]))
    if out:
        with open(out, "w") as f:
            json.dump({"w": w, "h": h, "frames": frames, "repeats": repeats, "runs": rows, "summary": summary}, f, indent=1)


if __name__ == "__main__":
    a = sys.argv[1:]
    if a and a[0] == "--one":
        one(a[1], a[2], int(a[3]), int(a[4]), int(a[5]))
    else:
        compare(a[0] if a else None, a[1] if len(a) > 1 else os.path.join(ROOT, "build", "ab", "librt_hip_parent.so"),
                int(a[2]) if len(a) > 2 else 3840, int(a[3]) if len(a) > 3 else 2160, int(a[4]) if len(a) > 4 else 256, int(a[5]) if len(a) > 5 else 3)
