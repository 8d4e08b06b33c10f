"""Soak of the uniform-material path (rt_kernel.hip: trace_pixel, UNI) on the random scenes of tests/soak_gpu_parity.py.

That soak compares the FIRST frame of every fresh upload, and the first frame from a camera runs the four-wave form of the product
kernel, which never takes the path.  Here every scene is rendered twice by the test library: the second frame runs one-wave workgroups
and is held to the C restatement (pixels beyond 1 LSB must be 0) and to the first frame's bytes (the general path's); the waves that
took the path are counted (rt_test_uniform_waves), per scene, so that the report says how much of it was the path's work.

    python tests/soak_gpu_uniform_blocks.py --seeds 2000 --first 900000 [--many-spheres] [--out report.json]
"""
import argparse
import ctypes as C
import json
import os
import signal
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "html5-canvas-raytracer_amd"))
sys.path.insert(0, HERE)
import oracle_util as ou  # noqa: E402
import rt_host  # noqa: E402
from soak_gpu_parity import draw_scene  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seeds", type=int, default=300)
    ap.add_argument("--first", type=int, default=900000)
    ap.add_argument("--many-spheres", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    lib = rt_host.load_library(rt_host.TEST_LIB_PATH)
    assert lib.rt_init(1) == 0, lib.rt_last_error()
    lib.rt_test_uniform_waves.restype = C.c_int
    lib.rt_test_uniform_waves.argtypes = [C.c_int, C.POINTER(C.c_ulonglong)]
    stop = {"now": False}
    signal.signal(signal.SIGTERM, lambda *_: stop.__setitem__("now", True))
    t0 = time.time()
    T = {"scenes": 0, "pixels": 0, "channels": 0, "off_by_one": 0, "flipped_pixels": 0, "worst": 0, "scenes_with_flips": [],
         "second_frames_that_differ_from_the_first": 0, "uniform_waves": 0, "scenes_with_uniform_waves": 0, "supersample_2_scenes_with_uniform_waves": 0,
         "exact_samples_first": 0, "exact_samples_second": 0}
    n = C.c_ulonglong()
    for seed in range(args.first, args.first + args.seeds):
        if stop["now"]:
            break
        scene, w, h = draw_scene(seed, False, args.many_spheres)
        blob = rt_host.flatten_scene(scene)
        want = np.frombuffer(ou.c_oracle_render(blob, w, h), dtype=np.uint8).reshape(w * h, 4).astype(np.int16)
        r = rt_host.Renderer(blob, 0, lib)
        d = lib.rt_alloc_device(0, w * h * 4)
        try:
            frames = []
            for k in range(2):
                assert lib.rt_test_uniform_waves(0, C.byref(n)) == 0
                st = r.render_tiles(w, h, d, None, want_stats=True)
                assert lib.rt_test_uniform_waves(0, C.byref(n)) == 0
                host = C.create_string_buffer(w * h * 4)
                assert lib.rt_copy_to_host(0, host, d, w * h * 4) == 0
                frames.append(host.raw)
                T["exact_samples_first" if k == 0 else "exact_samples_second"] += int(st.exact_samples)
            took = n.value                               # (the second frame's)
        finally:
            lib.rt_free_device(0, d)
            r.close()
        T["scenes"] += 1
        T["pixels"] += w * h
        T["uniform_waves"] += took
        T["scenes_with_uniform_waves"] += 1 if took else 0
        T["supersample_2_scenes_with_uniform_waves"] += 1 if (took and scene["supersample"] == 2) else 0
        T["second_frames_that_differ_from_the_first"] += 1 if frames[1] != frames[0] else 0
        diff = np.abs(np.frombuffer(frames[1], dtype=np.uint8).reshape(w * h, 4).astype(np.int16) - want)
        T["channels"] += diff.size
        T["off_by_one"] += int((diff == 1).sum())
        flips = int((diff.max(axis=1) > 1).sum())
        T["flipped_pixels"] += flips
        T["worst"] = max(T["worst"], int(diff.max()))
        if flips:
            T["scenes_with_flips"].append({"seed": seed, "w": w, "h": h, "pixels": flips, "segs": scene["segs"], "ss": scene["supersample"]})
        if T["scenes"] % 50 == 0:
            print("seed %d: %d pixels, %.0f s; flipped %d, second != first %d, uniform waves %d" % (
                seed, T["pixels"], time.time() - t0, T["flipped_pixels"], T["second_frames_that_differ_from_the_first"], T["uniform_waves"]), flush=True)
    out = dict(T, seeds=[args.first, args.first + T["scenes"] - 1], many_spheres=args.many_spheres, seconds=round(time.time() - t0, 1),
               interrupted=T["scenes"] < args.seeds, scenes_with_flips=T["scenes_with_flips"][:40])
    text = json.dumps(out, indent=1)
    if args.out:
        open(args.out, "w").write(text)
    print(text)


if __name__ == "__main__":
    main()
