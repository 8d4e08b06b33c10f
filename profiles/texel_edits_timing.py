#!/usr/bin/env python3
"""What a texel edit costs (docs/EVIDENCE.md, "Texel edits").  Three measurements, each a fresh process per run so that nothing warm
is shared, the two sides of a comparison alternating:
   python3 profiles/texel_edits_timing.py [out.json] [parent librt_hip.so] [repeats]
     blit   per iteration of `render probe 256x128 -> set_texels_device (the earth's texture) -> render 3840x2160` of default14 on ONE
            stream, beside the same loop without the edit; windows of ITER iterations between two device events, the loops alternating
            inside one process
     host   rt_render at 3840x2160 of default14 with the 256x128 earth texture changed in every call (host clock around the call, which
            returns with the frame in pinned memory), with this library and with one built from the parent commit, where the same call
            uploads; beside it the same call with nothing changed
     big    a whole 16384x16384 texture (1 GiB) through the host form (host clock from the call to the end of the stream) and the
            device form (device events), GB/s
   python3 profiles/texel_edits_timing.py --one blit|host|big ...      one run (RT_HIP_LIB selects the library)"""
import ctypes as C
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "html5-canvas-raytracer_amd"))
W, H, ITER, WINDOWS, WARMUP = 3840, 2160, 200, 10, 50


def earth_variants(scene, n):
    import numpy as np
    t = np.frombuffer(scene["textures"][0]["texels"], np.uint8).reshape(128, 256, 4)
    return [np.roll(t, 8 * (k + 1), axis=1).tobytes() for k in range(n)]               # the picture scrolls


def blit():
    import rt_host
    scene = rt_host.load_scene("default14")
    assert (scene["textures"][0]["width"], scene["textures"][0]["height"]) == (256, 128)
    lib = rt_host.load_library()
    assert lib.rt_init(1) == 0
    hip = C.CDLL("libamdhip64.so")
    stream, e0, e1 = C.c_void_p(), C.c_void_p(), C.c_void_p()
    assert hip.hipStreamCreate(C.byref(stream)) == 0 and hip.hipEventCreate(C.byref(e0)) == 0 and hip.hipEventCreate(C.byref(e1)) == 0
    d_probe, d_frame = lib.rt_alloc_device(0, 256 * 128 * 4), lib.rt_alloc_device(0, W * H * 4)
    r = rt_host.Renderer(scene, 0, lib)
    probe, frame = rt_host.RtTiles(128, 0, 1, 1), rt_host.RtTiles(H, 0, 1, 1)

    def window(edit, n):
        assert hip.hipEventRecord(e0, stream) == 0
        for _ in range(n):
            r.render_tiles(256, 128, d_probe, probe, stream=stream.value)
            if edit:
                r.set_texels_device(0, d_probe, 0, 0, 256, 128, stream=stream.value)
            r.render_tiles(W, H, d_frame, frame, stream=stream.value)
        assert hip.hipEventRecord(e1, stream) == 0 and hip.hipStreamSynchronize(stream) == 0
        t = C.c_float()
        assert hip.hipEventElapsedTime(C.byref(t), e0, e1) == 0
        return t.value / n

    window(True, WARMUP), window(False, WARMUP)
    rows = {"with_edit_ms": [], "without_ms": []}
    for _ in range(WINDOWS):
        rows["with_edit_ms"].append(window(True, ITER))
        rows["without_ms"].append(window(False, ITER))
    r.close()
    diff = [a - b for a, b in zip(rows["with_edit_ms"], rows["without_ms"])]
    print(json.dumps({"mode": "blit", "iterations_per_window": ITER, **rows, "median_with_ms": statistics.median(rows["with_edit_ms"]),
                      "median_without_ms": statistics.median(rows["without_ms"]), "median_difference_us": 1e3 * statistics.median(diff),
                      "difference_us_min_max": [1e3 * min(diff), 1e3 * max(diff)]}))


def host(change):
    import rt_host
    scene = rt_host.load_scene("default14")
    lib = rt_host.load_library()
    assert lib.rt_init(1) == 0
    blobs = [rt_host.flatten_scene(dict(scene, textures=[dict(scene["textures"][0], texels=t)] + scene["textures"][1:])) for t in earth_variants(scene, 8)]
    bufs = [C.create_string_buffer(b, len(b)) for b in blobs]
    p = lib.rt_alloc_pinned(W * H * 4)
    assert p

    def call(k):
        b = bufs[k % 8 if change else 0]
        t0 = time.perf_counter()
        assert lib.rt_render(b, len(b), W, H, C.c_void_p(p), 0, None) == 0, lib.rt_last_error()
        return 1e3 * (time.perf_counter() - t0)

    for k in range(WARMUP):
        call(k)
    ms = sorted(call(k) for k in range(ITER))
    print(json.dumps({"mode": "host", "texture_changes": bool(change), "calls": ITER, "median_ms": statistics.median(ms), "p10_ms": ms[len(ms) // 10],
                      "p90_ms": ms[(9 * len(ms)) // 10]}))


def big():
    import numpy as np
    import rt_host
    side, n = 16384, 16384 * 16384 * 4
    scene = rt_host.load_scene("default14")
    scene["textures"][0] = {"width": side, "height": side, "texels": bytes(n)}
    lib = rt_host.load_library()
    assert lib.rt_init(1) == 0
    hip = C.CDLL("libamdhip64.so")
    stream, e0, e1 = C.c_void_p(), C.c_void_p(), C.c_void_p()
    assert hip.hipStreamCreate(C.byref(stream)) == 0 and hip.hipEventCreate(C.byref(e0)) == 0 and hip.hipEventCreate(C.byref(e1)) == 0
    r = rt_host.Renderer(scene, 0, lib)
    src = np.full(n, 0x5A, np.uint8)
    d_src = lib.rt_alloc_device(0, n)
    assert d_src and lib.rt_memset_device(0, d_src, 0xA5, n) == 0
    host_s, dev_ms = [], []
    for k in range(4):                                     # (the first of each is the warm-up)
        t0 = time.perf_counter()
        assert lib.rt_scene_set_texels(r.handle, 0, 0, 0, side, side, src.ctypes.data, 0, stream) == 0, lib.rt_last_error()
        assert hip.hipStreamSynchronize(stream) == 0
        host_s.append(time.perf_counter() - t0)
        assert hip.hipEventRecord(e0, stream) == 0
        assert lib.rt_scene_set_texels_device(r.handle, 0, 0, 0, side, side, d_src, 0, stream) == 0, lib.rt_last_error()
        assert hip.hipEventRecord(e1, stream) == 0 and hip.hipStreamSynchronize(stream) == 0
        t = C.c_float()
        assert hip.hipEventElapsedTime(C.byref(t), e0, e1) == 0
        dev_ms.append(t.value)
    r.close()
    gb = n / 1e9
    print(json.dumps({"mode": "big", "bytes": n, "host_form_s": host_s[1:], "host_form_GBps": [gb / s for s in host_s[1:]],
                      "device_form_ms": dev_ms[1:], "device_form_GBps_written": [gb / (1e-3 * m) for m in dev_ms[1:]]}))


def run(args, env=None):
    p = subprocess.run([sys.executable, os.path.abspath(__file__), "--one"] + args, env=env, stdout=subprocess.PIPE, text=True, timeout=600)
    if p.returncode != 0:                                  # (a run that failed ends the measurement: nothing more is started on the GPU)
        sys.exit("run %s failed (exit status %d)" % (args, p.returncode))
    row = json.loads(p.stdout.strip().splitlines()[-1])
    print(json.dumps(row), flush=True)
    return row


def main(out, parent_lib, repeats):
    rows = []
    for rep in range(repeats):
        rows.append(run(["blit"]))
        for change in ("1", "0"):
            rows.append(dict(run(["host", change]), library="this"))
            rows.append(dict(run(["host", change], dict(os.environ, RT_HIP_LIB=parent_lib, RT_HIP_LIB_OLDER="1")), library="parent"))
    rows.append(run(["big"]))
    if out:
        with open(out, "w") as f:
            json.dump({"w": W, "h": H, "repeats": repeats, "runs": rows}, f, indent=1)


if __name__ == "__main__":
    a = sys.argv[1:]
    if a and a[0] == "--one":
        {"blit": blit, "host": lambda: host(a[2] == "1"), "big": big}[a[1]]()
    else:
        main(a[0] if a else None, a[1] if len(a) > 1 else os.path.join(ROOT, "build", "ab", "librt_hip_parent.so"), int(a[2]) if len(a) > 2 else 3)
