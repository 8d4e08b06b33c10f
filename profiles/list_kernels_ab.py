#!/usr/bin/env python3
"""The ray-list kernels of this build against another build's (the parent commit's librt_hip.so), both loaded in one process, on the
same device buffers: the 3840x2160 primary rays of h8 and default14 as a list (8.3 M rays).
  hits             rt_render_hits_device, id + depth + normal             rt_stats.kernel_ms
  ray hits         rt_scene_trace_rays_device, hits only                   rt_stats.kernel_ms
  occlusion        rt_scene_occlusion_device, default inputs               rt_stats.kernel_ms
  occlusion lights ... the segments of rt_host.light_segments to light 0 from the list's hit points (length, skip)
  shade            rt_scene_shade_rays_device                              rt_stats.kernel_ms
  spawn, fold      one level: the children of shade's nodes, and their fold   host clock around the call and a device synchronise
  order            rt_scene_order_rays_device                              host clock around the call and a device synchronise
Per kernel 3 warm-up calls per library, then `reps` repetitions in which the two libraries alternate (parent first).  The margin is the
parent's own range (max - min) in this run: "slower" is a new median above the parent's median by more than that.
   python3 profiles/list_kernels_ab.py <reps> <out.json> <parent librt_hip.so>"""
import ctypes
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "html5-canvas-raytracer_amd"))
import numpy as np
import rt_host

reps, out_path, parent_path = int(sys.argv[1]), sys.argv[2], sys.argv[3]
assert reps >= 6
w, h = 3840, 2160
libs = {"parent": rt_host.load_library(parent_path), "new": rt_host.load_library()}
for lib in libs.values():
    assert lib.rt_init(1) == 0
new = libs["new"]
hip = ctypes.CDLL("libamdhip64.so")
HIT = np.dtype([("object", "<i4"), ("inside", "<i4"), ("t", "<f8"), ("point", "<f8", 3), ("normal", "<f8", 3), ("u", "<f8"), ("v", "<f8")])


def alloc(nbytes, src=None):
    p = new.rt_alloc_device(0, nbytes)
    assert p, new.rt_last_error()
    if src is not None:
        src = np.ascontiguousarray(src)
        assert src.nbytes == nbytes and hip.hipMemcpy(ctypes.c_void_p(p), src.ctypes.data_as(ctypes.c_void_p), ctypes.c_size_t(nbytes), 1) == 0
    return p


def clocked(call):
    assert hip.hipDeviceSynchronize() == 0
    t0 = time.perf_counter()
    call()
    assert hip.hipDeviceSynchronize() == 0
    return (time.perf_counter() - t0) * 1e3


def ab(calls, by_stats):
    """calls: {library name: callable} -> per library the times of the alternating repetitions, and the verdict."""
    one = (lambda c: c().kernel_ms) if by_stats else clocked
    for c in calls.values():
        for _ in range(3):
            one(c)
    ms = {"parent": [], "new": []}
    for _ in range(reps):
        for name in ("parent", "new"):
            ms[name].append(one(calls[name]))
    res = {name: {"ms": v, "median_ms": statistics.median(v), "range_ms": max(v) - min(v)} for name, v in ms.items()}
    res["new_minus_parent_ms"] = res["new"]["median_ms"] - res["parent"]["median_ms"]
    res["slower"] = res["new_minus_parent_ms"] > res["parent"]["range_ms"]
    res["clock"] = "rt_stats.kernel_ms" if by_stats else "host clock, device synchronised"
    return res


out = {"w": w, "h": h, "reps": reps, "scenes": {}}
for name in ("h8", "default14"):
    scene = rt_host.load_scene(name)
    k = scene.get("supersample", 1)
    R = {ln: rt_host.Renderer(scene, 0, lib) for ln, lib in libs.items()}
    rays = rt_host.primary_rays(w, h, scene)
    n = samples = len(rays)                                 # (k w x k h: the sample grid)
    assert n == k * w * k * h
    d_rays = alloc(n * 48, rays)
    d_id, d_depth, d_normal = alloc(samples * 4), alloc(samples * 8), alloc(samples * 12)
    d_hits, d_li, d_bl, d_nodes = alloc(n * 80), alloc(n * 8), alloc(n * 4), alloc(n * 200)
    res = {"rays": n}
    res["hits"] = ab({ln: (lambda r=r: r.render_hits(w, h, d_id, d_depth, d_normal, want_stats=True)) for ln, r in R.items()}, True)
    res["ray hits"] = ab({ln: (lambda r=r: r.trace_rays(n, d_rays, 0, 0, d_hits, want_stats=True)) for ln, r in R.items()}, True)
    res["occlusion"] = ab({ln: (lambda r=r: r.occlusion(n, d_rays, 0, 0, 0, d_li, d_bl, want_stats=True)) for ln, r in R.items()}, True)
    # the segments from the list's hit points to the first light
    hits = np.empty(n, HIT)
    assert new.rt_copy_to_host(0, hits.ctypes.data, d_hits, n * 80) == 0
    facing = np.where((hits["inside"] != 0)[:, None], -hits["normal"], hits["normal"])
    sg = rt_host.light_segments(scene, hits["point"], facing, hits["object"])[0]
    d_seg, d_len, d_skip = alloc(n * 48, sg["rays"]), alloc(n * 8, sg["length"]), alloc(n * 4, sg["skip"])
    res["occlusion lights"] = ab({ln: (lambda r=r: r.occlusion(n, d_seg, d_len, 0, d_skip, d_li, d_bl, want_stats=True)) for ln, r in R.items()}, True)
    for p in (d_seg, d_len, d_skip, d_id, d_depth, d_normal, d_hits):
        new.rt_free_device(0, p)
    res["shade"] = ab({ln: (lambda r=r: r.shade_rays(n, d_rays, d_nodes, want_stats=True)) for ln, r in R.items()}, True)
    # one level: d_nodes holds shade's nodes (the same bytes from either library)
    wb = rt_host.nodes_spawn_work_bytes(n, new)
    d_child, d_links, d_count, d_work = alloc(2 * n * 48), alloc(n * 8), alloc(4), alloc(wb)
    res["spawn"] = ab({ln: (lambda r=r: r.spawn_rays(n, d_nodes, d_child, d_links, d_count, d_work, wb)) for ln, r in R.items()}, False)
    count = np.zeros(1, np.uint32)
    assert new.rt_copy_to_host(0, count.ctypes.data, d_count, 4) == 0
    res["spawn"]["children"] = int(count[0])
    new.rt_free_device(0, d_child)
    d_crgb, d_rgba = alloc(2 * n * 24, np.full(2 * n * 3, 0.25)), alloc(n * 4)
    res["fold"] = ab({ln: (lambda r=r: r.fold_nodes(n, d_nodes, d_links, d_crgb, 0, d_rgba)) for ln, r in R.items()}, False)
    for p in (d_crgb, d_rgba, d_links, d_count, d_work, d_nodes, d_li, d_bl):
        new.rt_free_device(0, p)
    ob = rt_host.rays_order_work_bytes(n, new)
    d_order, d_owork = alloc(n * 4), alloc(ob)
    res["order"] = ab({ln: (lambda r=r: r.order_rays(n, d_rays, d_order, d_owork, ob)) for ln, r in R.items()}, False)
    for p in (d_order, d_owork, d_rays):
        new.rt_free_device(0, p)
    for r in R.values():
        r.close()
    out["scenes"][name] = res
    for key, v in res.items():
        if key != "rays":
            print("%-10s %-17s parent %9.3f ms (range %.3f)   new %9.3f ms (range %.3f)   new - parent %+.3f ms  %s"
                  % (name, key, v["parent"]["median_ms"], v["parent"]["range_ms"], v["new"]["median_ms"], v["new"]["range_ms"], v["new_minus_parent_ms"],
                     "SLOWER" if v["slower"] else "within the parent's range"), flush=True)
with open(out_path, "w") as f:
    json.dump(out, f, indent=1)
