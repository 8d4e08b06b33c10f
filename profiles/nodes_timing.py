#!/usr/bin/env python3
"""The wavefront loop (rt_scene_shade_rays_device / rt_scene_spawn_rays_device / rt_scene_fold_nodes_device, the count read back per
level) against rt_scene_trace_rays_device on the same build: the primary rays of default14 and H8 at 3840x2160 as a ray list, in row
order and shuffled (one fixed permutation), the loop without and with per-level ordering (rt_scene_order_rays_device on every level
after the first), at the scene's own depth, rgba out.
Times are host clocks around work that ends in a device synchronise (the loop's stages: order, shade, spawn + count read-back, fold)
and rt_stats.kernel_ms for the recursive call; per configuration one warm-up pass, then `reps` passes in which the recursive call and
the loop alternate; medians.  The loop's buffers are allocated in the warm-up pass from the counts it reads back and used again (the
counts are a function of the list); the bytes they hold are reported.
   python3 profiles/nodes_timing.py [reps] [out.json]"""
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

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 5
w, h = 3840, 2160
n = w * h
lib = rt_host.load_library()
assert lib.rt_init(1) == 0
hip = ctypes.CDLL("libamdhip64.so")


def sync():
    assert hip.hipDeviceSynchronize() == 0


class Pool:
    """Device buffers by name, allocated on first use and kept."""

    def __init__(self):
        self.p, self.bytes = {}, 0

    def get(self, name, nbytes):
        if name not in self.p:
            self.p[name] = (lib.rt_alloc_device(0, max(nbytes, 16)), nbytes)
            assert self.p[name][0], lib.rt_last_error()
            self.bytes += nbytes
        assert self.p[name][1] >= nbytes, name
        return self.p[name][0]

    def close(self):
        for p, _ in self.p.values():
            lib.rt_free_device(0, p)


def stage(times, key, call):
    t0 = time.perf_counter()
    call()
    sync()
    times[key] = times.get(key, 0.0) + (time.perf_counter() - t0) * 1e3


def wavefront(r, pool, d_rays, d_rgba, segs, order_levels):
    """One pass of the loop -> (per-level counts, per-level stage times in ms)."""
    counts, levels = [], []
    rays, pix, path, c = d_rays, 0, 0, n
    for lv in range(segs):
        if c == 0:
            break
        t = {}
        counts.append(c)
        nodes = pool.get("nodes%d" % lv, c * 200)
        order = 0
        if order_levels and lv > 0:
            wb = rt_host.rays_order_work_bytes(c, lib)
            order, owork = pool.get("order%d" % lv, c * 4), pool.get("owork%d" % lv, wb)
            stage(t, "order_ms", lambda: r.order_rays(c, rays, order, owork, wb))
        stage(t, "shade_ms", lambda: r.shade_rays(c, rays, nodes, order_ptr=order, pix_ptr=pix, path_ptr=path))
        nxt = 0
        if lv + 1 < segs:
            wb = rt_host.nodes_spawn_work_bytes(c, lib)
            links, swork, count = pool.get("links%d" % lv, c * 8), pool.get("swork%d" % lv, wb), pool.get("count", 4)
            crays, cpix, cpath = pool.get("rays%d" % (lv + 1), 2 * c * 48), pool.get("pix%d" % (lv + 1), 2 * c * 4), pool.get("path%d" % (lv + 1), 2 * c * 4)
            got = np.zeros(1, np.uint32)

            def spawn():
                r.spawn_rays(c, nodes, crays, links, count, swork, wb, pix_ptr=pix, path_ptr=path, child_pix_ptr=cpix, child_path_ptr=cpath)
                assert lib.rt_copy_to_host(0, got.ctypes.data, count, 4) == 0
            stage(t, "spawn_ms", spawn)
            nxt = int(got[0])
            rays, pix, path = crays, cpix, cpath
        levels.append(t)
        c = nxt
    child = 0
    for lv in reversed(range(len(counts))):
        rgb = pool.get("rgb%d" % lv, counts[lv] * 24) if lv else 0            # (level 1 writes the list's rgba)
        links = pool.p["links%d" % lv][0] if lv + 1 < len(counts) else 0
        stage(levels[lv], "fold_ms", lambda: r.fold_nodes(counts[lv], pool.p["nodes%d" % lv][0], links, child, rgb, d_rgba if lv == 0 else 0))
        child = rgb
    return counts, levels


out = {"w": w, "h": h, "rays": n, "reps": reps, "scenes": {}}
for name in ("default14", "h8"):
    scene = rt_host.load_scene(name)
    segs = scene["segs"]
    rays = rt_host.primary_rays(w, h, scene)
    perm = np.random.default_rng(1).permutation(n)
    lists = {"row order": rays, "shuffled": np.ascontiguousarray(rays[perm])}
    r = rt_host.Renderer(scene, 0, lib)
    res = {"segs": segs}
    for list_name, src in lists.items():
        d_rays = lib.rt_alloc_device(0, src.nbytes)
        assert hip.hipMemcpy(ctypes.c_void_p(d_rays), src.ctypes.data_as(ctypes.c_void_p), ctypes.c_size_t(src.nbytes), 1) == 0
        d_rgba, d_rgba_rec = lib.rt_alloc_device(0, n * 4), lib.rt_alloc_device(0, n * 4)
        for order_levels in (False, True):
            pool = Pool()
            wavefront(r, pool, d_rays, d_rgba, segs, order_levels)            # warm-up: code objects, allocations
            r.trace_rays(n, d_rays, 0, d_rgba_rec, 0, want_stats=True)
            rec_ms, wave_ms, per_level, counts = [], [], [], None
            for _ in range(reps):
                rec_ms.append(r.trace_rays(n, d_rays, 0, d_rgba_rec, 0, want_stats=True).kernel_ms)
                counts, levels = wavefront(r, pool, d_rays, d_rgba, segs, order_levels)
                per_level.append(levels)
                wave_ms.append(sum(sum(t.values()) for t in levels))
            a, b = np.empty(n * 4, np.uint8), np.empty(n * 4, np.uint8)
            assert lib.rt_copy_to_host(0, a.ctypes.data, d_rgba, n * 4) == 0 and lib.rt_copy_to_host(0, b.ctypes.data, d_rgba_rec, n * 4) == 0
            med = lambda key, lv: statistics.median(p[lv].get(key, 0.0) for p in per_level)
            res["%s, %s" % (list_name, "levels ordered" if order_levels else "levels as spawned")] = {
                "recursive_median_ms": statistics.median(rec_ms), "recursive_min_ms": min(rec_ms),
                "wavefront_median_ms": statistics.median(wave_ms), "wavefront_min_ms": min(wave_ms),
                "wavefront_over_recursive": statistics.median(wave_ms) / statistics.median(rec_ms),
                "same_bytes": bool((a == b).all()), "device_bytes_held": pool.bytes,
                "levels": [{"rays": counts[lv], **{k: round(med(k, lv), 3) for k in ("order_ms", "shade_ms", "spawn_ms", "fold_ms")}} for lv in range(len(counts))]}
            pool.close()
        for p in (d_rays, d_rgba, d_rgba_rec):
            lib.rt_free_device(0, p)
    r.close()
    out["scenes"][name] = res
print(json.dumps(out, indent=1))
if len(sys.argv) > 2:
    with open(sys.argv[2], "w") as f:
        json.dump(out, f, indent=1)
