"""Count, with the HOST build of the launch table (no GPU), what the first-bounce sets state (rt_block.h: rt_first_bounce_set).

    python3 profiles/count_first_bounce.py [scene] [w] [h]        default: h8 3840 2160
    python3 profiles/count_first_bounce.py --frames               h8 at 3840x2160, 7680x4320 and 1001x563, one line each
    ... --per-wave                                                also the count per WAVE (below), with the C restatement's probe: a minute per 4K frame

Prints the stating entries (bit 31 of word 3), their waves (four per entry: every one of them may hold a mirror hit, and a wave that
holds one scans the entry's set at its first bounce instead of all the loop spheres), the summed set sizes against the full scan's tests,
the saving, and the entries by set size.  An upper bound on the saving: a wave of a stating entry none of whose primary rays meets the
mirror never bounces and scans nothing either way.  --per-wave counts exactly that: the waves of stating entries with at least one
sample whose ray tree has a second node (oracle/rt_oracle.c's per-sample probe, the scene read at depth 2), the tests of those waves
with the full scan and with their entry's set, and the saving - the number the change was decided on (at least 60 000 for the headline
frame)."""
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "html5-canvas-raytracer_amd"))
import rt_host  # noqa: E402

FIRST_BOUNCE = 1 | 2 | 4 | 32 | 128          # ranked, sky marks, masks + candidates, checker cells, first-bounce sets


def table(lib, blob, w, h, flags=FIRST_BOUNCE, tiles=None):
    t = rt_host.RtTiles(*(tiles or (h, 0, 1, 1)))
    buf = C.create_string_buffer(blob, len(blob))
    n, nb = C.c_uint32(), C.c_uint32()
    assert lib.rt_scene_launch_table(buf, len(blob), w, h, C.byref(t), flags, None, C.byref(n), C.byref(nb)) == 0, lib.rt_last_error()
    out = (C.c_uint32 * (4 * 8 * ((nb.value + 7) // 8)))()
    assert lib.rt_scene_launch_table(buf, len(blob), w, h, C.byref(t), flags, out, C.byref(n), C.byref(nb)) == 0, lib.rt_last_error()
    return np.frombuffer(out, dtype=np.uint32).reshape(-1, 4).copy()


def loop_spheres(scene):
    """Spheres the per-ray loops walk: all of them but an enclosing one (h8's skybox)."""
    return sum(1 for o in scene["objects"] if o["r2"] != 25000000)


def counts(tab, n_loop):
    live = tab[(tab[:, 0] >> 11) & 15 != 0]
    live = live[live[:, 1] >> 31 == 0]
    stating = live[live[:, 3] >> 31 == 1]
    sizes = np.array([bin((int(w3) >> 18) & 0x1fff).count("1") for w3 in stating[:, 3]], dtype=np.int64)
    waves = 4 * len(stating)
    return {"entries": len(live), "stating_entries": len(stating), "stating_waves": waves, "tests_full_scan": waves * n_loop,
            "tests_with_sets": int(4 * sizes.sum()), "tests_saved": int(waves * n_loop - 4 * sizes.sum()),
            "mean_set": round(float(sizes.mean()), 3) if len(sizes) else 0.0,
            "entries_by_set_size": {int(k): int((sizes == k).sum()) for k in range(1, n_loop + 1)}}


def per_wave(tab, scene, w, h, n_loop):
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import oracle_util as ou
    c = ou.c_oracle()
    c.oracle_probe_sample.restype = C.c_int
    c.oracle_probe_sample.argtypes = [C.c_void_p, C.c_size_t, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p]
    blob = rt_host.flatten_scene(dict(scene, segs=2))
    buf = C.create_string_buffer(blob, len(blob))
    ss = scene.get("supersample", 1)
    rec = np.zeros(64 * 24)
    nodes = rec.reshape(64, 24)
    live = tab[((tab[:, 0] >> 11) & 15 != 0) & (tab[:, 1] >> 31 == 0) & (tab[:, 3] >> 31 == 1)]
    waves = samples = with_sets = 0
    for w0, _, _, w3 in live:
        tile_x, rows_valid, frow0 = int(w0) & 2047, (int(w0) >> 11) & 15, int(w0) >> 15
        size = bin((int(w3) >> 18) & 0x1fff).count("1")
        for col in range(4):
            n = 0
            for sy in range(frow0 * ss, (frow0 + rows_valid) * ss):
                for sx in range((tile_x * 32 + col * 8) * ss, min((tile_x * 32 + col * 8 + 8) * ss, w * ss)):
                    rec[:] = 0.0
                    assert c.oracle_probe_sample(buf, len(blob), w, h, sx, sy, rec.ctypes.data) == 0
                    n += 1 if ((nodes[:, 23] == 1.0) & (nodes[:, 0] == 2.0)).any() else 0
            if n:
                waves, samples, with_sets = waves + 1, samples + n, with_sets + size
    return {"bouncing_waves": waves, "bouncing_samples": samples, "tests_full_scan": waves * n_loop, "tests_with_sets": with_sets,
            "tests_saved": waves * n_loop - with_sets}


def report(lib, name, w, h, waves=False):
    scene = rt_host.load_scene(name)
    tab = table(lib, rt_host.flatten_scene(scene), w, h)
    c = counts(tab, loop_spheres(scene))
    if waves:
        c["per_wave"] = per_wave(tab, scene, w, h, loop_spheres(scene))
    print(name, w, h, json.dumps(c))
    return c


if __name__ == "__main__":
    lib = rt_host.load_library()
    args = [a for a in sys.argv[1:] if a != "--per-wave"]
    waves = "--per-wave" in sys.argv[1:]
    if args[:1] == ["--frames"]:
        for w, h in ((3840, 2160), (7680, 4320), (1001, 563)):
            report(lib, "h8", w, h, waves)
        sys.exit(0)
    name = args[0] if args else "h8"
    w, h = (int(args[1]), int(args[2])) if len(args) > 2 else (3840, 2160)
    report(lib, name, w, h, waves)
