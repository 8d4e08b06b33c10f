"""Count, with the HOST build of the launch table and the C restatement's per-sample probe (no GPU), what the second-node bits state
(rt_block.h: rt_second_node_bits) - per WAVE, as profiles/count_first_bounce.py --per-wave counts the first-bounce sets.

    python3 profiles/count_second_node.py [scene] [w] [h]        default: h8 3840 2160
    python3 profiles/count_second_node.py --frames               h8 at 3840x2160, 7680x4320 and 1001x563, one line each

A wave (an 8-pixel column of a 32 x 8 block) counts when at least one of its samples has a second node (the scene read at depth 2).  Per frame:
  bouncing_waves      such waves of entries that state a first-bounce set, and the sphere tests they walk with the sets alone;
  sky_waves           those whose entry states SKY: the wave ends its reflected rays at the primary node's fold;
  self_tests_dropped  first-bounce tests the SELF bits take out of the walks (one per bouncing wave and named candidate);
  dark                the second node's SHADOW scans, per light: the bouncing waves with a lit second-node hit that faces the light (they
                      run one scan of every loop sphere); those of them whose entry states DARK for the light (rt_block.h:
                      rt_cand_second_dark; stated_waves, stated_tests at n_loop per scan - THE count the statement is decided on: at least
                      40 000 per headline launch, or it is not built); and, as the ceiling of any such statement, those in which NO lane's
                      segment to the light meets a loop sphere by the shadow rule (main.js:293-304), exact from the samples;
  masks               what full per-sphere masks for the second node (a fifth word per entry; not built) could add at most, exact from the
                      samples: a scanning wave would test only the spheres that SOME lane's segment meets (met_tests) instead of every loop
                      sphere (scan_tests); masks_ceiling = scan_tests - met_tests over the waves whose entry states no DARK for the light -
                      what is left to gain beside the DARK bits.  A conservative per-block mask names more spheres than the samples meet.
"""
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "html5-canvas-raytracer_amd"))
sys.path.insert(0, os.path.join(ROOT, "profiles"))
import rt_host  # noqa: E402
from count_first_bounce import table  # noqa: E402

SECOND_NODE = 1 | 2 | 4 | 32 | 128 | 256 | 512     # ranked, sky marks, masks + candidates, checker cells, first-bounce sets, second-node bits, DARK bits
EPS = 0.001


def count(lib, scene, w, h):
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import oracle_util as ou
    c = ou.c_oracle()
    c.oracle_probe_sample.restype = C.c_int
    c.oracle_probe_sample.argtypes = [C.c_void_p, C.c_size_t, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p]
    blob = rt_host.flatten_scene(dict(scene, segs=2))
    buf = C.create_string_buffer(blob, len(blob))
    ss = scene.get("supersample", 1)
    loop = [i for i, o in enumerate(scene["objects"]) if o["r2"] != 25000000]          # h8's skybox is outside the loops
    tab = table(lib, rt_host.flatten_scene(scene), w, h, SECOND_NODE)
    live = tab[((tab[:, 0] >> 11) & 15 != 0) & (tab[:, 1] >> 31 == 0) & (tab[:, 3] >> 31 == 1)]
    rec = np.zeros(64 * 24)
    nodes = rec.reshape(64, 24)
    out = {"stating_entries": len(live), "sky_entries": int(((live[:, 1] >> 26) & 1).sum()), "bouncing_waves": 0, "tests_with_sets": 0,
           "sky_waves": 0, "self_waves": 0, "self_tests_dropped": 0}
    wave_of, hit_p, hit_n, hit_i, wave_sn = [], [], [], [], []
    n_waves = 0
    for w0, w1, _, w3 in live:
        tile_x, rows_valid, frow0 = int(w0) & 2047, (int(w0) >> 11) & 15, int(w0) >> 15
        sn, size = (int(w1) >> 24) & 31, bin((int(w3) >> 18) & 0x1fff).count("1")
        for col in range(4):
            n = 0
            for sy in range(frow0 * ss, (frow0 + rows_valid) * ss):
                for sx in range((tile_x * 32 + col * 8) * ss, min((tile_x * 32 + col * 8 + 8) * ss, w * ss)):
                    rec[:] = 0.0
                    assert c.oracle_probe_sample(buf, len(blob), w, h, sx, sy, rec.ctypes.data) == 0
                    second = nodes[(nodes[:, 23] == 1.0) & (nodes[:, 0] == 2.0)]
                    if len(second):
                        n += 1
                        if second[0, 1] >= 0 and (int(second[0, 1]) >> 1) in loop:
                            wave_of.append(n_waves); hit_p.append(second[0, 3:6].copy()); hit_n.append(second[0, 6:9].copy()); hit_i.append(int(second[0, 1]) >> 1)
            if n:
                n_waves += 1
                wave_sn.append(sn)
                out["bouncing_waves"] += 1
                out["tests_with_sets"] += size
                out["sky_waves"] += 1 if sn & 4 else 0
                out["self_waves"] += 1 if sn & 3 else 0
                out["self_tests_dropped"] += bin(sn & 3).count("1")
    # the second node's shadow scans: an exact count from the samples (see the head comment)
    dark = []
    if hit_p:
        wave_of, hit_p, hit_n, hit_i = np.array(wave_of), np.array(hit_p), np.array(hit_n), np.array(hit_i)
        lit = np.array([scene["objects"][i]["mtl"]["albedo"][1] > 0 or scene["objects"][i]["mtl"]["albedo"][2] > 0 for i in hit_i])
        wave_sn = np.array(wave_sn)
        for k, li in enumerate(scene["lights"][:2]):
            sraw = np.array(li, dtype=np.float64) - hit_p
            llen = np.sqrt((sraw * sraw).sum(axis=1))
            sv = sraw / llen[:, None]
            scans = lit & ((sv * hit_n).sum(axis=1) > 0.0)
            met = np.zeros(len(hit_p), dtype=bool)
            met_pairs = set()                                           # (wave, sphere): some scanning lane's segment meets it
            for si in loop:
                o = scene["objects"][si]
                L = np.array(o["origin"], dtype=np.float64) - hit_p
                tca = (sv * L).sum(axis=1)
                d2 = (L * L).sum(axis=1) - tca * tca
                ok = ~(d2 > o["r2"])
                thc = np.sqrt(np.where(ok, o["r2"] - d2, 0.0))
                t0, t1 = tca - thc, tca + thc
                t = np.where(t0 < EPS, t1, t0)
                m1 = ok & (hit_i != si) & (t < llen) & ~(t < EPS)
                met |= m1
                met_pairs.update((int(wv), si) for wv in np.unique(wave_of[scans & m1]))
            scanning = np.unique(wave_of[scans])
            shadowed = np.unique(wave_of[scans & met])
            stated = scanning[(wave_sn[scanning] >> (3 + k)) & 1 == 1]
            assert not np.isin(stated, shadowed).any()                  # a stated wave with a shadowed lane: the statement would be wrong
            stated_set = set(stated.tolist())
            rest = len(scanning) - len(stated)
            met_rest = sum(1 for wv, _ in met_pairs if wv not in stated_set)
            dark.append({"scanning_waves": len(scanning), "stated_waves": len(stated), "stated_tests": len(stated) * len(loop),
                         "masks": {"scan_tests": rest * len(loop), "met_tests": met_rest, "masks_ceiling": rest * len(loop) - met_rest},
                         "waves_no_lane_shadowed": len(scanning) - len(shadowed), "tests_upper_bound": (len(scanning) - len(shadowed)) * len(loop)})
    out["dark"] = dark
    out["dark_stated_tests"] = sum(d["stated_tests"] for d in dark)
    out["dark_tests_upper_bound"] = sum(d["tests_upper_bound"] for d in dark)
    out["masks_ceiling"] = sum(d["masks"]["masks_ceiling"] for d in dark)
    return out


def report(lib, name, w, h):
    print(name, w, h, json.dumps(count(lib, rt_host.load_scene(name), w, h)), flush=True)


if __name__ == "__main__":
    lib = rt_host.load_library()
    args = sys.argv[1:]
    if args[:1] == ["--frames"]:
        for w, h in ((3840, 2160), (7680, 4320), (1001, 563)):
            report(lib, "h8", w, h)
        sys.exit(0)
    name = args[0] if args else "h8"
    w, h = (int(args[1]), int(args[2])) if len(args) > 2 else (3840, 2160)
    report(lib, name, w, h)
