"""TEST INFRASTRUCTURE for the occlusion tests (tests/test_occlusion.py, tests/test_gpu_occlusion.py): a scalar Python restatement of
the reference's shadow scan (main.js:293-304, intersectSphere :420-439) and the expected values it is held against - the intensity the
C restatement's probe (oracle/rt_oracle.c, q[18]) records after the light loop of every lit node of a sample's ray tree.

Python floats are binary64, `*`, `+`, `-`, `/` and math.sqrt are correctly rounded and nothing here is contracted: the restatement
carries the bits of the reference's expressions."""
import ctypes as C
import functools
import math

import numpy as np

import hits_util as hu
import rt_host

INF = float("inf")

# (scene, w, h) of the probe runs, the scenes at their own depth
CASES = {"default14": ("default14", 64, 36), "h8": ("h8", 64, 36), "lcg64_ss1": ("lcg64_ss1", 96, 96)}


def sphere_table(scene):
    """[(ox, oy, oz, r2, albedo[4])] of the scene dict's spheres, in blob order."""
    return [(float(o["origin"][0]), float(o["origin"][1]), float(o["origin"][2]), float(o["r2"]), float(o["mtl"]["albedo"][4])) for o in scene["objects"]]


def intersect_t(sph, eps, org, d):
    """intersectSphere(obj, org, dir, null) (main.js:420-439): t, or +Infinity."""
    lx, ly, lz = sph[0] - org[0], sph[1] - org[1], sph[2] - org[2]
    tca = d[0] * lx + d[1] * ly + d[2] * lz
    d2 = (lx * lx + ly * ly + lz * lz) - tca * tca
    if d2 > sph[3]:
        return INF
    x = sph[3] - d2
    thc = math.sqrt(x) if x >= 0.0 else float("nan")       # (NaN only for a NaN d2)
    t0, t1 = tca - thc, tca + thc
    if t0 < t1:
        if t0 < eps:
            if t1 < eps:
                return INF
            return t1
        return t0
    if t1 < eps:
        if t0 < eps:
            return INF
        return t0
    return t1


def scan(table, eps, ray, length, intensity, skip):
    """The scan of main.js:293-304 for one segment -> (intensity, blocker): a non-finite ray is not traced (NaN, -1)."""
    if not all(math.isfinite(x) for x in ray):
        return float("nan"), -1
    org, d = ray[0:3], ray[3:6]
    li = intensity
    for j, sph in enumerate(table):
        if j == skip:
            continue
        if intersect_t(sph, eps, org, d) < length:
            if sph[4] != 0.0:
                li = li / sph[4]
            else:
                return 0.0, j
    return li, -1


def scan_list(scene, rays, length=None, intensity=None, skip=None):
    """scan over a list, with the library's defaults for an input that is None -> (intensity float64 (n,), blocker int32 (n,))."""
    table, eps = sphere_table(scene), float(scene.get("epsilon", 0.001))
    n = len(rays)
    li, bl = np.empty(n, np.float64), np.empty(n, np.int32)
    default = float(scene.get("light_intensity", 50))
    for i in range(n):
        li[i], bl[i] = scan(table, eps, [float(x) for x in rays[i]], INF if length is None else float(length[i]),
                            default if intensity is None else float(intensity[i]), -1 if skip is None else int(skip[i]))
    return li, bl


@functools.lru_cache(maxsize=None)
def nodes(case):
    """Every hit node of every sample's ray tree (the scene at its own depth) whose sphere has albedo[1] > 0 || albedo[2] > 0 - the nodes
    whose light loop runs: {"point" (m, 3) = q[3:6], "facing" (m, 3) = hit.l (q[6:9], negated when inside), "sphere" (m,) = q[1] >> 1,
    "expected" (m,) = q[18], "overflowed": samples whose probe filled all its records}."""
    name, w, h = CASES[case]
    scene = rt_host.load_scene(name)
    probe = hu.Probe(scene, w, h)
    blob = rt_host.flatten_scene(scene)                    # (hu.Probe flattens at depth 1: here the scene's own depth)
    buf = C.create_string_buffer(blob, len(blob))
    k = scene.get("supersample", 1)
    objs = scene["objects"]
    point, facing, sphere, expected, overflowed = [], [], [], [], 0
    for sy in range(k * h):
        for sx in range(k * w):
            assert probe.lib.oracle_probe_sample(buf, len(blob), w, h, sx, sy, probe.rec.ctypes.data) == 0
            used = probe.rec[probe.rec[:, 23] == 1]
            overflowed += len(used) >= hu.PROBE_NODES
            for q in used:
                code = int(q[1])
                if code < 0:
                    continue
                a = objs[code >> 1]["mtl"]["albedo"]
                if not (a[1] > 0 or a[2] > 0):
                    continue
                point.append(q[3:6].copy())
                facing.append(-q[6:9] if code & 1 else q[6:9].copy())
                sphere.append(code >> 1)
                expected.append(q[18])
    return {"scene": scene, "point": np.array(point), "facing": np.array(facing), "sphere": np.array(sphere, np.int32),
            "expected": np.array(expected), "overflowed": overflowed}


@functools.lru_cache(maxsize=None)
def segments(case):
    """The segments of nodes(case) the reference scans (lights in order, shadow_dot > 0), each with the intensity the chaining rule
    hands it and the restatement's answer: {"rays" (s, 6), "length", "intensity" (in), "skip", "node", "light", "want_intensity",
    "want_blocker"} in node-major order, and "final" (m,): the intensity after the whole light loop per node."""
    nd = nodes(case)
    scene = nd["scene"]
    table, eps = sphere_table(scene), float(scene.get("epsilon", 0.001))
    per_light = rt_host.light_segments(scene, nd["point"], nd["facing"], nd["sphere"])
    m = len(nd["sphere"])
    out = {k: [] for k in ("rays", "length", "intensity", "skip", "node", "light", "want_intensity", "want_blocker")}
    final = np.empty(m, np.float64)
    for i in range(m):
        li = float(scene.get("light_intensity", 50))
        for k, sg in enumerate(per_light):
            if not sg["shadow_dot"][i] > 0:
                continue
            ray = [float(x) for x in sg["rays"][i]]
            got, blocker = scan(table, eps, ray, float(sg["length"][i]), li, int(nd["sphere"][i]))
            for key, v in (("rays", ray), ("length", float(sg["length"][i])), ("intensity", li), ("skip", int(nd["sphere"][i])), ("node", i),
                           ("light", k), ("want_intensity", got), ("want_blocker", blocker)):
                out[key].append(v)
            li = got
        final[i] = li
    res = {"rays": np.array(out["rays"], np.float64).reshape(-1, 6), "final": final}
    for key in ("length", "intensity", "want_intensity"):
        res[key] = np.array(out[key], np.float64)
    for key in ("skip", "node", "light", "want_blocker"):
        res[key] = np.array(out[key], np.int32)
    return res


def classes(case):
    """(unchanged, zeroed, raised) nodes: the expected intensity equal to, zero, above the scene's."""
    nd = nodes(case)
    li = float(nd["scene"].get("light_intensity", 50))
    e = nd["expected"]
    return int((e == li).sum()), int((e == 0).sum()), int((e > li).sum())


def same_bits(a, b):
    return np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes()
