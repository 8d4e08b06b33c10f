"""Numpy restatements of sampled lights (include/rt_hip.h: struct rt_lighting), written from the header's block and not from
csrc/rt_lighting.h: the segments of one (sample, light) of a list of receivers, the fold of the per-(sample, light) results of
rt_host.occlusion into diffuse, intensity, lit and rgba - the intensity chained from light to light and only the receivers that face a
light scanned, as rt_host.light_intensity_at does -, the receivers the GPU tests share, and the C restatement's per-node records
(q[15] diffuse, q[18] intensity) of the occlusion cases.  numpy's float64 + - * / and sqrt are IEEE operations without contraction, so
what comes out here is compared with the library bit for bit."""
import ctypes as C
import functools

import numpy as np

import ambient_util as au
import hits_util as hu
import occlusion_util as ocu
import rt_host

bits, entry, scanned, hand_built = au.bits, au.entry, au.scanned, au.hand_built
OUTPUTS = ("diffuse", "intensity", "lit", "rgba")


def lights_of(scene_or_lights):
    lights = scene_or_lights["lights"] if isinstance(scene_or_lights, dict) else scene_or_lights
    return np.array(rt_host.light_positions(lights), np.float64).reshape(-1, 3)


def segments(scene_or_lights, hits, offs, sample, light, light_radius, stride=1, base=0):
    """-> the dict rt_host.lighting_segments gives, of (`sample`, `light`): the header's expressions, one numpy operation per operation."""
    n = len(hits)
    ok = scanned(hits)
    ins = (hits["inside"] != 0)[:, None]
    l = np.where(ins, -hits["normal"], hits["normal"])
    p = hits["point"]
    lk = lights_of(scene_or_lights)[light]
    if light_radius == 0.0:
        pos = np.tile(lk, (n, 1))
    else:
        offs = np.asarray(offs, np.float64)
        e = np.array([entry(base, i, stride, sample, len(offs)) for i in range(n)], np.int64)
        pos = lk[None, :] + float(light_radius) * offs[e]
    with np.errstate(all="ignore"):
        sv = pos - p
        mag = (sv[:, 0] * sv[:, 0] + sv[:, 1] * sv[:, 1]) + sv[:, 2] * sv[:, 2]
        length = np.sqrt(mag)
        k = np.where(length != 0.0, 1.0 / length, 1.0)
        sv = np.where((length != 0.0)[:, None], sv * k[:, None], sv)
        dot = (sv[:, 0] * l[:, 0] + sv[:, 1] * l[:, 1]) + sv[:, 2] * l[:, 2]
        rays = np.full((n, 6), np.nan)
        rays[ok, 0:3] = p[ok]
        rays[ok, 3:6] = sv[ok]
        nan = np.full(n, np.nan)
        dot = np.where(ok, dot, nan)
        mask = ~(dot <= 0.0) & ok
    return {"rays": rays, "length": np.where(ok, length, nan), "light_mag": np.where(ok, mag, nan), "shadow_dot": dot, "mask": mask,
            "skip": np.where(ok, hits["object"], -1).astype(np.int32)}


def to_byte(c):
    """The store rule of main.js:195-198: 255 c, a NaN stored as 0, clamped, rounded half to even."""
    with np.errstate(invalid="ignore"):
        return np.rint(np.fmin(np.fmax(255.0 * c, 0.0), 255.0)).astype(np.uint32)


def jsmin1(x):
    """Math.min(1, x): NaN for a NaN."""
    with np.errstate(invalid="ignore"):
        return np.where(np.isnan(x), np.nan, np.where(x > 1.0, 1.0, x))


def fold_samples(x):
    acc = x[0].copy()
    for s in range(1, x.shape[0]):
        acc = acc + x[s]
    with np.errstate(invalid="ignore"):
        return acc / float(x.shape[0])


def by_occlusion(scene, hits, offs, n_samples, light_radius, stride=1, base=0, lib=None, probe=None, occlusion=None):
    """The yardstick of the fused kernel: per sample the light loop over the probe's segments, each light's facing receivers through
    the existing rt_host.occlusion (length = light_len, intensity = what the light before left, the probe's skips), folded in the
    header's order.  -> {"diffuse", "intensity", "lit", "rgba" (uint32), "li" (n_samples, n), "contributed" (n_samples, n)}.
    `occlusion`: another scan with rt_host.occlusion's signature (a CPU one), for checks that must not touch a GPU."""
    probe = probe or (lambda *a, **kw: rt_host.lighting_segments(*a, lib=lib, **kw))
    occlusion = occlusion or (lambda *a, **kw: rt_host.occlusion(*a, lib=lib, **kw))
    n, n_lights = len(hits), len(lights_of(scene))
    ok = scanned(hits)
    li_s, df_s, ct_s = np.empty((n_samples, n)), np.empty((n_samples, n)), np.zeros((n_samples, n), np.int64)
    for s in range(n_samples):
        li = np.full(n, float(scene.get("light_intensity", 50)), np.float64)
        diffuse = np.zeros(n)
        for k in range(n_lights):
            sg = probe(scene, hits, s, k, n_samples, light_radius, offs=offs, stride=stride, base=base)
            m = sg["mask"]
            if not m.any():
                continue
            li[m] = occlusion(scene, sg["rays"][m], length=sg["length"][m], intensity=li[m], skip=sg["skip"][m], want=("intensity",))["intensity"]
            go = m & ~(li == 0.0)
            with np.errstate(invalid="ignore"):
                diffuse[go] = diffuse[go] + (li[go] * sg["shadow_dot"][go]) / sg["light_mag"][go]
            ct_s[s, go] += 1
        li_s[s], df_s[s] = li, diffuse
    diffuse = np.where(ok, fold_samples(df_s), np.nan)
    intensity = np.where(ok, fold_samples(li_s), np.nan)
    lit = ct_s.sum(axis=0).astype(np.float64) / float(n_samples * n_lights) if n_lights else np.zeros(n)
    b = to_byte(jsmin1(diffuse))
    rgba = (b | (b << 8) | (b << 16) | np.uint32(0xff000000)).astype(np.uint32)
    return {"diffuse": diffuse, "intensity": intensity, "lit": lit, "rgba": rgba, "li": li_s, "contributed": ct_s}


def cpu_occlusion(scene, rays, length=None, intensity=None, skip=None, want=("intensity",)):
    """rt_host.occlusion's answer from the scalar Python restatement (occlusion_util.scan_list): no GPU."""
    li, bl = ocu.scan_list(scene, rays, length, intensity, skip)
    return {"intensity": li, "blocker": bl}


def turned_sets(n_samples, sets):
    """`sets` copies of lighting_offsets(n_samples), copy t turned about z by t golden angles, back to back - whole well-spread sets
    for stride = n_samples, as tools/soft_shadows.py builds them.  -> (sets n_samples, 3)."""
    o = rt_host.lighting_offsets(n_samples)
    ang = np.arange(sets) * (np.pi * (3.0 - np.sqrt(5.0)))
    c, s = np.cos(ang)[:, None], np.sin(ang)[:, None]
    x, y, z = o[None, :, 0], o[None, :, 1], o[None, :, 2]
    return np.ascontiguousarray(np.stack([c * x - s * y, s * x + c * y, np.broadcast_to(z, (sets, n_samples))], axis=2).reshape(-1, 3))


@functools.lru_cache(maxsize=None)
def probe_nodes(case):
    """occlusion_util.nodes(case)'s walk again, for what it does not return: per lit node the hit record's own words - "normal" (q[6:9],
    as the reference has hit.n), "inside" (q[1] & 1) - and "diffuse" (q[15]: min(1, diffuse_intensity) * albedo[1]) with "albedo1".
    The nodes come in nodes(case)'s order (asserted), so its "expected" (q[18]) lines up."""
    name, w, h = ocu.CASES[case]
    scene = rt_host.load_scene(name)
    probe = hu.Probe(scene, w, h)
    blob = rt_host.flatten_scene(scene)
    buf = C.create_string_buffer(blob, len(blob))
    k = scene.get("supersample", 1)
    objs = scene["objects"]
    point, normal, inside, sphere, diffuse, albedo1 = [], [], [], [], [], []
    for sy in range(k * h):
        for sx in range(k * w):
            assert probe.lib.oracle_probe_sample(buf, len(blob), w, h, sx, sy, probe.rec.ctypes.data) == 0
            for q in probe.rec[probe.rec[:, 23] == 1]:
                code = int(q[1])
                if code < 0:
                    continue
                a = objs[code >> 1]["mtl"]["albedo"]
                if not (a[1] > 0 or a[2] > 0):
                    continue
                point.append(q[3:6].copy()); normal.append(q[6:9].copy()); inside.append(code & 1); sphere.append(code >> 1)
                diffuse.append(q[15]); albedo1.append(float(a[1]))
    nd = ocu.nodes(case)
    out = {"scene": scene, "point": np.array(point), "normal": np.array(normal), "inside": np.array(inside, np.int32), "sphere": np.array(sphere, np.int32),
           "diffuse": np.array(diffuse), "albedo1": np.array(albedo1), "expected": nd["expected"], "overflowed": nd["overflowed"]}
    assert ocu.same_bits(out["point"], nd["point"]) and np.array_equal(out["sphere"], nd["sphere"])
    assert ocu.same_bits(np.where(out["inside"][:, None] != 0, -out["normal"], out["normal"]), nd["facing"])
    return out


def node_receivers(case):
    nd = probe_nodes(case)
    return rt_host.hit_records(nd["point"], nd["normal"], nd["sphere"], nd["inside"])


def camera_view(scene):
    c = scene["camera"]
    return rt_host.view(rt_host.RT_VIEW_PINHOLE, c["origin"], c["axisX"], c["axisY"], c["axisZ"], scene["fovDeg"])


def oracle_primary_receivers(scene, w, h):
    """The primary hits of the reference's own camera at w x h from the C restatement's probe (hits_util.Probe), as receivers: what a
    view of the scene's camera sees, made without a GPU."""
    pr = hu.Probe(scene, w, h)
    k = scene.get("supersample", 1)
    point, normal, obj, inside = [], [], [], []
    for y in range(h):
        for x in range(w):
            q = pr.root(x * k, y * k)
            code = int(q[1])
            point.append(q[3:6]); normal.append(q[6:9]); obj.append(code >> 1 if code >= 0 else -1); inside.append(code & 1 if code >= 0 else 0)
    return rt_host.hit_records(np.array(point), np.array(normal), np.array(obj), np.array(inside))


def soft_counts(want, scene):
    """(receivers with 0 < lit < 1, receivers whose samples do not agree on how many lights arrive - a penumbra proper -, receivers whose
    intensity exceeds the scene's - glass crossed, carried on) of a by_occlusion result."""
    lit, ct = want["lit"], want["contributed"]
    with np.errstate(invalid="ignore"):
        raised = want["intensity"] > float(scene.get("light_intensity", 50))
    return int(((lit > 0) & (lit < 1)).sum()), int((ct.min(axis=0) != ct.max(axis=0)).sum()), int(raised.sum())
