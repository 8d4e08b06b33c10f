"""TEST INFRASTRUCTURE for the ray-list tests (tests/test_rays.py, tests/test_gpu_rays.py): arbitrary rays whose expected colour and hit
record come from the unchanged C restatement (oracle/rt_oracle.c), which traces camera rays only - through MICRO-CAMERAS.

Pixel (sx, sy) of a 2 x 2 frame from the camera {origin o, axisX (a, 0, 0), axisY (0, b, 0), axisZ (0, 0, c)} is the ray
unit(((o + a d0) - o, (o + b d1) - o, (o + c d2) - o)) with d = (sx - 1 + 0.5, 1 - sy - 0.5, 1 / tan(fov / 2)): any origin, and any
direction by choice of a, b, c.  The four rays are computed here in numpy; the expected bytes are c_oracle_render(blob with that
camera, 2, 2), the expected hit record hits_util.Probe's root record.  Four rays at list positions 0..3 also have the stars sampler's
pix of the 2 x 2 frame's pixels.  The scene the library holds keeps its own camera: only the oracle sees the micro-camera."""
import ctypes as C
import math
import struct

import numpy as np

import hits_util as hu
import oracle_util as ou
import rt_host

CAMERA_OFFSET, SEGS_OFFSET, SUPERSAMPLE_OFFSET = 16, 160, 164        # in rt_scene_header (include/rt_hip.h)
SMALL_R2 = 1e4                                                         # below: a sphere of the scene proper (not the floor, not the skybox)


def micro_rays(cams, fov_deg):
    """cams (m, 6) = {origin[3], a, b, c} -> (4 m, 6) rays {org, dir}: camera j's pixels (0,0), (1,0), (0,1), (1,1) at 4 j .. 4 j + 3,
    main.js:184-193 operation for operation (the zero axis components add +-0 products, which change nothing)."""
    cams = np.asarray(cams, np.float64)
    m = cams.shape[0]
    proj_d = 1.0 / math.tan(fov_deg * math.pi / 180.0 / 2.0)
    sx = np.array([0.0, 1.0, 0.0, 1.0])
    sy = np.array([0.0, 0.0, 1.0, 1.0])
    d = np.stack([(sx - 1.0) + 0.5, (1.0 - sy) - 0.5, np.full(4, proj_d)], axis=1)          # (4, 3)
    o = cams[:, None, 0:3]                                                                    # (m, 1, 3)
    abc = cams[:, None, 3:6]
    rays = np.empty((m, 4, 6), np.float64)
    for c in range(3):
        terms = [np.zeros((m, 4)), np.zeros((m, 4)), np.zeros((m, 4))]                       # axisX[c] d, axisY[c] d, axisZ[c] d
        terms[c] = abc[..., c] * d[None, :, c]
        target = ((o[..., c] + terms[0]) + terms[1]) + terms[2]
        rays[..., c] = o[..., c]
        rays[..., 3 + c] = target - o[..., c]
    rays[..., 3:] = rt_host.normal3d(rays[..., 3:])
    return rays.reshape(4 * m, 6)


def _camera_words(cam):
    o, (a, b, c) = cam[0:3], cam[3:6]
    return [*o, a, 0.0, 0.0, 0.0, b, 0.0, 0.0, 0.0, c]


class MicroOracle:
    """The restatement's answers for micro-cameras of one scene (at the scene's depth, or `segs`)."""

    def __init__(self, scene, segs=None):
        s = dict(scene)
        s["supersample"] = 1                              # the 2 x 2 frame is the four rays themselves
        if segs is not None:
            s["segs"] = segs
        self.scene = s
        self.blob = bytearray(rt_host.flatten_scene(s))
        self.probe = hu.Probe(s, 2, 2)                    # (its blob: the same scene at depth 1)
        self.fov = float(s.get("fovDeg", 60))

    def expected(self, cams):
        """-> rgba (4 m, 4) uint8, roots (4 m, 24) float64: the restatement's bytes and root probe records, in micro_rays' order."""
        m = len(cams)
        rgba = np.empty((m, 4, 4), np.uint8)
        roots = np.empty((m, 4, hu.PROBE_WORDS), np.float64)
        for j, cam in enumerate(np.asarray(cams, np.float64)):
            words = _camera_words(cam)
            struct.pack_into("<12d", self.blob, CAMERA_OFFSET, *words)
            struct.pack_into("<12d", self.probe.buf, CAMERA_OFFSET, *words)
            rgba[j] = np.frombuffer(ou.c_oracle_render(bytes(self.blob), 2, 2), np.uint8).reshape(4, 4)
            for k in range(4):
                roots[j, k] = self.probe.root(k & 1, k >> 1)
        return rgba.reshape(4 * m, 4), roots.reshape(4 * m, hu.PROBE_WORDS)

    def hit_of(self, q):
        """A root probe record as the rt_hit the library returns (rt_host._hit_dict's form), None for a miss."""
        code = int(q[1])
        if code < 0:
            return None
        u, v = self.probe.uv(q[6:9])
        return {"object": code >> 1, "inside": bool(code & 1), "t": float(q[2]), "point": [float(x) for x in q[3:6]],
                "normal": [float(x) for x in q[6:9]], "u": u, "v": v}


def draw_cameras(scene, count, seed, outside_radius=None):
    """`count` micro-cameras {origin, a, b, c} from a fixed seed: most origins in a box of +-4 around the scene, a fifth inside
    spheres of the scene proper (refracting ones first in line), and - outside_radius given - a tenth beyond that radius.
    a, b, c in +-2: directions in all octants."""
    rng = np.random.default_rng(seed)
    cams = np.empty((count, 6), np.float64)
    cams[:, 0:3] = rng.uniform(-4.0, 4.0, (count, 3)) + np.array([0.0, 1.5, 0.0])
    cams[:, 3:6] = rng.uniform(-2.0, 2.0, (count, 3))
    small = [o for o in scene["objects"] if o["r2"] < SMALL_R2]
    small.sort(key=lambda o: -o["mtl"]["albedo"][4])
    n_in = count // 5 if small else 0
    for j in range(n_in):
        o = small[j % min(len(small), 8)]
        v = rng.normal(size=3)
        v *= 0.8 * rng.uniform() ** (1.0 / 3.0) * math.sqrt(o["r2"]) / np.linalg.norm(v)
        cams[j, 0:3] = np.array(o["origin"], np.float64) + v
    if outside_radius is not None:
        for j in range(n_in, n_in + count // 10):
            v = rng.normal(size=3)
            cams[j, 0:3] = v / np.linalg.norm(v) * outside_radius * rng.uniform(1.2, 3.0)
    return cams


def store_rule(rgb):
    """The Uint8ClampedArray store of 255 * rgb (main.js:195-198) in numpy: NaN -> 0, clamp, round half to even; alpha 255."""
    v = 255.0 * np.asarray(rgb, np.float64)
    v = np.where(np.isnan(v), 0.0, v)
    out = np.full((v.shape[0], 4), 255, np.uint8)
    out[:, :3] = np.rint(np.clip(v, 0.0, 255.0)).astype(np.uint8)
    return out


def hits_equal(got, want):
    """rt_hit dicts: object and inside exact, t, point, normal bit for bit, u and v equal."""
    if got is None or want is None:
        return got is None and want is None
    words = lambda h: struct.pack("<9d", h["t"], *h["point"], *h["normal"], h["u"], h["v"])
    return got["object"] == want["object"] and got["inside"] == want["inside"] and words(got) == words(want)
