"""TEST INFRASTRUCTURE: scenes that carry RT_MAX_TEXTURES textures of odd shapes, built in code (no fixture file).

The texels come from a seeded generator in which every texel differs from each of its four neighbours in at least one channel,
so that a texel index off by one anywhere - a `ceil(u * w) - 1` edge at width or height 1, the product kernel's fixed-point floor
at width 16384 - changes the colour of the sample.  Used by tests/test_gpu_restyle.py, tests/test_oracle.py and
oracle/record_reference_results.py (which records the reference's frames of these scenes)."""
import copy

import numpy as np

import rt_host

MAX_TEXTURES = 16                      # include/rt_hip.h RT_MAX_TEXTURES
# (width, height): the degenerate shapes first, then the widest and tallest the library admits (16384)
SHAPES = [(1, 1), (3, 7), (257, 129), (16384, 2), (2, 16384), (1, 9), (9, 1), (2, 2),
          (5, 3), (31, 17), (64, 1), (1, 64), (128, 96), (7, 5), (33, 65), (256, 128)]
assert len(SHAPES) == MAX_TEXTURES


def texels(w, h, seed):
    """w x h RGBA8 texels (bytes).  Red steps by 37 per column and green by 53 per row (odd steps: a neighbour in x or y never has the
    same red / green), blue is seeded noise, alpha 255."""
    rng = np.random.default_rng(seed)
    x = np.arange(w, dtype=np.int64)[None, :]
    y = np.arange(h, dtype=np.int64)[:, None]
    off = int(rng.integers(0, 256))
    t = np.empty((h, w, 4), dtype=np.uint8)
    t[..., 0] = (x * 37 + y * 11 + off) & 255
    t[..., 1] = (y * 53 + x * 7 + 3 * off) & 255
    t[..., 2] = rng.integers(0, 256, size=(h, w), dtype=np.uint8)
    t[..., 3] = 255
    return t.tobytes()


def textures(seed=1):
    return [{"width": w, "height": h, "texels": texels(w, h, seed * 1000 + k)} for k, (w, h) in enumerate(SHAPES)]


def with_textures(scene, seed=1):
    """A copy of `scene` whose texture table is the MAX_TEXTURES generated ones (its texture samplers keep their indices, which are
    below 3 in every scene here)."""
    s = copy.deepcopy(scene)
    s["textures"] = textures(seed)
    return s


def textured(scene, assign):
    """A copy of `scene` with sphere i drawing texture k for every i: k in `assign` (colour white, so the texel is the colour)."""
    s = copy.deepcopy(scene)
    for i, k in assign.items():
        m = s["objects"][i]["mtl"]
        m["sampler"] = {"kind": rt_host.SAMPLER_TEXTURE, "texture": k}
        m["color"] = [1.0, 1.0, 1.0]
    return s


# Scenes whose reference frames are recorded (tests/golden/reference_results.json "texture_scenes"): h8's four small spheres and its
# two planets draw six of the textures each, so that the three scenes together show all sixteen.
H8_SPHERES = (0, 2, 3, 4, 1, 5)
ORACLE_SCENES = [
    ("h8_tex_a", (0, 5, 6, 3, 4, 1), 160, 90),
    ("h8_tex_b", (2, 7, 8, 9, 10, 11), 128, 72),
    ("h8_tex_c", (12, 13, 14, 15, 3, 0), 96, 54),
]


def oracle_scene(name):
    """(scene, w, h) of one of ORACLE_SCENES."""
    _, ks, w, h = next(x for x in ORACLE_SCENES if x[0] == name)
    return textured(with_textures(rt_host.load_scene("h8")), dict(zip(H8_SPHERES, ks))), w, h

