"""The vector side of the reflection-only product frame kernels: the one-instruction clamps of the uniform-material path's leaf and of the
fold (rt_kernel_math.h: rt_min1_nn, rt_min_nn, rt_max_nn - IEEE minNum / maxNum, which return the NUMBER of a NaN and a number where the
reference's Math.min(1, NaN) is NaN), the path's way out for a camera inside its candidate, the reflection in l instead of the restored
normal, and its normalisation without selects (unit_go).  What can go wrong is a NaN that a one-instruction clamp swallows, a wave that
takes the fast arm beside a lane that needed the exact one, a sign that mattered after all, and a direction read by a lane that was not
meant to read it.  So the scenes put NaN where the clamps are - a material constant of infinity makes 0 * inf - beside clamped lanes in
ONE wave, and bounce inside a sphere, where l = -n at every node.

Every test passes on the parent commit's libraries too (run there once: docs/EVIDENCE.md, "Vector diet"): they pin behaviour, not the change.
Frames are held as tests/test_gpu_prologue_loads.py holds its shapes - second frame == first frame == the test library's general path ==
the product library's, and within 1 LSB of the C restatement (oracle/rt_oracle.c) - except where a docstring says otherwise."""
import copy
import hashlib
import os

import numpy as np
import pytest

import oracle_util as ou
import rt_host
import test_gpu_prologue_loads as pl          # hold, frames, restatement: the three yardsticks
import test_gpu_scalar_paths as sp            # floor_alone, low_camera: the one-floor-sphere band
from objects_util import fresh, tlib  # noqa: F401  (tlib: fixture, the test library)
from test_gpu_prologue_loads import lib, plib  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu

INF, NAN = float("inf"), float("nan")
W, H = 64, 16
BAND = (H, 3, 1, 1)                  # tile 3 of four 16-row tiles of a W x 64 frame: eight waves in each of two rows
WHITE = dict(sampler={"kind": 0}, color=[1, 1, 1])


def equal_frames(lib, plib, scene, w, h, tiles=None):
    """hold()'s byte-for-byte clauses without its restatement clause; returns (the frame, the waves that completed the uniform-material path)."""
    tiles = tiles or (h, 0, 1, 1)
    (first, second), took = pl.frames(lib, scene, w, h, tiles, count=True)
    os.environ[pl.SWITCH] = "1"
    try:
        (_, general), none = pl.frames(lib, scene, w, h, tiles, count=True)
    finally:
        os.environ.pop(pl.SWITCH, None)
    assert none == 0, none
    assert second == first, "one-wave frame differs from the four-wave frame"
    assert second == general, "one-wave frame differs from the general path's"
    (pfirst, psecond), _ = pl.frames(plib, scene, w, h, tiles)
    assert psecond == pfirst, "product library: one-wave frame differs from the four-wave frame"
    assert psecond == second, "product library's frame differs from the test library's"
    return second, took


def nan_pixels_per_wave(rows, w, h):
    """Pixels whose three channels are byte 0, per 8x8 wave of a w x h band (row-major), and the mask itself."""
    a = np.frombuffer(rows, dtype=np.uint8).reshape(h, w, 4)
    z = (a[:, :, :3] == 0).all(axis=2)
    return [int(z[y:y + 8, x:x + 8].sum()) for y in range(0, h, 8) for x in range(0, w, 8)], z


def shadowed_floor(**mtl):
    """tests/test_gpu_scalar_paths.py's shadow scene: the floor alone from h8's camera, a small ball between light 0 and the band."""
    s = sp.floor_alone(**mtl)
    ball = copy.deepcopy(next(o for o in pl.h8()["objects"] if o["r2"] == 1))
    ball["origin"], ball["r2"] = [3.0, 6.0, 5.4], 0.09
    s["objects"].insert(0, ball)
    return s


def side_light(s):
    s = sp.low_camera(s)
    s["lights"] = [[3, 2, 11]]          # beside and behind the low camera: the mirrored light faces the eye on the band's left, away from it on its right
    return s


# scene, and what the C restatement's rows must show: waves that hold NaN pixels AND others, NaN pixels in no wave / in every wave (strict: see there)
BAND_SCENES = {
    # specular albedo inf: a lane whose mirrored light faces away keeps specular = 0 and 0 * inf is NaN; the others clamp inf to 1
    "a2_inf_mixed": (lambda: side_light(sp.floor_alone(albedo=[0, 0.5, INF, 0, 0], **WHITE)), "mixed"),
    # diffuse albedo inf: the ball's shadow (li = 0, diffuse = 0: NaN) crosses waves whose other lanes clamp inf to 1
    "a1_inf_shadow_mixed": (lambda: shadowed_floor(albedo=[0, INF, 0.8, 0, 0], **WHITE), "mixed"),
    # a colour channel inf: the ambient term inf * 0 is NaN in every lane, the channel sums are inf (the first operand of the outer clamp).
    # Held to the STRICT kernel's frame: maxa(NaN, x) is x in both kernels where the reference's Math.max(NaN, x) is NaN, so the channel is
    # byte 255 here and 0 in the restatement - at the parent commit too (docs/EVIDENCE.md, "Vector diet": a finding of its own)
    "colour_inf": (lambda: sp.low_camera(sp.floor_alone(sampler={"kind": 0}, color=[INF, 0.5, 0.5])), "strict"),
    "no_nan": (lambda: sp.low_camera(sp.floor_alone()), "none"),                              # h8's floor as it is: the fast arm in every wave
    "a1_nan_uniform": (lambda: sp.low_camera(sp.floor_alone(albedo=[0, NAN, 0.8, 0, 0])), "all"),   # the exact arm in every wave
}


@pytest.mark.parametrize("name", sorted(BAND_SCENES))
def test_nan_beside_clamped_lanes_on_the_uniform_path(lib, plib, name):
    """The 64x16 band of one floor sphere, every wave on the uniform-material path: waves that hold NaN pixels beside clamped ones (asserted
    from the restatement's rows), waves with none, waves of nothing else.  Held as hold() holds; a NaN pixel is byte 0 in all channels."""
    make, kind = BAND_SCENES[name]
    scene = make()
    per_wave, z = nan_pixels_per_wave(pl.restatement(scene, W, 4 * H, BAND), W, H)
    print(name, "NaN pixels per wave, by the restatement:", per_wave)
    if kind == "mixed":
        assert any(0 < n < 64 for n in per_wave), per_wave          # no wave trivially skips the arm
    elif kind == "none":
        assert not any(per_wave), per_wave
    elif kind == "all":
        assert all(n == 64 for n in per_wave), per_wave
    frame, took = equal_frames(lib, plib, scene, W, 4 * H, tiles=BAND)
    assert took > 0, "no wave took the uniform-material path"
    if kind == "strict":
        strict = fresh(plib, scene, W, 4 * H, tiles=BAND, flags=rt_host.RT_FLAG_STRICT_FP)
        lsb, frac = ou.max_lsb(frame, strict)
        print(name, "|product - strict| <= %d LSB in %.2e of the channels" % (lsb, frac))
        assert lsb <= 1, (lsb, frac)
        return
    assert pl.hold(lib, plib, scene, W, 4 * H, tiles=BAND) == took
    got, zg = nan_pixels_per_wave(frame, W, H)
    assert (zg == z).all(), (got, per_wave)                          # the NaN pixels, exactly: byte 0 in all channels, and no others


def mirror_of(s):
    return next(o for o in s["objects"] if o["mtl"]["albedo"][3] > 0 and o["r2"] < pl.FLOOR_R2)


def h8_mirror(**mtl):
    s = pl.h8()
    m = mirror_of(s)["mtl"]
    for k, v in mtl.items():
        if k == "a2":
            m["albedo"][2] = v
        else:
            m[k] = v
    return s


# sha256 of the product library's frame at the PARENT commit (the product fold swallows a NaN child - maxNum / minNum - so these frames
# are not the restatement's; recorded once with the parent's libraries, docs/EVIDENCE.md "Vector diet")
PARENT_SHA256 = {
    ("a2_inf", 96, 24): "83ba83105ca95063c0e610685cbd7b5e6caaa90772951ead641f8a6d0e06e819",
    ("a2_inf", 33, 9): "77be6104782e9cf85e9bc940541b701ec9fe1d496a50b26a746761b90ca475a4",
    ("colour_inf", 96, 24): "2eaa0c0a838f21d926a273d84a854e1a27b0ac6e9b5ce24cf648d669be6b1374",
    ("colour_inf", 33, 9): "c5ad12269fee88afc899621e632b91a7002461f29977a4b41422d9165a5acc18",
}


@pytest.mark.parametrize("w,h", [(96, 24), (33, 9)])
@pytest.mark.parametrize("variant", ["plain", "a2_inf", "colour_inf"])
def test_general_leaf_and_fold(lib, plib, variant, w, h):
    """h8 with one mirror's specular albedo, and separately its colour, infinite: a NaN leaf under a fold, a clamped leaf under a fold, and a
    NaN that appears only at the second node (33x9: odd both ways - rt_retrace takes the centre lines).  The frames with an infinite constant
    are held byte for byte to what the parent commit's product library gave; plain h8 to the restatement within 1 LSB."""
    if variant == "plain":
        pl.hold(lib, plib, pl.h8(), w, h)
        return
    scene = h8_mirror(a2=INF) if variant == "a2_inf" else h8_mirror(color=[INF, 0.5, 0.5], sampler={"kind": 0})
    frame, _ = equal_frames(lib, plib, scene, w, h)
    sha = hashlib.sha256(frame).hexdigest()
    lsb, frac = ou.max_lsb(frame, pl.restatement(scene, w, h, (h, 0, 1, 1)))
    print("%s %dx%d sha256 %s; against the restatement: %d LSB in %.2e of the channels (not asserted)" % (variant, w, h, sha, lsb, frac))
    assert sha == PARENT_SHA256[(variant, w, h)]


def inside_mirror():
    """h8 seen from inside a mirror sphere of radius 3 around its camera (off centre): every node of every sample is `inside`, l = -n."""
    s = pl.h8()
    o = copy.deepcopy(next(x for x in s["objects"] if x["r2"] == 1))
    c = s["camera"]["origin"]
    o["origin"], o["r2"] = [c[0] + 0.4, c[1] - 0.3, c[2] + 0.5], 9.0
    o["mtl"].update(albedo=[0.1, 0.5, 0.3, 0.6, 0], sampler={"kind": 0}, color=[0.9, 0.7, 0.5], specular_exponent=10)
    s["objects"].insert(0, o)
    s["segs"] = 3
    return s


@pytest.mark.parametrize("w,h", [(32, 8), (33, 9)])
def test_bounces_inside_a_mirror_sphere(lib, plib, w, h):
    """Reflection-only kernel, depth 3, every bounce from the inside: held as hold() holds, and within 1 LSB of the strict kernel's frame."""
    scene = inside_mirror()
    pl.hold(lib, plib, scene, w, h)
    strict = fresh(plib, scene, w, h, flags=rt_host.RT_FLAG_STRICT_FP)
    product = fresh(plib, scene, w, h)
    lsb, frac = ou.max_lsb(product, strict)
    print("%dx%d inside a mirror: |product - strict| <= %d LSB in %.2e of the channels" % (w, h, lsb, frac))
    assert lsb <= 1, (lsb, frac)
    assert len(set(product[i:i + 4] for i in range(0, len(product), 4))) > 8, "a flat frame: the scene does not test what it is meant to"


def test_mirrors_from_outside(lib, plib):
    pl.hold(lib, plib, pl.h8(), 100, 20)


def test_camera_inside_the_floor_sphere_leaves_the_uniform_path(lib, plib):
    """The camera below the floor's surface: every primary ray meets the floor sphere from the inside.  The launch table names no
    candidate the camera is inside of, so no wave takes the uniform-material path - and should it ever name one, the path's hit test sends
    the wave back to the general path.  Frames held as hold() holds."""
    s = sp.floor_alone(albedo=[0.3, 0.5, 0.8, 0, 0])          # (an ambient term: from the inside no light faces the surface)
    s["camera"]["origin"] = [0.0, -0.5, 10.0]
    took = pl.hold(lib, plib, s, W, H)
    assert took == 0, took
