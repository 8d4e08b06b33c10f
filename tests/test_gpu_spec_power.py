"""The product kernel's specular power (rt_kernel.hip: rt_pow_spec) on constructed scenes: the host classifies each material's
exponent once (rt_device.h: rt_spec_n), and the kernel takes a scalar walk when a wave's lanes share one integer exponent, a per-lane
walk when they do not, and OCML's pow for the rest.  Every path is held to <= 1 LSB against the C restatement, and a restyle that
changes nothing but an exponent must render what a fresh upload of the edited scene renders."""
import copy

import numpy as np
import pytest

import rt_host
from objects_util import Frames, fresh, oracle_gap

pytestmark = pytest.mark.gpu

W, H = 160, 96
FLOOR_R2 = 250000.0


@pytest.fixture(scope="module")
def lib(built):
    lib = rt_host.load_library()
    rc = lib.rt_init(1)
    assert rc == 0, lib.rt_last_error()
    return lib


def h8():
    return rt_host.load_scene("h8")


def floor(s):
    return next(i for i, o in enumerate(s["objects"]) if o["r2"] == FLOOR_R2)


def three_spheres(s):
    """The three unit spheres of h8 (blue in the middle, red, green), in that order."""
    return [i for i, o in enumerate(s["objects"]) if o["r2"] == 1.0]


def mixed_h8(refract=False):
    """h8 with five exponents among the floor, the three unit spheres and the small mirror: 10, 2.5 (OCML's pow), 3, 7, 500."""
    s = h8()
    s["objects"][floor(s)]["mtl"]["specular_exponent"] = 10
    for i, e in zip(three_spheres(s), (2.5, 3, 7)):
        s["objects"][i]["mtl"]["specular_exponent"] = e
    if refract:                                        # the general (refracting) kernel
        m = s["objects"][three_spheres(s)[1]]["mtl"]
        m["albedo"][4], m["refract_index"] = 0.7, 1.4
    return s


def near_oracle(frame, scene, w, h):
    worst, frac = oracle_gap(frame, scene, w, h)
    assert worst <= 1, (worst, frac)


def test_one_block_sees_several_exponents_and_a_generic_one(lib):
    """At 32x24 the three unit spheres and the floor share 8x8 blocks: some block's primary hits alone carry at least three integer
    exponents and the non-integer one."""
    w, h = 32, 24
    s = mixed_h8()
    ids = rt_host.hits(w, h, s, lib)["id"]            # blob order, | inside << 16; -1 on a miss
    exps = [o["mtl"]["specular_exponent"] for o in s["objects"]]
    best = 0
    for by in range(0, h, 8):
        for bx in range(0, w, 8):
            e = {exps[i & 0xFFFF] for i in np.unique(ids[by:by + 8, bx:bx + 8]) if i >= 0}
            if 2.5 in e:
                best = max(best, len(e - {2.5}))
    assert best >= 3, best
    near_oracle(rt_host.render(w, h, s, lib=lib)[0], s, w, h)


@pytest.mark.parametrize("refract", [False, True], ids=["reflect", "refract"])
@pytest.mark.parametrize("wh", [(32, 24), (W, H)], ids=["32x24", "160x96"])
def test_mixed_exponents_within_1_lsb(lib, wh, refract):
    s = mixed_h8(refract)
    near_oracle(fresh(lib, s, *wh), s, *wh)


@pytest.mark.parametrize("e", [0, 1, 2, 65536, 65537, 2.5])
def test_exponents_at_the_ends_of_the_integer_range(lib, e):
    """0 (x^0 = 1), 1, 2, the largest integer exponent and the first one past it (OCML's pow), on every sphere that has a highlight:
    each wave has one exponent."""
    s = h8()
    for o in s["objects"]:
        if o["mtl"]["albedo"][2] > 0:
            o["mtl"]["specular_exponent"] = e
    near_oracle(fresh(lib, s, W, H), s, W, H)


def test_many_sphere_scene_with_mixed_exponents(lib):
    """The many-sphere kernels read their materials from HBM: exponents cycled over the spheres, generic ones included."""
    s = rt_host.load_scene("lcg64")
    cycle = (0, 1, 2, 3, 10, 2.5, 50, 65536, 65537, 0.5)
    for k, o in enumerate(s["objects"]):
        o["mtl"]["specular_exponent"] = cycle[k % len(cycle)]
    near_oracle(fresh(lib, s, W, H), s, W, H)


@pytest.mark.parametrize("name,e", [("h8", 3), ("h8", 2.5), ("h8", 65537), ("lcg64", 2.5)])
def test_a_restyle_of_an_exponent_renders_as_a_fresh_upload(lib, name, e):
    """rt_scene_set_objects with records that differ only in specular_exponent: the next frame changes, and equals a fresh upload's."""
    s = rt_host.load_scene(name)
    t = copy.deepcopy(s)
    if name == "h8":
        ids = [floor(t)]
    else:
        ids = [i for i, o in enumerate(t["objects"]) if o["mtl"]["albedo"][2] > 0]
    for i in ids:
        t["objects"][i]["mtl"]["specular_exponent"] = e
    r = rt_host.Renderer(rt_host.flatten_scene(s), 0, lib)
    try:
        f = Frames(lib, W, H, (H, 0, 1, 1))
        f.render(r)
        for i in ids:
            r.set_objects(t["objects"][i:i + 1], i)
        f.render(r)
        r.set_objects(s["objects"], 0)
        f.render(r)
        before, after, back = f.read()
    finally:
        r.close()
    assert after != before
    assert after == fresh(lib, t, W, H)
    assert back == before == fresh(lib, s, W, H)
    near_oracle(after, t, W, H)
