"""Sampled lights from Node (js/index.js: RT.lighting, RT.lightingView, RT.lightingOffsets -> napi/rt_napi.cc -> rt_lighting,
rt_lighting_view, rt_lighting_sphere_offsets): the table is the library's own, bit for bit, and the results are the bytes Python's
rt_host.lighting and rt_host.lighting_view give for the same receivers."""
import base64
import json
import os
import subprocess

import pytest

import oracle_util as ou
import rt_host

ROOT = ou.ROOT
PKG = os.path.join(ROOT, "html5-canvas-raytracer_amd")
CHECK = os.path.join(ROOT, "tests", "js_lighting_check.js")
pytestmark = pytest.mark.skipif(ou.node_path() is None, reason="node not installed")
W, H = 40, 24
KEYS = ("diffuse", "intensity", "lit", "rgba")


def node(*args):
    r = subprocess.run([ou.node_path(), CHECK, PKG] + [str(a) for a in args], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    return json.loads(r.stdout.strip().splitlines()[-1])


def test_the_table_is_pythons_bits(built):
    out = node("offsets")
    for n, d in zip([1, 16, 64], out["offsets"]):
        assert base64.b64decode(d) == rt_host.lighting_offsets(n).tobytes(), n


@pytest.mark.gpu
def test_node_gives_pythons_bytes(built):
    out = node("lighting", W, H)
    scene = rt_host.load_scene("default14")
    c = scene["camera"]
    v = rt_host.view(rt_host.RT_VIEW_PINHOLE, c["origin"], c["axisX"], c["axisY"], c["axisZ"], scene["fovDeg"])
    hits = rt_host.view_hit_records(scene, v, W, H)
    offs = rt_host.lighting_offsets(64)
    py = rt_host.lighting(scene, hits, 5, 1.0, offs=offs, stride=7, want=KEYS)
    assert 0 < ((py["lit"] > 0) & (py["lit"] < 1)).sum() and len({bytes(q) for q in py["rgba"]}) > 3       # a picture, not a constant
    assert out["list"]["type"] == "[object Uint8ClampedArray]"
    for k in KEYS:
        assert base64.b64decode(out["list"][k]) == py[k].tobytes(), k
        assert base64.b64decode(out["view"][k]) == py[k].tobytes(), k
        assert base64.b64decode(out["pieces"][0][k]) + base64.b64decode(out["pieces"][1][k]) == py[k].tobytes(), k
    pv = rt_host.lighting_view(scene, v, W, H, 5, 1.0, offs=offs, stride=7, want=KEYS)
    assert all(pv[k].tobytes() == py[k].tobytes() for k in KEYS)
    # the defaults
    plain = rt_host.lighting(scene, hits[:50])
    assert base64.b64decode(out["plain"]["diffuse"]) == plain["diffuse"].tobytes()
    assert out["plain"]["intensity"] is None and out["plain"]["lit"] is None and out["plain"]["rgba"] is None
    picture = rt_host.lighting_view(scene, v, W, H, 5, 1.0)
    assert base64.b64decode(out["picture"]["rgba"]) == picture["rgba"].tobytes()
    assert out["picture"]["diffuse"] is None and out["picture"]["intensity"] is None and out["picture"]["lit"] is None
    assert out["refused"] == ["TypeError"] * 3
