"""Ambient occlusion from Node (js/index.js: RT.ambient, RT.ambientView, RT.ambientDirs -> napi/rt_napi.cc -> rt_ambient, rt_ambient_view,
rt_ambient_cosine_dirs): the table is the library's own, bit for bit, and the results are the bytes Python's rt_host.ambient and
rt_host.ambient_view give for the same receivers."""
import base64
import json
import os
import subprocess

import numpy as np
import pytest

import oracle_util as ou
import rt_host

ROOT = ou.ROOT
PKG = os.path.join(ROOT, "html5-canvas-raytracer_amd")
CHECK = os.path.join(ROOT, "tests", "js_ambient_check.js")
pytestmark = pytest.mark.skipif(ou.node_path() is None, reason="node not installed")
W, H = 40, 24


def node(*args):
    r = subprocess.run([ou.node_path(), CHECK, PKG] + [str(a) for a in args], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    return json.loads(r.stdout.strip().splitlines()[-1])


def test_the_table_is_pythons_bits(built):
    out = node("dirs")
    for n, d in zip([1, 16, 64], out["dirs"]):
        assert base64.b64decode(d) == rt_host.ambient_dirs(n).tobytes(), n


@pytest.mark.gpu
def test_node_gives_pythons_bytes(built):
    out = node("ambient", W, H)
    scene = rt_host.load_scene("default14")
    c = scene["camera"]
    v = rt_host.view(rt_host.RT_VIEW_PINHOLE, c["origin"], c["axisX"], c["axisY"], c["axisZ"], scene["fovDeg"])
    hits = rt_host.view_hit_records(scene, v, W, H)
    keys = ("open", "intensity", "rgba")
    py = rt_host.ambient(scene, hits, 5, 2.0, dirs=rt_host.ambient_dirs(64), stride=7, want=keys)
    assert 0 < ((py["open"] > 0) & (py["open"] < 1)).sum() and len({bytes(q) for q in py["rgba"]}) > 3       # a picture, not a constant
    assert out["list"]["type"] == "[object Uint8ClampedArray]"
    for k in keys:
        assert base64.b64decode(out["list"][k]) == py[k].tobytes(), k
        assert base64.b64decode(out["view"][k]) == py[k].tobytes(), k
        assert base64.b64decode(out["pieces"][0][k]) + base64.b64decode(out["pieces"][1][k]) == py[k].tobytes(), k
    pv = rt_host.ambient_view(scene, v, W, H, 5, 2.0, dirs=rt_host.ambient_dirs(64), stride=7, want=keys)
    assert all(pv[k].tobytes() == py[k].tobytes() for k in keys)
    # the defaults
    plain = rt_host.ambient(scene, hits[:50], 16, float("inf"))
    assert base64.b64decode(out["plain"]["open"]) == plain["open"].tobytes() and out["plain"]["intensity"] is None and out["plain"]["rgba"] is None
    picture = rt_host.ambient_view(scene, v, W, H, 5, 2.0)
    assert base64.b64decode(out["picture"]["rgba"]) == picture["rgba"].tobytes() and out["picture"]["open"] is None and out["picture"]["intensity"] is None
    assert out["refused"] == "TypeError"
