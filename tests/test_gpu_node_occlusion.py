"""RT.occlusion and RT.lightSegments from Node on the GPU (js/index.js, napi/rt_napi.cc): the default14 case of tests/occlusion_util.py -
the reference's light loop over every lit node of the ray trees, held to the C restatement's q[18] bit for bit."""
import base64
import json
import os

import numpy as np
import pytest
import subprocess

import occlusion_util as ocu
import oracle_util as ou

pytestmark = pytest.mark.gpu
ROOT = ou.ROOT
PKG = os.path.join(ROOT, "html5-canvas-raytracer_amd")


@pytest.mark.skipif(ou.node_path() is None or not os.path.exists(os.path.join(PKG, "napi", "rt_napi.node")), reason="node or the addon not present")
def test_node_light_loop_is_the_probes(built):
    nd, sg = ocu.nodes("default14"), ocu.segments("default14")
    b64 = lambda a, t: base64.b64encode(np.ascontiguousarray(a, t).tobytes()).decode()
    out = subprocess.check_output([ou.node_path(), os.path.join(ROOT, "tests", "js_occlusion_check.js"), PKG, "default14",
                                   b64(nd["point"], np.float64), b64(nd["facing"], np.float64), b64(nd["sphere"], np.int32)], text=True, timeout=300)
    res = json.loads(out.strip().splitlines()[-1])
    got = np.frombuffer(base64.b64decode(res["intensity"]), np.float64)
    assert got.tobytes() == nd["expected"].tobytes(), int((got.view(np.uint64) != nd["expected"].view(np.uint64)).sum())
    assert res["same"] is True                             # {bin: true}: the same bytes
    for k, blockers in enumerate(res["blockers"]):        # per light, the segments of the nodes that face it, in node order
        assert blockers == sg["want_blocker"][sg["light"] == k].tolist()
    assert res["bare"] == [None, True, 2]                  # no blocker unless asked for; a non-finite ray is NaN
