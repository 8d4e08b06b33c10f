"""Light moves on a resident scene, the parts that need no GPU (include/rt_hip.h: rt_scene_set_lights, rt_scene_set_light_intensity):
the declared and exported entry points, the Python host's argument checks, where the two flatteners keep the lights and their
intensity (rt_render's scene cache diffs exactly those bytes, csrc/rt_frame.hip: scene_for), and the register budget of the kernel
that rewrites a moved light's records (csrc/rt_objects_gpu.hip)."""
import json
import os
import re
import struct
import subprocess

import pytest

import oracle_util as ou
import rt_host
from lights_util import INTENSITY_OFFSET, blob_intensity, blob_lights, lights_offset, move_lights
from test_kernel_resources import TOOLS      # the same code-object tools

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "html5-canvas-raytracer_amd")
CSRC = os.path.join(PKG, "csrc")

needs_node = pytest.mark.skipif(ou.node_path() is None, reason="node not installed")


def test_light_entry_points_are_declared_and_exported(built):
    header = open(os.path.join(ROOT, "include", "rt_hip.h")).read()
    assert re.search(r"int rt_scene_set_lights\(rt_scene_dev \*scene, uint32_t first, uint32_t count, const double \*xyz, void \*hip_stream\);", header)
    assert re.search(r"int rt_scene_set_light_intensity\(rt_scene_dev \*scene, double light_intensity\);", header)
    assert re.search(r"#define RT_ABI_VERSION\s+2u?\b", header)                 # the blob does not change
    assert "rt_scene_set_lights" in rt_host.ABI and "rt_scene_set_light_intensity" in rt_host.ABI
    xyz = (rt_host.C.c_double * 3)(1.0, 2.0, 3.0)
    for path in (None, rt_host.TEST_LIB_PATH):
        lib = rt_host.load_library(path)
        # a NULL scene is refused before any device call: RT_ERR_INVALID also where there is no GPU
        assert lib.rt_scene_set_lights(None, 0, 1, xyz, None) == -1
        assert lib.rt_scene_set_lights(None, 0, 0, None, None) == -1
        assert lib.rt_scene_set_light_intensity(None, 50.0) == -1
        assert b"NULL scene" in lib.rt_last_error()


class _NoLibrary:
    def __getattr__(self, name):
        raise AssertionError("the library was called (%s) for an argument the host must refuse" % name)


@pytest.mark.parametrize("bad", [
    [[1.0, 2.0]],                        # a 2-vector
    [[1.0, 2.0, 3.0, 4.0]],
    5,                                   # not a sequence
    None,
    "5,10,5",                            # a string
    ["abc"],                             # ... also one of length 3
    [[1.0, "2", 3.0]],
    [[1.0, True, 3.0]],
    [1.0, 2.0, 3.0]])                    # one light, not a list of lights
def test_set_lights_refuses_what_is_not_a_list_of_3_vectors(bad):
    r = rt_host.Renderer.__new__(rt_host.Renderer)          # no __init__: no library, no GPU
    r.lib, r.handle = _NoLibrary(), None
    with pytest.raises(ValueError):
        r.set_lights(bad)
    with pytest.raises(ValueError):
        rt_host.light_positions(bad)


def test_set_lights_and_intensity_check_their_other_arguments():
    r = rt_host.Renderer.__new__(rt_host.Renderer)
    r.lib, r.handle = _NoLibrary(), None
    for first in (-1, 1.0, True, None):
        with pytest.raises(ValueError):
            r.set_lights([[1.0, 2.0, 3.0]], first)
    for value in ("50", None, True, [50.0]):
        with pytest.raises(ValueError):
            r.set_light_intensity(value)
    assert rt_host.light_positions([[1, 2, 3], (4.5, 5, 6)]) == [1.0, 2.0, 3.0, 4.5, 5.0, 6.0]
    assert rt_host.light_positions([]) == []


@pytest.mark.parametrize("name", ["h8", "default14_stars", "lcg64", "cfg1"])
def test_python_flattener_keeps_lights_and_intensity_in_place(name):
    s0 = rt_host.load_scene(name)
    b0 = rt_host.flatten_scene(s0)
    off = lights_offset(b0)
    assert off == rt_host.HEADER_BYTES + len(s0["objects"]) * rt_host.SPHERE_BYTES
    assert blob_lights(b0) == [[float(c) for c in l] for l in s0["lights"]]
    assert blob_intensity(b0) == float(s0.get("light_intensity", 50))
    s1 = move_lights(s0, 5, swap=True)
    s1["light_intensity"] = 31.5
    b1 = rt_host.flatten_scene(s1)
    n = len(s0["lights"])
    for k in range(n):
        assert struct.unpack_from("<3d", b1, off + 24 * k) == tuple(s1["lights"][k]), (name, k)
    assert blob_intensity(b1) == 31.5
    # nothing else of the blob moves: what scene_for's carve-outs rest on
    assert b1[:INTENSITY_OFFSET] == b0[:INTENSITY_OFFSET] and b1[INTENSITY_OFFSET + 8:off] == b0[INTENSITY_OFFSET + 8:off]
    assert b1[off + 24 * n:] == b0[off + 24 * n:]
    assert b1[off:off + 24 * n] != b0[off:off + 24 * n]


@needs_node
@pytest.mark.parametrize("name", ["h8", "default14_stars", "lcg64"])
def test_js_flattener_writes_a_moved_light_into_the_same_bytes(name, tmp_path):
    s1 = move_lights(rt_host.load_scene(name), 6, swap=True)
    s1["light_intensity"] = 12.25
    js = """
const fs = require('fs'), path = require('path');
const F = require(%r);
const sc = F.sceneFromJSON(fs.readFileSync(%r, 'utf8'), path.dirname(%r));
fs.writeFileSync(%r, Buffer.from(F.flattenScene(sc)));
const lights = %s;
lights.forEach((l, k) => { sc.lights[k] = l; });            // what a page does between two redraws
sc.light_intensity = %s;
fs.writeFileSync(%r, Buffer.from(F.flattenScene(sc)));
""" % (os.path.join(PKG, "js", "flatten.js"), ou.scene_json(name), ou.scene_json(name), str(tmp_path / "b0"),
       json.dumps(s1["lights"]), json.dumps(s1["light_intensity"]), str(tmp_path / "b1"))
    subprocess.run([ou.node_path(), "-e", js], check=True, timeout=120)
    b0, b1 = (tmp_path / "b0").read_bytes(), (tmp_path / "b1").read_bytes()
    assert b0 == rt_host.flatten_scene(rt_host.load_scene(name))
    assert b1 == rt_host.flatten_scene(s1)
    off = lights_offset(b1)
    for k, l in enumerate(s1["lights"]):
        assert struct.unpack_from("<3d", b1, off + 24 * k) == tuple(l), (name, k)
    assert struct.unpack_from("<d", b1, INTENSITY_OFFSET)[0] == 12.25


def _notes(obj, tmp_path):
    fat, co = tmp_path / "o.bin", tmp_path / "o.co"
    subprocess.run([TOOLS[0], "--dump-section", ".hip_fatbin=%s" % fat, obj], check=True)
    subprocess.run([TOOLS[1], "--unbundle", "--type=o", "--input=%s" % fat,
                    "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", "--output=%s" % co], check=True)
    text = subprocess.run([TOOLS[2], "--notes", str(co)], check=True, capture_output=True, text=True).stdout
    kernels = {}
    for block in re.split(r"\n\s+- \.agpr_count:", text)[1:]:
        f = dict(re.findall(r"\.(name|vgpr_count|vgpr_spill_count|sgpr_spill_count|private_segment_fixed_size):\s+(\S+)", block))
        kernels[f["name"]] = {k: int(v) for k, v in f.items() if k != "name"}
    return kernels


@pytest.mark.skipif(not all(os.path.exists(t) for t in TOOLS), reason="ROCm LLVM tools not installed")
def test_light_move_kernels_do_not_spill_or_use_scratch(built, tmp_path):
    """The light list travels by value in the kernarg segment and is indexed by the workgroup: it must be read from there, not copied
    into private memory."""
    obj = os.path.join(CSRC, "rt_objects_gpu.o")
    k = _notes(obj, tmp_path)
    names = {n for n in k if re.search(r"rt_(light_anchor|sgrid_build)", n)}
    assert len(names) == 2, sorted(k)
    for n in names:
        r = k[n]
        assert r["vgpr_spill_count"] == 0 and r["sgpr_spill_count"] == 0 and r["private_segment_fixed_size"] == 0, (n, r)
