#!/usr/bin/env python3
"""ORACLE / TEST INFRASTRUCTURE: records what the reference itself renders for the CPU tests that hold the restatements to it
(tests/test_oracle.py), so that those tests need nothing outside the repository.  Runs only where the reference and node are
present (like oracle/make_golden.js):

    python oracle/record_reference_results.py

Writes tests/golden/reference_results.json, data only: the SHA-256 of frames rendered by the reference - its own main(), its
intersectWorld on scenes of our schema at sizes that differ from the golden frames, the random scenes of
tests/soak_oracle_vs_reference.py, and the scenes of tests/texture_util.py that carry sixteen textures of odd shapes (1x1 ... 16384x2).
"""
import json
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "html5-canvas-raytracer_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import oracle_util as ou  # noqa: E402
import soak_oracle_vs_reference as sr  # noqa: E402
import texture_util as tu  # noqa: E402

MAIN_SIZES = [(64, 48)]
SCENES = [("cfg1", 96, 96), ("cfg2", 160, 90), ("h8", 200, 112), ("h8_d8", 120, 68), ("default14", 128, 72), ("lcg64", 48, 48),
          ("lcg64_ss1", 64, 64)]
RANDOM_FIRST, RANDOM_SEEDS = 1000, 10


def main():
    if not ou.have_reference():
        raise SystemExit("record_reference_results.py: the reference (or node) is not here")
    out = {"generator": "oracle/record_reference_results.py", "reference": ou.manifest()["reference"],
           "main": [], "scenes": [], "random_scenes": {"first": RANDOM_FIRST, "frames": []},
           "texture_scenes": []}
    for w, h in MAIN_SIZES:
        out["main"].append({"w": w, "h": h, "sha256": ou.node_cli("main", w, h)["sha256"]})
    for scene, w, h in SCENES:
        out["scenes"].append({"scene": scene, "w": w, "h": h, "sha256": ou.node_cli("reference", ou.scene_json(scene), w, h)["sha256"]})
    with tempfile.TemporaryDirectory() as td:
        p = os.path.join(td, "s.json")
        for seed in range(RANDOM_FIRST, RANDOM_FIRST + RANDOM_SEEDS):
            scene, w, h = sr.scene_without_stars(seed)
            with open(p, "w") as f:
                f.write(sr.to_json(scene))
            out["random_scenes"]["frames"].append({"seed": seed, "w": w, "h": h, "sha256": ou.node_cli("reference", p, w, h)["sha256"]})
        for name, _, _, _ in tu.ORACLE_SCENES:
            scene, w, h = tu.oracle_scene(name)
            with open(p, "w") as f:
                f.write(sr.to_json(scene))
            out["texture_scenes"].append({"scene": name, "w": w, "h": h, "sha256": ou.node_cli("reference", p, w, h)["sha256"]})
    path = os.path.join(ou.GOLDEN, "reference_results.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("wrote %s: %d main(), %d scenes, %d random scenes, %d texture scenes" % (path, len(out["main"]), len(out["scenes"]),
                                                                                len(out["random_scenes"]["frames"]), len(out["texture_scenes"])))


if __name__ == "__main__":
    main()
