"""The stream-ordering rules of a resident scene (csrc/rt_scene_sync.h: R1-R6) on a CPU: tests/host/scene_sync_check.cpp defines the
HIP functions the header calls as recorders, drives a scene_sync through launches, moves and texel edits on one and two streams, and
compares the recorded calls - which event is recorded on which stream, which stream waits for which event, when the device is drained,
when a ring slot waits for its previous use, that everything made is destroyed once - with the expected ones written in its source.
No HIP runtime is linked and no GPU is needed."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "html5-canvas-raytracer_amd", "csrc")
ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")
CXX = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("c++") or shutil.which("clang++")


@pytest.mark.skipif(CXX is None, reason="no host C++ compiler")
def test_the_ordering_rules_make_the_expected_hip_calls(tmp_path):
    exe = str(tmp_path / "scene_sync_check")
    subprocess.run([CXX, "-std=c++17", "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(ROCM, "include"), "-I" + CSRC,
                    os.path.join(HERE, "host", "scene_sync_check.cpp"), "-o", exe], check=True)
    run = subprocess.run([exe], capture_output=True, text=True)
    print(run.stdout + run.stderr)
    assert run.returncode == 0, run.stderr
