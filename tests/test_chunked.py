"""The chunk driver of the host forms (csrc/rt_chunked.h) on a CPU: tests/host/chunked_check.cpp defines the HIP functions the header
calls as recorders, drives the driver as a list (chunk 4; n = 1, 4, 5, 9) and as a view (w = 3, h = 5; 1 and 2 rows per chunk), and
compares the recorded calls - which rows are allocated and with how many bytes, each copy's direction, host offset and size, the
units each step sees, one stream synchronise per chunk, NULL for a row without a host pointer, every allocation freed once - with the
expected ones written in its source; then it injects a failure at the third hipMalloc, the second chunk's copy-in, a step and the
final synchronise.  Built twice where the host compiler has the runtimes: plainly, and with -fsanitize=address,undefined.  No HIP
runtime is linked and no GPU is needed."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "html5-canvas-raytracer_amd", "csrc")
ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")
CXX = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("c++") or shutil.which("clang++")
SANITIZE = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"]


def build(tmp_path, name, extra):
    exe = str(tmp_path / name)
    cmd = [CXX, "-std=c++17", "-Wall", "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(ROCM, "include"), "-I" + CSRC] + extra + \
          [os.path.join(HERE, "host", "chunked_check.cpp"), "-o", exe]
    return exe, subprocess.run(cmd, capture_output=True, text=True)


def run(exe):
    r = subprocess.run([exe], capture_output=True, text=True)
    print(r.stdout + r.stderr)
    assert r.returncode == 0, r.stderr


@pytest.mark.skipif(CXX is None, reason="no host C++ compiler")
def test_the_driver_makes_the_expected_hip_calls(tmp_path):
    exe, made = build(tmp_path, "chunked_check", [])
    assert made.returncode == 0, made.stderr
    run(exe)


@pytest.mark.skipif(CXX is None, reason="no host C++ compiler")
def test_the_driver_under_the_address_and_undefined_behaviour_sanitizers(tmp_path):
    """the program has its own main: the sanitizers' runtimes are linked into it"""
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    has = subprocess.run([CXX] + SANITIZE + [str(probe), "-o", str(tmp_path / "probe")], capture_output=True, text=True)
    if has.returncode != 0:
        pytest.skip("the host compiler has no sanitizer runtimes")
    exe, made = build(tmp_path, "chunked_check_san", SANITIZE)
    assert made.returncode == 0, made.stderr
    run(exe)
