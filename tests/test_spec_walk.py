"""The specular power's multiply sequence (csrc/rt_spec_walk.h) on a CPU: tests/host/spec_walk_check.cpp compiles the header the kernels
compile and holds every form of the walk - the gap form, the ladder of the few-sphere one-wave kernels (at the kernels' length and at
lengths that make exponents of the range run its loop), the per-lane form - to the documented loop
    r = 1.0; do { if (k & 1) r *= b; b *= b; k >>= 1; } while (k);
bit for bit, for every exponent 0..4096 and 2 000 bases in (0, 1], denormal results included, and counts the multiplies of the gap and
ladder forms (no 1.0 * b, no squaring behind the top bit).  Built twice where the host compiler has the runtimes: plainly, and with
-fsanitize=address,undefined.  No GPU is needed.
The program also holds the one integer form of a floating-point predicate the kernels use on a scalar double (csrc/rt_uniform_pred.h:
rt_nonzero_bits for `x != 0.0`) to that statement over the edge patterns - +-0, denormals, 1, infinities, quiet and signalling NaNs, negative
values - and 100 000 random ones."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "html5-canvas-raytracer_amd", "csrc")
CXX = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("c++") or shutil.which("clang++")
SANITIZE = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"]


def build(tmp_path, name, extra):
    exe = str(tmp_path / name)
    cmd = [CXX, "-std=c++17", "-O2", "-Wall", "-ffp-contract=off", "-I" + CSRC] + extra + [os.path.join(HERE, "host", "spec_walk_check.cpp"), "-o", exe]
    return exe, subprocess.run(cmd, capture_output=True, text=True)


def run(exe):
    r = subprocess.run([exe], capture_output=True, text=True)
    print(r.stdout + r.stderr)
    assert r.returncode == 0, r.stdout + r.stderr


@pytest.mark.skipif(CXX is None, reason="no host C++ compiler")
def test_every_form_of_the_walk_is_the_documented_loop(tmp_path):
    exe, made = build(tmp_path, "spec_walk_check", [])
    assert made.returncode == 0, made.stderr
    run(exe)


@pytest.mark.skipif(CXX is None, reason="no host C++ compiler")
def test_the_walk_under_the_address_and_undefined_behaviour_sanitizers(tmp_path):
    """the program has its own main: the sanitizers' runtimes are linked into it"""
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    has = subprocess.run([CXX] + SANITIZE + [str(probe), "-o", str(tmp_path / "probe")], capture_output=True, text=True)
    if has.returncode != 0:
        pytest.skip("the host compiler has no sanitizer runtimes")
    exe, made = build(tmp_path, "spec_walk_check_san", SANITIZE)
    assert made.returncode == 0, made.stderr
    run(exe)
