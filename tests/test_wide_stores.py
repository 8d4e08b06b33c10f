"""The 16-byte frame stores of the product trace kernels, without a GPU (csrc/rt_wide.h, rt_device.h: rt_wide_stores_of).

The kernel's epilogue stores through addresses it works out by hand, so before any of it runs on a GPU every store of every launch
shape that tests/test_gpu_wide_stores.py renders is enumerated here - from the launch table as the host builds it
(rt_scene_launch_table) and the header the epilogue is written from (the test build's probe rt_test_wide_stores) - and held to:
16-byte aligned, inside [out, out + frames x stride), and together covering every pixel of the call's band exactly once and
nothing else.  The host rule that admits a launch is tested the way tests/test_variants.py tests the variant rules; the header's
stand-alone check program is built with -fsanitize=address,undefined and run once, on its own."""
import ctypes as C
import itertools
import os
import shutil
import subprocess

import numpy as np
import pytest

import rt_host

CSRC = os.path.join(os.path.dirname(os.path.abspath(rt_host.__file__)), "csrc")
TABLE_FLAGS = 1 | 2 | 4                      # ranked, sky blocks marked, candidates: a product frame's words 0 and 1
WIDE, THROUGH_SKY, THROUGH_TRACED = 1, 2, 4  # rt_device.h: RT_WIDE_*
MAX_BYTES = 64 << 20                         # rt_device.h: RT_WIDE_MAX_BYTES - a launch that writes more takes the 16-byte stores plain
WIDE_WIDTHS = (4, 8, 28, 32, 36, 60, 64, 68, 132, 640)
FALLBACK_WIDTHS = (33, 63, 65, 1001)
HEIGHTS = (1, 7, 8, 9, 17)
SCENES = ("h8", "h8_ss2", "lcg64_ss1", "default14")


def scene_of(name):
    s = rt_host.load_scene("h8" if name == "h8_ss2" else name)
    s["supersample"] = 2 if name == "h8_ss2" else 1
    return s


@pytest.fixture(scope="module")
def lib(built):
    lib = rt_host.load_library(rt_host.TEST_LIB_PATH)
    lib.rt_test_wide_rule.restype = C.c_int
    lib.rt_test_wide_rule.argtypes = [C.c_uint32, C.c_uint32, C.c_uint64, C.c_uint32, C.c_uint64, C.c_uint64, C.POINTER(C.c_uint32)]
    lib.rt_test_wide_stores.restype = C.c_int
    lib.rt_test_wide_stores.argtypes = [C.c_uint32, C.c_uint32, C.c_int, C.c_uint32, C.POINTER(C.c_uint32), C.c_uint32, C.POINTER(C.c_uint32)]
    return lib


def entries(lib, blob, w, h, tiles):
    """The launch table's entries (words 0..3) of `tiles` of the w x h frame, empty slots left out."""
    t = rt_host.RtTiles(*tiles)
    buf = C.create_string_buffer(blob, len(blob))
    n, nb = C.c_uint32(), C.c_uint32()
    assert lib.rt_scene_launch_table(buf, len(blob), w, h, C.byref(t), TABLE_FLAGS, None, C.byref(n), C.byref(nb)) == 0, lib.rt_last_error()
    out = (C.c_uint32 * (4 * 8 * ((nb.value + 7) // 8)))()
    assert lib.rt_scene_launch_table(buf, len(blob), w, h, C.byref(t), TABLE_FLAGS, out, C.byref(n), C.byref(nb)) == 0, lib.rt_last_error()
    tab = np.frombuffer(out, dtype=np.uint32).reshape(-1, 4)
    tab = tab[((tab[:, 0] >> 11) & 15) != 0]                  # (an entry without rows - a tile's row block past the frame - stores nothing: its workgroup leaves at once)
    assert 0 < len(tab) <= n.value
    return tab


def sky_runs(tab):
    return sorted({((int(e1) >> 24) & 127) + 1 for _, e1, _, _ in tab if int(e1) >> 31})


def stores_of(lib, tab, ss2, w):
    """Every store of the launch: rows of (wave, row in the band, first pixel)."""
    cap = 128 * 64
    buf, n = (C.c_uint32 * (3 * cap))(), C.c_uint32()
    out = []
    for e0, e1, _, _ in tab:
        assert lib.rt_test_wide_stores(int(e0), int(e1), int(ss2), w, buf, cap, C.byref(n)) == 0, lib.rt_last_error()
        assert n.value <= cap
        got = np.frombuffer(buf, dtype=np.uint32)[:3 * n.value].reshape(-1, 3).copy()
        if int(e1) >> 31:                                     # a sky run: block t of the run is wave t % 4's
            px0 = (int(e0) & 2047) * 32
            assert ((got[:, 2] - px0) // 32 % 4 == got[:, 0]).all()
        out.append(got)
    return np.concatenate(out) if out else np.zeros((0, 3), np.uint32)


def check_launch(lib, scene_name, w, h, tiles=None, out_address=0x7f0000000000, n_frames=1, stride_words=None):
    """Enumerate one launch's stores and hold them to the statement of the module docstring.  Returns the sky run lengths."""
    scene = scene_of(scene_name)
    tiles = tiles or (h, 0, 1, 1)
    band_rows = tiles[3] * tiles[0]
    stride_words = stride_words if stride_words is not None else band_rows * w
    flags = C.c_uint32()
    assert lib.rt_test_wide_rule(0, w, out_address, n_frames, stride_words, n_frames * band_rows * w * 4, C.byref(flags)) == 0
    assert flags.value & WIDE, "the launch is expected to take the 16-byte stores"
    tab = entries(lib, rt_host.flatten_scene(scene), w, h, tiles)
    st = stores_of(lib, tab, scene["supersample"] == 2, w).astype(np.int64)
    # rows of the band the frame really has: a tile's rows past the frame's last row are no pixels of the call
    valid = np.zeros((band_rows, w), bool)
    for i in range(tiles[3]):
        r0 = (tiles[1] + i * tiles[2]) * tiles[0]
        valid[i * tiles[0]: i * tiles[0] + max(0, min(tiles[0], h - r0))] = True
    hits = np.zeros((band_rows, w), np.int32)
    assert (st[:, 2] % 4 == 0).all() and (st[:, 2] + 4 <= w).all() and (st[:, 1] < band_rows).all()
    for k in range(4):
        np.add.at(hits, (st[:, 1], st[:, 2] + k), 1)
    assert (hits[valid] == 1).all() and (hits[~valid] == 0).all(), "every valid pixel exactly once, and nothing else"
    for f in range(n_frames):
        addr = out_address + 4 * (f * stride_words + st[:, 1] * w + st[:, 2])
        assert (addr % 16 == 0).all()
        assert (addr >= out_address).all() and (addr + 16 <= out_address + 4 * n_frames * stride_words).all()
    return sky_runs(tab)


@pytest.mark.parametrize("scene", SCENES)
@pytest.mark.parametrize("w", WIDE_WIDTHS)
def test_every_store_of_a_whole_frame(lib, scene, w):
    for h in HEIGHTS:
        check_launch(lib, scene, w, h)


def test_640_has_sky_runs_of_every_wave_residue_and_two_turns_of_the_stride(lib):
    """At 640 a row has 20 blocks.  The run lengths are read off the host table: over the scenes and heights of this file the runs of 1
    to 5 blocks (every wave residue) and one of 8 or more (the t += 4 stride turns twice) all occur - in lcg64_ss1's frames; the strips
    of h8 and default14 this low show sky in runs of 5 only."""
    runs = {s: set() for s in SCENES}
    for s in SCENES:
        for h in HEIGHTS:
            runs[s] |= set(check_launch(lib, s, 640, h))
    every = set().union(*runs.values())
    assert {1, 2, 3, 4, 5} <= every and max(every) >= 8, runs


@pytest.mark.parametrize("rank", [0, 1])
def test_interleaved_tiles_of_two_ranks(lib, rank):
    w, h = 640, 72                           # 16-row tiles: four and a half of them, dealt to two ranks
    n_tiles = (-(-h // 16) - rank + 1) // 2
    for scene in ("h8", "h8_ss2"):
        check_launch(lib, scene, w, h, tiles=(16, rank, 2, n_tiles))


def test_batch_with_a_stride_and_an_offset_output(lib):
    w, h = 132, 17
    check_launch(lib, "h8", w, h, n_frames=2, stride_words=w * h + 4 * 5)
    check_launch(lib, "h8", w, h, out_address=0x7f0000000010)


def test_the_rule(lib):
    """rt_wide_stores_of against its statement written out by hand, over every combination of facts."""
    def ask(facts, w, addr, n_frames, stride, out_bytes):
        f = C.c_uint32(0xffffffff)
        assert lib.rt_test_wide_rule(facts, w, addr, n_frames, stride, out_bytes, C.byref(f)) == 0
        return f.value
    seen = set()
    sizes = (16, 3840 * 2160 * 4, MAX_BYTES, MAX_BYTES + 1, 7680 * 4320 * 4, 1 << 32)
    for facts, w, off, n_frames, pad, size in itertools.product(range(8), WIDE_WIDTHS + FALLBACK_WIDTHS, (0, 4, 8, 12, 16, 256), (1, 2, 3), (0, 1, 2, 3, 4), sizes):
        stride = w * 17 + pad
        ok = facts == 0 and w % 4 == 0 and off % 16 == 0 and (n_frames == 1 or stride % 4 == 0)
        through = (THROUGH_SKY | THROUGH_TRACED) if size <= MAX_BYTES else 0
        got = ask(facts, w, 0x7f0000000000 + off, n_frames, stride, size)
        assert got == ((WIDE | through) if ok else 0), (facts, w, off, n_frames, stride, size)
        seen.add(got)
    assert seen == {0, WIDE, WIDE | THROUGH_SKY | THROUGH_TRACED}
    assert lib.rt_test_wide_rule(0, 4, 0, 1, 4, 16, None) != 0


def test_the_headers_check_program_under_sanitizers(tmp_path):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++") or "/opt/rocm/llvm/bin/clang++"
    exe = str(tmp_path / "rt_wide_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    os.path.join(CSRC, "rt_wide_check.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0 and r.stdout.startswith("ok "), r.stdout[-2000:]
