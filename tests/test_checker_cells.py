"""Checker cells of the launch table (csrc/rt_block.h: rt_column_cell; CPU only, the host build of the table).

With RT_TABLE_CELLS (bit 5 of rt_scene_launch_table's `ranked`) word 3 of a one-candidate block also says, per 8-pixel column (the 64
samples of one wave of the one-wave trace kernels), that every primary ray meets the candidate inside ONE checker cell, and that cell's
parity.  The kernel then skips the sampler for the wave, so the statement has to be conservative: for every flagged wave the C
restatement of the reference (oracle/rt_oracle.c, its per-sample probe) must put all the wave's samples on the candidate, in the
same cell, with the flagged parity and the flagged cell's colour, and none within 2^-18 of a cell boundary - twice the kernel's
prefilter band (RT_XY_INDEX: a fraction within 2^-20 below or 2^-19 above an integer), outside of which the kernel neither takes the
precise test nor marks a sample.  (u, v are taken from the oracle's normal with numpy's atan2 / asin: they differ from the oracle's
own fdlibm by an ulp, 1e-16 x frequency <= 1e-11 in the coordinate, five orders below the margin asserted.)"""
import copy
import ctypes as C
import math
import os
import sys

import numpy as np
import pytest

import oracle_util as ou
import rt_host

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PLAIN, CELLS = 1 | 2 | 4, 1 | 2 | 4 | 32
FLOOR_R2 = 250000.0
MARGIN = 2.0 ** -18
PROBE_WORDS, PROBE_NODES = 24, 64
H8_4K_FLAGGED = 26638           # docs/EVIDENCE.md (checker cells, step 1): the count this change was decided on


@pytest.fixture(scope="module")
def lib(built):
    return rt_host.load_library()


def table(lib, blob, w, h, flags, tiles=None):
    t = rt_host.RtTiles(*(tiles or (h, 0, 1, 1)))
    buf = C.create_string_buffer(blob, len(blob))
    n, nb = C.c_uint32(), C.c_uint32()
    assert lib.rt_scene_launch_table(buf, len(blob), w, h, C.byref(t), flags, None, C.byref(n), C.byref(nb)) == 0, lib.rt_last_error()
    out = (C.c_uint32 * (4 * 8 * ((nb.value + 7) // 8)))()
    assert lib.rt_scene_launch_table(buf, len(blob), w, h, C.byref(t), flags, out, C.byref(n), C.byref(nb)) == 0, lib.rt_last_error()
    return np.frombuffer(out, dtype=np.uint32).reshape(-1, 4).copy()


def flagged_waves(tab):
    """(tile_x, first frame row, column, parity, loop index of the candidate) of every flagged wave; flags sit on one-candidate entries only."""
    out = []
    for w0, w1, _, w3 in tab:
        cell = int(w3) >> 18
        if not cell & 15:
            continue
        assert (int(w0) >> 11) & 15 and not int(w1) >> 31 and (int(w3) >> 16) & 3 == 1 and cell < 256, (w0, w1, w3)
        for c in range(4):
            if cell >> c & 1:
                out.append((int(w0) & 2047, int(w0) >> 15, c, cell >> (4 + c) & 1, int(w3) & 255))
        assert not (cell >> 4) & ~cell & 15                   # no parity without its flag
    return out


def loop_order(scene):
    """Scene indices in the product kernel's loop order: the enclosing sphere (the skybox, if any) last."""
    idx = list(range(len(scene["objects"])))
    sky = [i for i in idx if scene["objects"][i]["r2"] == 25000000]
    return [i for i in idx if i not in sky] + sky


def check(lib, scene, w, h, every=1):
    """Every flagged wave of the frame (every `every`-th, to bound the time of the largest frames' sweeps) against the oracle's probe."""
    blob = rt_host.flatten_scene(scene)
    ss = scene.get("supersample", 1)
    assert ss in (1, 2)
    flagged = flagged_waves(table(lib, blob, w, h, CELLS))
    c = ou.c_oracle()
    c.oracle_probe_sample.restype = C.c_int
    c.oracle_probe_sample.argtypes = [C.c_void_p, C.c_size_t, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p]
    buf = C.create_string_buffer(blob, len(blob))
    rec = np.zeros(PROBE_NODES * PROBE_WORDS)
    order = loop_order(scene)
    cw, ch = (16, 4) if ss == 2 else (8, 8)                   # a wave's samples
    for tile_x, frow0, col, parity, loop_i in flagged[::every]:
        obj = scene["objects"][order[loop_i]]
        smp = obj["mtl"]["sampler"]
        assert smp["kind"] == 2                                # RT_SAMPLER_CHECKER
        x0, y0 = (tile_x * 32 + col * 8) * ss, frow0 * ss
        rows = []
        for sy in range(y0, y0 + ch):
            for sx in range(x0, min(x0 + cw, w * ss)):         # (samples beyond the frame's right edge are traced by the wave but never stored)
                assert c.oracle_probe_sample(buf, len(blob), w, h, sx, sy, rec.ctypes.data) == 0
                rows.append(rec[:PROBE_WORDS].copy())
        if not rows:
            continue                                          # (a column wholly beyond the right edge)
        q = np.array(rows)
        assert (q[:, 23] == 1.0).all() and (q[:, 1] == 2 * order[loop_i]).all(), (tile_x, frow0, col)     # every sample's primary hit: the candidate, from outside
        n = q[:, 6:9]
        u = np.arctan2(-n[:, 1], -n[:, 0]) / math.pi / 2 + 0.5
        v = np.arcsin(-n[:, 2]) / (math.pi / 2) / 2 + 0.5
        xu, xv = u * smp["freqU"], v * smp["freqV"]
        ku, kv = np.floor(xu), np.floor(xv)
        where = (tile_x, frow0, col, parity)
        assert (ku == ku[0]).all() and (kv == kv[0]).all(), where
        assert (int(ku[0]) ^ int(kv[0])) & 1 == parity, where
        for x, k in ((xu, ku), (xv, kv)):
            assert (x - k >= MARGIN).all() and (k + 1 - x >= MARGIN).all(), where
        assert (q[:, 12:15] == np.array(smp["colors"][parity], dtype=np.float64)).all(), where      # the oracle's own decision
    return len(flagged)


def h8(**kw):
    s = rt_host.load_scene("h8")
    s.update(kw)
    return s


def floor_of(s):
    return next(o for o in s["objects"] if o["r2"] == FLOOR_R2)


def scaled(factor=None, freq=None):
    s = h8()
    smp = floor_of(s)["mtl"]["sampler"]
    if freq is not None:
        smp["freqU"], smp["freqV"] = freq
    else:
        smp["freqU"], smp["freqV"] = smp["freqU"] * factor, smp["freqV"] * factor
    return s


def pole_scene():
    """A checker sphere small enough that a pole (n.z = 1, facing the camera on +z) and the branch cut of atan2 (n.y = 0, n.x > 0) are
    on screen, with cells large enough that whole waves fit into them."""
    s = h8()
    ball = copy.deepcopy(floor_of(s))
    ball["origin"], ball["r2"] = [0, 2.5, 0], 6.25
    ball["mtl"]["sampler"]["freqU"], ball["mtl"]["sampler"]["freqV"] = 8, 4
    s["objects"] = [o for o in s["objects"] if o["r2"] in (FLOOR_R2, 25000000)] + [ball]
    return s


def test_h8_headline_frame(lib):
    """3840x2160: every flagged wave, all 64 samples; and not vacuously - at least the count the change was decided on."""
    n = check(lib, h8(), 3840, 2160)
    assert n >= H8_4K_FLAGGED, n


def test_h8_ragged_size(lib):
    assert check(lib, h8(), 1001, 563) > 0


def test_h8_moving_camera(lib):
    """The 64 cameras of bench.py's moving-camera leg."""
    sys.path.insert(0, ROOT)
    import bench
    total = 0
    for k in range(64):
        s = h8()
        s["camera"] = bench.moving_camera(s, k, 64)
        total += check(lib, s, 1280, 720)
    assert total > 0


def test_h8_supersample_2(lib):
    assert check(lib, h8(supersample=2), 1001, 563) > 0
    assert check(lib, h8(supersample=2), 1920, 1080, every=3) > 0


@pytest.mark.parametrize("factor", [0.1, 10.0])
def test_scaled_frequencies(lib, factor):
    n = check(lib, scaled(factor), 1920, 1080)
    assert n > 0 or factor > 1.0                              # (ten times finer: cells of 6 cm - few waves, if any, fit)


def test_largest_admitted_frequency(lib):
    """2^17 per unit on both axes: cells of millimetres.  Whatever is flagged must hold; nothing needs to be."""
    check(lib, scaled(freq=(131072.0, 131072.0)), 1920, 1080)
    s = scaled(freq=(131072.0, 131072.0))
    s["camera"] = copy.deepcopy(s["camera"])
    s["camera"]["origin"] = [0, 0.002, 10]                    # a camera millimetres above the floor: blocks near the nadir are inside one cell
    check(lib, s, 1920, 1080)


def test_out_of_range_frequencies_get_no_flag(lib):
    for f in ((0.0, 2500.0), (5000.0, 0.0), (262144.0, 2500.0)):
        s = scaled(freq=f)
        assert flagged_waves(table(lib, rt_host.flatten_scene(s), 1920, 1080, CELLS)) == []


def test_poles_and_branch_cut_on_screen(lib):
    assert check(lib, pole_scene(), 1920, 1080) > 0


@pytest.mark.parametrize("scene,wh", [("h8", (3840, 2160)), ("h8", (1001, 563)), ("h8_ss2", (1001, 563)), ("default14", (1280, 720)), ("lcg64_ss1", (1280, 720))])
def test_a_table_without_the_flag_is_todays_table(lib, scene, wh):
    """Word for word: the table built without RT_TABLE_CELLS is the table built with it, word 3's upper bits masked off - and it has none."""
    s = h8(supersample=2) if scene == "h8_ss2" else rt_host.load_scene(scene)
    if s.get("supersample", 1) > 2:
        s["supersample"] = 1
    blob = rt_host.flatten_scene(s)
    for tiles in (None, (16, 1, 2, (wh[1] // 16) // 2)):
        plain, cells = table(lib, blob, *wh, PLAIN, tiles), table(lib, blob, *wh, CELLS, tiles)
        assert (plain[:, 3] >> 18 == 0).all()
        masked = cells.copy()
        masked[:, 3] &= 0x3ffff
        assert (masked == plain).all()
