"""Per-axis checker statements of the launch table (csrc/rt_block.h: rt_column_cell, rt_cells_word; CPU only, the host build of the table).

With bit 6 of rt_scene_launch_table's `ranked` (beside bit 5, the checker cells) word 3 of a one-candidate block also says, for a
column that does NOT lie inside one checker cell, that ONE of the checker's two coordinates - u f_u or v f_v, bit 30 says which for the
whole entry - lies inside one unit cell for every sample of the column (bit 26 + c), and that cell's index & 1 (bit 22 + c, the parity
slot such a column does not use).  The kernel's wave then works out only the other coordinate, so the statement has to be
conservative: for every such column the C restatement of the reference (oracle/rt_oracle.c, its per-sample probe) must put all the
column's samples on the candidate, from outside, with the stated coordinate inside ONE unit cell, none within 2^-18 of its ends (twice
the kernel's prefilter band), and with the stated parity.  (u, v from the oracle's normal with numpy's atan2 / asin, as in
test_checker_cells.py: an ulp off the oracle's own, five orders below the margin asserted.)"""
import ctypes as C
import math
import os
import sys

import numpy as np
import pytest

import oracle_util as ou
import rt_host
import test_checker_cells as tc
from test_checker_cells import lib  # noqa: F401  (the module's fixture)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
AXES = tc.CELLS | 64
MARGIN = 2.0 ** -18


def axis_columns(tab):
    """(tile_x, first frame row, column, axis (0 u, 1 v), parity, loop index of the candidate) of every column with ONE axis stated."""
    out = []
    for w0, w1, _, w3 in tab:
        cell = int(w3) >> 18
        assert cell < (1 << 13), (w0, w1, w3)
        if not (cell >> 8) & 15:
            assert not cell >> 12, (w0, w1, w3)                # no axis named without a column that states it
            continue
        assert (int(w0) >> 11) & 15 and not int(w1) >> 31 and (int(w3) >> 16) & 3 == 1, (w0, w1, w3)
        assert not (cell >> 8) & cell & 15                     # a column has its whole cell stated, or one axis, never both
        for c in range(4):
            if cell >> (8 + c) & 1:
                out.append((int(w0) & 2047, int(w0) >> 15, c, cell >> 12 & 1, cell >> (4 + c) & 1, int(w3) & 255))
        assert not (cell >> 4) & ~(cell | cell >> 8) & 15     # no parity bit without a statement
    return out


def whole_cells(tab):
    """The table with the per-axis statements taken out: what test_checker_cells.flagged_waves reads."""
    out = tab.copy()
    stated = (out[:, 3] >> 26) & 15
    out[:, 3] &= ~((stated << 22) | (63 << 26)) & 0xffffffff
    return out


def check(lib, scene, w, h, every=1):
    """Every column with an axis statement against the oracle's probe; returns (u-only columns, v-only columns)."""
    blob = rt_host.flatten_scene(scene)
    ss = scene.get("supersample", 1)
    assert ss in (1, 2)
    cols = axis_columns(tc.table(lib, blob, w, h, AXES))
    c = ou.c_oracle()
    c.oracle_probe_sample.restype = C.c_int
    c.oracle_probe_sample.argtypes = [C.c_void_p, C.c_size_t, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p]
    buf = C.create_string_buffer(blob, len(blob))
    rec = np.zeros(tc.PROBE_NODES * tc.PROBE_WORDS)
    order = tc.loop_order(scene)
    cw, ch = (16, 4) if ss == 2 else (8, 8)
    for tile_x, frow0, col, axis, parity, loop_i in cols[::every]:
        smp = scene["objects"][order[loop_i]]["mtl"]["sampler"]
        assert smp["kind"] == 2                                # RT_SAMPLER_CHECKER
        x0, y0 = (tile_x * 32 + col * 8) * ss, frow0 * ss
        rows = []
        for sy in range(y0, y0 + ch):
            for sx in range(x0, min(x0 + cw, w * ss)):
                assert c.oracle_probe_sample(buf, len(blob), w, h, sx, sy, rec.ctypes.data) == 0
                rows.append(rec[:tc.PROBE_WORDS].copy())
        if not rows:
            continue
        q = np.array(rows)
        where = (tile_x, frow0, col, axis, parity)
        assert (q[:, 23] == 1.0).all() and (q[:, 1] == 2 * order[loop_i]).all(), where      # every sample's primary hit: the candidate, from outside
        n = q[:, 6:9]
        if axis == 0:
            x = (np.arctan2(-n[:, 1], -n[:, 0]) / math.pi / 2 + 0.5) * smp["freqU"]
        else:
            x = (np.arcsin(-n[:, 2]) / (math.pi / 2) / 2 + 0.5) * smp["freqV"]
        k = np.floor(x)
        assert (k == k[0]).all(), where
        assert int(k[0]) & 1 == parity, where
        assert (x - k >= MARGIN).all() and (k + 1 - x >= MARGIN).all(), where
    return sum(1 for t in cols if t[3] == 0), sum(1 for t in cols if t[3] == 1)


def test_h8_1280x720_and_not_vacuous(lib):
    """At least 300 u-only and 150 v-only columns: a quarter of what a count over the frame's pixel centres promised (1 210 and 570)."""
    nu, nv = check(lib, tc.h8(), 1280, 720)
    assert nu >= 300 and nv >= 150, (nu, nv)


def test_h8_ragged_size(lib):
    assert sum(check(lib, tc.h8(), 1001, 563)) > 0


def test_h8_supersample_2(lib):
    assert sum(check(lib, tc.h8(supersample=2), 1001, 563)) > 0


def test_h8_moving_camera(lib):
    """Four of the 64 cameras of bench.py's moving-camera leg."""
    sys.path.insert(0, ROOT)
    import bench
    total = 0
    for k in (0, 17, 34, 51):
        s = tc.h8()
        s["camera"] = bench.moving_camera(s, k, 64)
        total += sum(check(lib, s, 1280, 720))
    assert total > 0


@pytest.mark.parametrize("factor", [0.1, 10.0])
def test_scaled_frequencies(lib, factor):
    assert sum(check(lib, tc.scaled(factor), 1280, 720)) > 0


def test_poles_and_branch_cut_on_screen(lib):
    assert sum(check(lib, tc.pole_scene(), 1280, 720)) > 0


def test_out_of_range_frequencies_get_none(lib):
    for f in ((0.0, 2500.0), (5000.0, 0.0), (262144.0, 2500.0)):
        tab = tc.table(lib, rt_host.flatten_scene(tc.scaled(freq=f)), 1280, 720, AXES)
        assert (tab[:, 3] >> 18 == 0).all()


@pytest.mark.parametrize("scene,wh", [("h8", (1280, 720)), ("h8", (1001, 563)), ("h8_ss2", (1001, 563)), ("default14", (1280, 720))])
def test_a_table_without_the_option_is_the_table_with_it_masked(lib, scene, wh):
    """Word for word.  Without the option: the checker-cell table (no bit above 25; a parity bit only beside its flag).  With it: the
    same words, plus bits 26..30 and, for the columns that state an axis, their parity slot 22 + c."""
    s = tc.h8(supersample=2) if scene == "h8_ss2" else rt_host.load_scene(scene)
    if s.get("supersample", 1) > 2:
        s["supersample"] = 1
    blob = rt_host.flatten_scene(s)
    for tiles in (None, (16, 1, 2, (wh[1] // 16) // 2)):
        cells, axes = tc.table(lib, blob, *wh, tc.CELLS, tiles), tc.table(lib, blob, *wh, AXES, tiles)
        assert (cells[:, 3] >> 26 == 0).all()
        assert (whole_cells(axes) == cells).all()
        assert ((axes[:, 3] ^ cells[:, 3]) & (15 << 18) == 0).all()          # bits 18..21 mean "inside one checker cell" with or without the option
