"""Checker statements of the launch table on RANDOM scenes (csrc/rt_block.h: rt_column_cell, rt_cells_word; CPU only, the host build).

test_checker_cells.py and test_checker_axes.py probe the statements on h8 and what is derived from it.  Here the scenes are the GPU
soaks' own (tests/soak_gpu_parity.py: draw_scene - checker spheres of any radius, position and frequency, a ground or none, cameras
anywhere, also inside a sphere and with arbitrary axes, every field of view, supersample 1 and 2), at the size drawn and at four times
that size (more waves fit into one cell).  For every whole-cell wave and every per-axis column of the host table the C restatement's
per-sample probe (oracle/rt_oracle.c) must put all samples on ONE sphere, met from outside, whose sampler is the checker; the stated
coordinates inside one unit cell, 2^-18 clear of its ends, with the stated parity - and for a whole cell the oracle's own colour."""
import ctypes as C
import math

import numpy as np
import pytest

import oracle_util as ou
import rt_host
import test_checker_axes as ta
import test_checker_cells as tc
from soak_gpu_parity import draw_scene
from test_checker_cells import lib  # noqa: F401  (the module's fixture)

MARGIN = 2.0 ** -18
SEEDS = range(900000, 900070)        # (with 240 seeds: 103 539 whole-cell waves and 81 557 per-axis columns, all held; 70 keep the test to half a minute)


def probe_block(c, buf, nbytes, w, h, ss, tile_x, frow0, col, rec):
    cw, ch = (16, 4) if ss == 2 else (8, 8)
    x0, y0 = (tile_x * 32 + col * 8) * ss, frow0 * ss
    rows = []
    for sy in range(y0, y0 + ch):
        for sx in range(x0, min(x0 + cw, w * ss)):
            assert c.oracle_probe_sample(buf, nbytes, w, h, sx, sy, rec.ctypes.data) == 0
            rows.append(rec[:tc.PROBE_WORDS].copy())
    return np.array(rows) if rows else None


def coords(q, smp):
    n = q[:, 6:9]
    xu = (np.arctan2(-n[:, 1], -n[:, 0]) / math.pi / 2 + 0.5) * smp["freqU"]
    xv = (np.arcsin(-n[:, 2]) / (math.pi / 2) / 2 + 0.5) * smp["freqV"]
    return xu, xv


def one_cell(x, where):
    k = np.floor(x)
    assert (k == k[0]).all(), where
    assert (x - k >= MARGIN).all() and (k + 1 - x >= MARGIN).all(), where
    return int(k[0])


def check_scene(lib, scene, w, h, seed):
    """Returns (whole-cell waves, per-axis columns) probed."""
    blob = rt_host.flatten_scene(scene)
    ss = scene["supersample"]
    axes = tc.table(lib, blob, w, h, ta.AXES)
    assert (ta.whole_cells(axes) == tc.table(lib, blob, w, h, tc.CELLS)).all(), seed
    whole, cols = tc.flagged_waves(ta.whole_cells(axes)), ta.axis_columns(axes)
    if not whole and not cols:
        return 0, 0
    c = ou.c_oracle()
    c.oracle_probe_sample.restype = C.c_int
    c.oracle_probe_sample.argtypes = [C.c_void_p, C.c_size_t, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p]
    # the probe records a node after its children and keeps 64 nodes: it reads the scene at depth 1, where the primary hit is the one
    # record (hit, normal and sampler colour do not depend on the depth, nor does the table's statement)
    blob = rt_host.flatten_scene(dict(scene, segs=1))
    buf = C.create_string_buffer(blob, len(blob))
    rec = np.zeros(tc.PROBE_NODES * tc.PROBE_WORDS)

    def sampler_of(q, where):
        # every sample's primary hit: ONE sphere (the probe's id is twice its scene index), from outside, a checker sphere
        assert (q[:, 23] == 1.0).all() and (q[:, 1] == q[0, 1]).all() and int(q[0, 1]) % 2 == 0, where
        smp = scene["objects"][int(q[0, 1]) // 2]["mtl"]["sampler"]
        assert smp["kind"] == 2, where
        return smp

    for tile_x, frow0, col, parity, _ in whole:
        q = probe_block(c, buf, len(blob), w, h, ss, tile_x, frow0, col, rec)
        if q is None:
            continue
        where = (seed, w, h, "whole", tile_x, frow0, col, parity)
        smp = sampler_of(q, where)
        xu, xv = coords(q, smp)
        assert (one_cell(xu, where) ^ one_cell(xv, where)) & 1 == parity, where
        assert (q[:, 12:15] == np.array(smp["colors"][parity], dtype=np.float64)).all(), where
    for tile_x, frow0, col, axis, parity, _ in cols:
        q = probe_block(c, buf, len(blob), w, h, ss, tile_x, frow0, col, rec)
        if q is None:
            continue
        where = (seed, w, h, "axis", tile_x, frow0, col, axis, parity)
        x = coords(q, sampler_of(q, where))[axis]
        assert one_cell(x, where) & 1 == parity, where
    return len(whole), len(cols)


@pytest.mark.parametrize("many", [False, True])
def test_random_scenes(lib, many):
    """Not vacuous: the draws must yield statements of both kinds (the counts are printed)."""
    whole = cols = 0
    for seed in SEEDS:
        scene, w, h = draw_scene(seed, False, many)
        for k in (1, 4):
            a, b = check_scene(lib, scene, k * w, k * h, seed)
            whole, cols = whole + a, cols + b
    print("random scenes%s: %d whole-cell waves, %d per-axis columns probed" % (" (many spheres)" if many else "", whole, cols))
    assert whole > 0 and cols > 0, (whole, cols)
