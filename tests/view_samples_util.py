"""Numpy restatements of a sampled view (include/rt_hip.h: rt_view_sample, rt_view_lens), written from the header's block and not from
csrc/rt_view_samples.h: every operation in binary64, in the order the header states, so that the comparison with the library is
bitwise.  A sample is (dx, dy, lu, lv); a lens (radius, focus) or None.  The panorama's tables are arguments: the SAMPLE's own table."""
import math

import numpy as np

from views_util import EQUIRECT, ORTHO, PINHOLE, REFERENCE, proj_d, unit_rows

ZERO = (0.0, 0.0, 0.0, 0.0)
ARBITRARY = (0.25, -0.375, 0.5, -0.25)
LENS = (0.07, 6.5)
SIZES = [(5, 3), (257, 2)]


def grid(k):
    """The k x k pattern's dx, dy as the header states them: [(dx, dy)] for sample j k + i."""
    return [((i + 0.5) / k - 0.5, (j + 0.5) / k - 0.5) for j in range(k) for i in range(k)]


def sample_tables(w, h, samples):
    """The panorama's tables of the samples with Python's own sin / cos (the host's libm) on the header's angle expressions."""
    lon, lat = [], []
    for dx, dy, _, _ in samples:
        lon += [f(2.0 * math.pi * ((x + 0.5) + dx) / w - math.pi) for x in range(w) for f in (math.sin, math.cos)]
        lat += [f(math.pi / 2.0 - math.pi * ((y + 0.5) + dy) / h) for y in range(h) for f in (math.sin, math.cos)]
    return np.array(lon, np.float64), np.array(lat, np.float64)


def rays(model, w, h, o, ax, ay, az, sample, lens=None, fov_deg=60.0, scale=1.0, lon=None, lat=None, first_row=0, rows=None):
    """-> (rows * w, 6) float64 {org, dir}: rows [first_row, first_row + rows) of the sample's rays in row order."""
    rows = h - first_row if rows is None else rows
    dx, dy, lu, lv = sample
    o, ax, ay, az = (np.array(v, np.float64) for v in (o, ax, ay, az))
    xs = np.arange(w, dtype=np.float64)
    ys = np.arange(first_row, first_row + rows, dtype=np.float64)
    X = np.broadcast_to((((xs - w / 2.0) + 0.5) + dx)[None, :], (rows, w))
    Y = np.broadcast_to((((h / 2.0 - ys) - 0.5) - dy)[:, None], (rows, w))
    out = np.empty((rows, w, 6), np.float64)
    out[..., 0:3] = o
    if model == REFERENCE:
        d = (X, Y, np.full((rows, w), proj_d(fov_deg, w)))
        for c in range(3):
            target = ((o[c] + ax[c] * d[c]) + ay[c] * d[c]) + az[c] * d[c]
            out[..., 3 + c] = target - o[c]
    elif model == PINHOLE:
        pd = proj_d(fov_deg, w)
        for c in range(3):
            out[..., 3 + c] = (ax[c] * X + ay[c] * Y) + az[c] * pd
        if lens is not None and lens[0] > 0.0:
            radius, focus = lens
            f = focus / pd
            lx, ly = lu * radius, lv * radius
            for c in range(3):
                off = ax[c] * lx + ay[c] * ly
                out[..., c] = o[c] + off
                out[..., 3 + c] = out[..., 3 + c] * f - off
    elif model == ORTHO:
        sx, sy = X * scale, Y * scale
        for c in range(3):
            out[..., c] = (o[c] + ax[c] * sx) + ay[c] * sy
            out[..., 3 + c] = az[c]
    else:
        sl, cl = (np.broadcast_to(np.asarray(lon, np.float64)[k::2][None, :], (rows, w)) for k in (0, 1))
        sa, ca = (np.broadcast_to(np.asarray(lat, np.float64)[k::2][first_row:first_row + rows, None], (rows, w)) for k in (0, 1))
        l0, l1, l2 = ca * sl, sa, ca * cl
        for c in range(3):
            out[..., 3 + c] = (ax[c] * l0 + ay[c] * l1) + az[c] * l2
    out[..., 3:] = unit_rows(out[..., 3:])
    return out.reshape(rows * w, 6)


def fold(rgbs):
    """The stated mean of n samples' rgb arrays: acc = r0; acc = acc + rs in order; acc / n."""
    acc = np.array(rgbs[0], np.float64)
    for r in rgbs[1:]:
        acc = acc + r
    return acc / float(len(rgbs))
