"""Numpy restatements of the four camera models of a view (include/rt_hip.h: rt_view), written from the header's table and not from
csrc/rt_views.h: every operation in binary64, in the order the header states, so that the comparison with the library is bitwise.
The panorama's tables are arguments ({sin, cos} interleaved, as the library takes them)."""
import math

import numpy as np

REFERENCE, PINHOLE, ORTHO, EQUIRECT = 0, 1, 2, 3
SIZES = [(1, 1), (3, 5), (256, 2), (257, 3), (700, 9)]        # 3x5: X == 0 and Y == 0 occur; 256 / 257: one workgroup and one lane more
BAND = (700, 9, 4, 3)                                         # w, h, first_row, rows
# the oblique camera of tests/test_gpu_parity.py: every axis has x, y and z parts
OBLIQUE = ([6.0, 3.0, 8.0], [0.0, 1.0, 0.0], [0.0, 1.0, 0.0])


def unit_rows(d):
    """normal3D per row: v * (1 / sqrt(x x + y y + z z)), a zero vector left as it is."""
    x, y, z = d[..., 0], d[..., 1], d[..., 2]
    l = np.sqrt(x * x + y * y + z * z)
    with np.errstate(divide="ignore"):
        k = np.where(l != 0.0, 1.0 / l, 1.0)
    return np.where((l != 0.0)[..., None], d * k[..., None], d)


def proj_d(fov_deg, w):
    proj_a = fov_deg * math.pi / 180.0
    return (w / 2.0) / math.tan(proj_a / 2.0)


def tables_numpy(w, h):
    """The panorama's tables with numpy's own sin / cos (tools/panorama.py's expressions)."""
    lon = 2.0 * np.pi * (np.arange(w) + 0.5) / w - np.pi
    lat = np.pi / 2.0 - np.pi * (np.arange(h) + 0.5) / h
    return np.stack([np.sin(lon), np.cos(lon)], 1).reshape(-1), np.stack([np.sin(lat), np.cos(lat)], 1).reshape(-1)


def rays(model, w, h, o, ax, ay, az, fov_deg=60.0, scale=1.0, lon=None, lat=None, first_row=0, rows=None):
    """-> (rows * w, 6) float64 {org, dir}, rows [first_row, first_row + rows) of the view in row order."""
    rows = h - first_row if rows is None else rows
    o, ax, ay, az = (np.array(v, np.float64) for v in (o, ax, ay, az))
    xs = np.arange(w, dtype=np.float64)
    ys = np.arange(first_row, first_row + rows, dtype=np.float64)
    X = np.broadcast_to(((xs - w / 2.0) + 0.5)[None, :], (rows, w))
    Y = np.broadcast_to(((h / 2.0 - ys) - 0.5)[:, None], (rows, w))
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


def look_at(org, tgt, up):
    """main.js:92-100 -> origin, axisX, axisY, axisZ (lists)."""
    org, tgt, up = (np.array(v, np.float64) for v in (org, tgt, up))
    cross = lambda a, b: np.array([a[1] * b[2] - b[1] * a[2], a[2] * b[0] - b[2] * a[0], a[0] * b[1] - b[0] * a[1]])
    z = tgt - org
    x = cross(up, z)
    y = cross(z, x)
    return org.tolist(), unit_rows(x).tolist(), unit_rows(y).tolist(), unit_rows(z).tolist()


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)
