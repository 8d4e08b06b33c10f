"""Numpy restatements of ambient occlusion (include/rt_hip.h: struct rt_ambient), written from the header's block and not from
csrc/rt_ambient.h: the segments of one sample of a list of receivers, the fold of the per-scan results of rt_host.occlusion into open,
intensity and rgba, and the receivers the GPU tests share.  numpy's float64 + - * / and sqrt are IEEE operations without contraction, so
what comes out here is compared with the library bit for bit."""
import numpy as np

import rt_host

HIT = np.dtype(rt_host.HIT_FIELDS)


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64) if a.dtype == np.float64 else a.view(np.uint8)


def entry(base, i, stride, s, n_dirs):
    """e = ((base + i) * stride + s) % n_dirs in unsigned 64-bit arithmetic, wrapping at 2^64 (Python integers, masked)."""
    m = (1 << 64) - 1
    return ((((base + i) & m) * stride & m) + s & m) % n_dirs


def scanned(hits):
    finite = np.isfinite(hits["point"]).all(axis=1) & np.isfinite(hits["normal"]).all(axis=1)
    return (hits["object"] >= 0) & finite


def segments(hits, dirs, sample, stride=1, base=0):
    """-> (rays (n, 6), skip (n,) int32) of sample `sample`: the header's expressions, one numpy operation per operation."""
    n = len(hits)
    dirs = np.asarray(dirs, np.float64)
    ok = scanned(hits)
    ins = (hits["inside"] != 0)[:, None]
    l = np.where(ins, -hits["normal"], hits["normal"])
    l0, l1, l2 = l[:, 0], l[:, 1], l[:, 2]
    with np.errstate(all="ignore"):
        sg = np.copysign(1.0, l2)
        a = -1.0 / (sg + l2)
        b = (l0 * l1) * a
        t = np.stack([1.0 + (sg * (l0 * l0)) * a, sg * b, -sg * l0], axis=1)
        bt = np.stack([b, sg + (l1 * l1) * a, -l1], axis=1)
        e = np.array([entry(base, i, stride, sample, len(dirs)) for i in range(n)], np.int64)
        d = dirs[e]
        d0, d1, d2 = d[:, 0:1], d[:, 1:2], d[:, 2:3]
        v = (t * d0 + bt * d1) + l * d2
        length = np.sqrt((v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + v[:, 2] * v[:, 2])          # normal3D (main.js:62-66)
        k = np.where(length != 0.0, 1.0 / length, 1.0)
        v = np.where((length != 0.0)[:, None], v * k[:, None], v)
    rays = np.full((n, 6), np.nan)
    rays[ok, 0:3] = hits["point"][ok]
    rays[ok, 3:6] = v[ok]
    return rays, np.where(ok, hits["object"], -1).astype(np.int32)


def to_byte(c):
    """The store rule of main.js:195-198 for a channel in [0, 1]: 255 c, clamped, rounded half to even."""
    return np.rint(np.clip(255.0 * c, 0.0, 255.0)).astype(np.uint32)


def fold(li, blocker):
    """The (n_samples, n) results of the scans -> open, intensity, rgba as the header defines them."""
    n_samples = li.shape[0]
    count = (blocker < 0).sum(axis=0)
    open_ = count.astype(np.float64) / float(n_samples)
    acc = li[0].copy()
    for s in range(1, n_samples):
        acc = acc + li[s]
    with np.errstate(invalid="ignore"):
        intensity = acc / float(n_samples)
    b = to_byte(open_)
    rgba = (b | (b << 8) | (b << 16) | np.uint32(0xff000000)).astype(np.uint32)
    return open_, intensity, rgba


def by_occlusion(scene, hits, dirs, n_samples, radius, stride=1, base=0, lib=None, probe=rt_host.ambient_segments):
    """The yardstick of the fused kernel: per sample the probe's segments through the existing rt_host.occlusion (length = radius,
    intensity = 1.0, the probe's skips), folded.  -> (open, intensity, rgba, li (n_samples, n), blocker (n_samples, n))."""
    n = len(hits)
    li, bl = np.empty((n_samples, n)), np.empty((n_samples, n), np.int32)
    for s in range(n_samples):
        rays, skip = probe(hits, s, n_samples, dirs=dirs, stride=stride, base=base, lib=lib)
        got = rt_host.occlusion(scene, rays, length=np.full(n, float(radius)), intensity=np.ones(n), skip=skip, want=("intensity", "blocker"), lib=lib)
        li[s], bl[s] = got["intensity"], got["blocker"]
    return fold(li, bl) + (li, bl)


def hand_built():
    """Receivers no view gives: inside a sphere (the normal is turned round), a miss, and records with a non-finite word."""
    h = rt_host.hit_records([[0.0, 1.5, 0.0], [0.3, 0.2, -0.1], [1.0, 2.0, 3.0], [np.nan, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 0.0]],
                            [[0.0, 1.0, 0.0], [0.6, 0.0, 0.8], [0.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, np.inf, 0.0], [0.0, 0.0, -1.0]],
                            [1, 0, -1, 2, 2, 3], [0, 1, 0, 0, 0, 1])
    return h
