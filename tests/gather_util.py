"""The yardstick of gathered light (include/rt_hip.h: struct rt_gather), built only from calls that exist without it: per sample the
host probe's segments (rt_host.ambient_segments), traced by the soft trace at levels 0 with one sample of point lights
(Renderer.trace_rays_soft, pix_base = pix_base + s pix_stride), folded in numpy in the stated order and passed through the store rule.
numpy's float64 + and / are IEEE operations, so what comes out here is compared with the library byte for byte."""
import ctypes as C

import numpy as np

import rt_host
from test_gpu_views import Dev


def to_byte(c):
    """The store rule of main.js:195-198: 255 c, NaN -> 0, clamped to 0..255, rounded half to even."""
    with np.errstate(invalid="ignore"):
        x = 255.0 * c
    x = np.where(np.isnan(x), 0.0, x)
    return np.rint(np.clip(x, 0.0, 255.0)).astype(np.uint32)


def fold(c):
    """(n_samples, n, 3) colours -> rgb (n, 3) float64, rgba (n,) uint32 as the header defines them."""
    acc = c[0].copy()
    for s in range(1, c.shape[0]):
        acc = acc + c[s]
    with np.errstate(invalid="ignore"):
        rgb = acc / float(c.shape[0])
    b = to_byte(rgb)
    return rgb, (b[:, 0] | (b[:, 1] << 8) | (b[:, 2] << 16) | np.uint32(0xff000000)).astype(np.uint32)


def by_soft(lib, hip, r, hits, dirs, n_samples, stride=1, segs=0, base=0, pix_base=0, pix_stride=None, objects=False):
    """-> (rgb, rgba, c (n_samples, n, 3)[, obj (n_samples, n) int32: the sphere each gathered ray meets first, -1 none]) with the
    resident scene of the Renderer `r` as it stands."""
    n = len(hits)
    ps = n if pix_stride is None else pix_stride
    d_rays, d_rgb, d_hits = Dev(lib, n * 48), Dev(lib, n * 24), Dev(lib, n * 80 if objects else 16)
    c, obj = np.empty((n_samples, n, 3)), np.empty((n_samples, n), np.int32)
    try:
        for s in range(n_samples):
            rays, _ = rt_host.ambient_segments(hits, s, n_samples, dirs=dirs, stride=stride, base=base, lib=lib)
            assert hip.hipMemcpy(C.c_void_p(d_rays.p), rays.ctypes.data_as(C.c_void_p), C.c_size_t(rays.nbytes), 1) == 0
            r.trace_rays_soft(n, d_rays.p, d_rgb.p, 0, 0, 1, 1, 0.0, levels=0, segs=segs, pix_base=pix_base + s * ps)
            c[s] = d_rgb.read(np.float64).reshape(n, 3)
            if objects:
                r.trace_rays(n, d_rays.p, 0, 0, d_hits.p, segs=1)
                obj[s] = d_hits.read(rt_host.HIT_DTYPE)["object"]
                obj[s][np.isnan(rays).any(axis=1)] = -1
    finally:
        for d in (d_rays, d_rgb, d_hits):
            d.close()
    return fold(c) + ((c, obj) if objects else (c,))
