"""TEST INFRASTRUCTURE for relit nodes (tests/test_relight.py, tests/test_gpu_relight.py, tests/test_node_relight.py).  The yardstick
needs nothing of the feature: a relit node is the mean of the nodes rt_host.shade_rays writes for the same ray in scenes whose lights
were moved on the host, so by_moved_lights shades the list once per table entry it uses, gathers each node's (diffuse, specular) pairs
by the stated index and folds them in the stated order, in numpy float64."""
import json

import numpy as np

import lighting_util as lu
import nodes_util as nu
import rt_host

W, H = 96, 54
RELIT = slice(104, 120)                                   # the bytes of a node a relight may write: diffuse and specular


def copy_of(scene, **changes):
    """A scene dict to edit: everything but the textures' texels copied."""
    return dict(json.loads(json.dumps({k: v for k, v in scene.items() if k != "textures"})), textures=scene["textures"], **changes)


def entries(n, n_offs, n_samples, stride, base, pix=None):
    """-> (n, n_samples) int64: e = ((base + pix_i) * stride + s) % n_offs in unsigned 64-bit arithmetic that wraps at 2^64."""
    pix = np.arange(n) if pix is None else np.asarray(pix)
    out = np.empty((n, n_samples), np.int64)
    for i, p in enumerate(pix.tolist()):
        P = ((base + p) * stride) % 2 ** 64
        for s in range(n_samples):
            out[i, s] = ((P + s) % 2 ** 64) % n_offs
    return out


def moved_scene(scene, o, radius):
    """The scene with every light at light[c] + radius * o[c]: one multiply and one add per component in float64 (lgt_light_pos); the
    lights themselves at radius 0, where the table is not read."""
    lights = np.array(scene["lights"], np.float64).reshape(-1, 3)
    if radius != 0.0:
        lights = lights + np.float64(radius) * np.asarray(o, np.float64)[None, :]
    return copy_of(scene, lights=lights.tolist())


def fold(x):
    """x (n, n_samples) -> acc = x_0; acc = acc + x_s in order; acc / (double)n_samples."""
    acc = x[:, 0].copy()
    with np.errstate(invalid="ignore", over="ignore"):
        for s in range(1, x.shape[1]):
            acc = acc + x[:, s]
        return acc / np.float64(x.shape[1])


def by_moved_lights(scene, rays, offs, n_samples, radius, stride=1, base=0, pix=None, path=None, lib=None, shaded=None):
    """-> (NODE_DTYPE array, diffuse (n, n_samples), specular (n, n_samples)): what a relight of shade_rays(scene, rays) has to give,
    and the samples it is the fold of, from rt_host.shade_rays alone - one call per distinct table entry the list uses (one at radius
    0).  shaded: a dict that keeps the nodes per entry, for the cases that share scene, rays, pix, table and radius - the reference is
    computed once and never written to."""
    n = len(rays)
    n_offs = n_samples if offs is None else len(offs)
    e = entries(n, n_offs, n_samples, stride, base, pix) if radius != 0.0 else np.zeros((n, n_samples), np.int64)
    used = np.unique(e)
    assert len(used) <= 8, "the yardstick is held to 8 shade calls per case"
    diffuse, specular = np.empty((n, n_samples)), np.empty((n, n_samples))
    template = None
    for k in used.tolist():
        if shaded is not None and k in shaded:
            nodes = shaded[k]
        else:
            nodes = rt_host.shade_rays(moved_scene(scene, offs[k] if radius != 0.0 else None, radius), rays, pix=pix, path=path, lib=lib)
            nodes.setflags(write=False)
            if shaded is not None:
                shaded[k] = nodes
        if template is None:
            template = nodes.copy()
        else:                                             # a light decides two numbers of a node and nothing else
            a, b = template.view(np.uint8).reshape(n, 200), nodes.view(np.uint8).reshape(n, 200)
            assert (a[:, :104] == b[:, :104]).all() and (a[:, 120:] == b[:, 120:]).all()
        m = e == k
        diffuse[m] = np.broadcast_to(nodes["diffuse"][:, None], m.shape)[m]
        specular[m] = np.broadcast_to(nodes["specular"][:, None], m.shape)[m]
    template["diffuse"], template["specular"] = fold(diffuse), fold(specular)
    return template, diffuse, specular


def same_nodes(got, want, what):
    n = len(want)
    assert len(got) == n, what
    g, w = np.ascontiguousarray(got).view(np.uint8).reshape(n, 200), np.ascontiguousarray(want).view(np.uint8).reshape(n, 200)
    bad = (g != w).any(axis=1)
    assert not bad.any(), (what, int(bad.sum()), int(np.flatnonzero(bad)[0]), got[np.flatnonzero(bad)[0]], want[np.flatnonzero(bad)[0]])


_lists = {}


def ray_list(lib, name):
    """Per scene, once: (scene, rays) - the W x H view from the scene's camera and one level of its spawned children, so that the
    direction and `inside` vary - with the number of primary rays."""
    if name not in _lists:
        scene = rt_host.load_scene(name)
        primary = rt_host.view_rays(lu.camera_view(scene), W, H, lib=lib).reshape(-1, 6)
        r = rt_host.Renderer(scene, 0, lib)
        try:
            levels = nu.walk(lib, r, primary, 2)
        finally:
            r.close()
        rays = np.ascontiguousarray(np.concatenate([lv["rays"] for lv in levels]))
        _lists[name] = (scene, rays, len(primary))
    return _lists[name]


class Relit:
    """A ray list, its shaded nodes (canary-framed) and a table in device memory, and Renderer.relight_nodes on them."""

    def __init__(self, lib, r, rays, offs=None, pix=None, order=None, nodes=None):
        self.lib, self.r, self.n = lib, r, len(rays)
        self.n_offs = 0 if offs is None else len(offs)
        self.d_rays = nu.Dev(lib, self.n * 48, np.asarray(rays, np.float64))
        self.d_nodes = nu.Dev(lib, self.n * 200, nodes)
        self.d_offs = nu.Dev(lib, self.n_offs * 24, np.asarray(offs, np.float64)) if offs is not None else None
        self.d_pix = nu.Dev(lib, self.n * 4, np.asarray(pix, np.uint32)) if pix is not None else None
        self.d_order = nu.Dev(lib, len(order) * 4, np.asarray(order, np.uint32)) if order is not None else None
        if nodes is None:
            r.shade_rays(self.n, self.d_rays.ptr, self.d_nodes.ptr, pix_ptr=self.d_pix.ptr if self.d_pix else 0)

    def nodes(self):
        return self.d_nodes.read().view(rt_host.NODE_DTYPE)

    def relight(self, n_samples, radius, stride=1, base=0, n=None, use_order=True, **kw):
        return self.r.relight_nodes(self.n if n is None else n, self.d_rays.ptr, self.d_nodes.ptr, self.d_offs.ptr if self.d_offs else 0,
                                    self.n_offs or n_samples, n_samples, radius, stride=stride, base=base,
                                    order_ptr=self.d_order.ptr if self.d_order and use_order else 0, pix_ptr=self.d_pix.ptr if self.d_pix else 0, **kw)

    def close(self):
        for d in (self.d_rays, self.d_nodes, self.d_offs, self.d_pix, self.d_order):
            if d:
                d.close()
