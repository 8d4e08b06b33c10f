"""TEST INFRASTRUCTURE for the wavefront tests (tests/test_nodes.py, tests/test_gpu_nodes.py, tests/test_gpu_nodes_edges.py): the C restatement's probe records
(oracle/rt_oracle.c oracle_probe_sample: every node of a sample's ray tree) for micro-cameras (tests/rays_util.py) at a given depth,
those records as rt_node arrays level by level, and a walk of a ray list level by level through Renderer.shade_rays / spawn_rays."""
import ctypes as C
import math
import struct

import numpy as np

import hits_util as hu
import rays_util as ru
import rt_host

MISS_COLOR_OFFSET = 136                                   # in rt_scene_header (include/rt_hip.h)
CANARY = 0x5A


# ------------------------------------------------------------------ the restatement's trees
class TreeOracle:
    """Probe records of micro-cameras of one scene at depth `segs`: per ray {path: record}."""

    def __init__(self, scene, segs):
        s = dict(scene)
        s["supersample"] = 1
        s["segs"] = segs
        self.scene, self.segs = s, segs
        self.blob = bytearray(rt_host.flatten_scene(s))
        self.lib = hu.oracle_lib()
        self.fov = float(s.get("fovDeg", 60))
        self.miss_color = struct.unpack_from("<3d", self.blob, MISS_COLOR_OFFSET)
        self.albedo = np.array([o["mtl"]["albedo"] for o in s["objects"]], np.float64)
        self.rec = np.zeros((hu.PROBE_NODES, hu.PROBE_WORDS), np.float64)
        self.overflowed = 0

    def trees(self, cams):
        """-> [ {path: q (24 float64)} per ray ], in micro_rays' order (camera j's four pixels at 4 j .. 4 j + 3)."""
        out = []
        for cam in np.asarray(cams, np.float64):
            struct.pack_into("<12d", self.blob, ru.CAMERA_OFFSET, *ru._camera_words(cam))
            buf = C.create_string_buffer(bytes(self.blob), len(self.blob))
            for k in range(4):
                assert self.lib.oracle_probe_sample(buf, len(self.blob), 2, 2, k & 1, k >> 1, self.rec.ctypes.data) == 0
                valid = self.rec[self.rec[:, 23] == 1]
                tree = {int(q[0]): q.copy() for q in valid}
                assert len(tree) == len(valid)
                # complete: a root, every other record's parent, and exactly the children the masks name
                whole = 1 in tree and all(p == 1 or (p >> 1) in tree for p in tree) and \
                    all(((2 * p in tree), (2 * p + 1 in tree)) == (bool(int(q[22]) & 1), bool(int(q[22]) & 2)) for p, q in tree.items())
                if not whole:
                    self.overflowed += 1
                out.append(tree)
        return out

    def rgba(self, cams):
        """c_oracle_render's bytes of the same rays: (4 m, 4) uint8."""
        import oracle_util as ou
        out = []
        for cam in np.asarray(cams, np.float64):
            struct.pack_into("<12d", self.blob, ru.CAMERA_OFFSET, *ru._camera_words(cam))
            out.append(np.frombuffer(ou.c_oracle_render(bytes(self.blob), 2, 2), np.uint8).reshape(4, 4))
        return np.concatenate(out)

    def levels(self, trees):
        """The trees as the wavefront form holds them: per level a NODE_DTYPE array in (parent, reflect-then-refract) order, its (n, 2)
        links into the next level, and per node (root ray, path).  The fields are the probe's; the weights come from the scene."""
        levels = []
        cur = [(j, 1) for j in range(len(trees))]
        while cur:
            nodes = np.zeros(len(cur), rt_host.NODE_DTYPE)
            links = np.full((len(cur), 2), -1, np.int32)
            nxt = []
            for i, (j, p) in enumerate(cur):
                q = trees[j][p]
                code = int(q[1])
                nd = nodes[i]
                if code < 0:
                    nd["object"], nd["t"], nd["sample"] = -1, np.inf, self.miss_color
                else:
                    a = self.albedo[code >> 1]
                    nd["object"], nd["inside"], nd["t"], nd["point"], nd["normal"] = code >> 1, code & 1, q[2], q[3:6], q[6:9]
                    nd["sample"], nd["diffuse"], nd["specular"] = q[12:15], q[15], q[16]
                    nd["ambient"], nd["reflect_weight"], nd["refract_weight"] = a[0], a[3], a[4]
                    nd["children"] = int(q[22])
                for k in range(2):
                    if 2 * p + k in trees[j]:
                        links[i, k] = len(nxt)
                        nxt.append((j, 2 * p + k))
            levels.append({"nodes": nodes, "links": links, "ids": cur})
            cur = nxt
        return levels


def fold_levels(levels):
    """rt_host.fold_nodes_host bottom-up -> the roots' (n, 3) rgb."""
    rgb = None
    for lv in reversed(levels):
        rgb = rt_host.fold_nodes_host(lv["nodes"], lv["links"] if rgb is not None else None, rgb)
    return rgb


# ------------------------------------------------------------------ device memory
_hip = None


def hip():
    global _hip
    if _hip is None:
        _hip = C.CDLL("libamdhip64.so")                   # (the ABI has no upload helper: hosts hand over memory they filled themselves)
    return _hip


class Dev:
    """A canary-framed device array."""
    PAD = 256

    def __init__(self, lib, nbytes, src=None, fill=CANARY):
        self.lib, self.nbytes, self.fill = lib, nbytes, fill
        self.base = lib.rt_alloc_device(0, nbytes + 2 * self.PAD)
        assert self.base, lib.rt_last_error()
        assert lib.rt_memset_device(0, self.base, fill, nbytes + 2 * self.PAD) == 0
        self.ptr = self.base + self.PAD
        if src is not None:
            src = np.ascontiguousarray(src)
            assert src.nbytes == nbytes
            assert hip().hipMemcpy(C.c_void_p(self.ptr), src.ctypes.data_as(C.c_void_p), C.c_size_t(nbytes), 1) == 0

    def read(self, dtype=np.uint8):
        raw = np.empty(self.nbytes + 2 * self.PAD, np.uint8)
        assert self.lib.rt_copy_to_host(0, raw.ctypes.data, self.base, raw.nbytes) == 0
        assert (raw[:self.PAD] == self.fill).all() and (raw[-self.PAD:] == self.fill).all(), "a write outside the array"
        return raw[self.PAD:self.PAD + self.nbytes].view(dtype).copy()

    def close(self):
        if self.base:
            self.lib.rt_free_device(0, self.base)
            self.base = 0


def spawn(lib, r, nodes, pix=None, path=None):
    """Renderer.spawn_rays of a host NODE_DTYPE array -> dict(count, rays (count, 6), pix, path, links (n, 2), raw: the four buffers' bytes)."""
    n = len(nodes)
    wb = rt_host.nodes_spawn_work_bytes(n, lib)
    bufs = [Dev(lib, n * 200, nodes), Dev(lib, 2 * n * 48), Dev(lib, 2 * n * 4), Dev(lib, 2 * n * 4), Dev(lib, 2 * n * 4), Dev(lib, 4), Dev(lib, wb)]
    d_pix = Dev(lib, n * 4, np.asarray(pix, np.uint32)) if pix is not None else None
    d_path = Dev(lib, n * 4, np.asarray(path, np.uint32)) if path is not None else None
    try:
        d_nodes, d_rays, d_cpix, d_cpath, d_links, d_count, d_work = bufs
        r.spawn_rays(n, d_nodes.ptr, d_rays.ptr, d_links.ptr, d_count.ptr, d_work.ptr, wb, pix_ptr=d_pix.ptr if d_pix else 0,
                     path_ptr=d_path.ptr if d_path else 0, child_pix_ptr=d_cpix.ptr, child_path_ptr=d_cpath.ptr)
        count = int(d_count.read(np.uint32)[0])
        assert count <= 2 * n
        raw = [d_rays.read(), d_cpix.read(), d_cpath.read(), d_links.read()]
        return {"count": count, "rays": raw[0].view(np.float64).reshape(2 * n, 6)[:count], "pix": raw[1].view(np.uint32)[:count],
                "path": raw[2].view(np.uint32)[:count], "links": raw[3].view(np.int32).reshape(n, 2), "raw": [x.tobytes() for x in raw]}
    finally:
        for b in bufs + [d_pix, d_path]:
            if b:
                b.close()


def shade(lib, r, rays, pix=None, path=None, order=None, fill=CANARY):
    """Renderer.shade_rays of a host ray list -> NODE_DTYPE array (order: a host uint32 array, or None)."""
    n = len(rays)
    d_rays, d_nodes = Dev(lib, n * 48, np.asarray(rays, np.float64)), Dev(lib, n * 200, fill=fill)
    opt = [Dev(lib, len(a) * 4, np.asarray(a, np.uint32)) if a is not None else None for a in (pix, path, order)]
    try:
        r.shade_rays(n, d_rays.ptr, d_nodes.ptr, order_ptr=opt[2].ptr if opt[2] else 0, pix_ptr=opt[0].ptr if opt[0] else 0,
                     path_ptr=opt[1].ptr if opt[1] else 0, want_stats=True)
        return d_nodes.read().view(rt_host.NODE_DTYPE)
    finally:
        for b in [d_rays, d_nodes] + opt:
            if b:
                b.close()


def fold(lib, r, nodes, links=None, child_rgb=None, want_rgb=True, want_rgba=True):
    """Renderer.fold_nodes of host arrays -> (rgb (n, 3) float64, rgba (n, 4) uint8).  An output that is not wanted is handed over as
    NULL and comes back as None: its buffer is there all the same, and must still hold the canary throughout."""
    n = len(nodes)
    d_nodes, d_rgb, d_rgba = Dev(lib, n * 200, nodes), Dev(lib, n * 24), Dev(lib, n * 4)
    d_links = Dev(lib, n * 8, np.asarray(links, np.int32)) if links is not None else None
    d_child = Dev(lib, max(len(child_rgb), 1) * 24, np.asarray(child_rgb, np.float64) if len(child_rgb) else np.zeros(3)) if links is not None else None
    try:
        r.fold_nodes(n, d_nodes.ptr, d_links.ptr if d_links else 0, d_child.ptr if d_child else 0, d_rgb.ptr if want_rgb else 0,
                     d_rgba.ptr if want_rgba else 0)
        rgb, rgba = d_rgb.read(np.float64).reshape(n, 3), d_rgba.read().reshape(n, 4)
        assert want_rgb or (rgb.view(np.uint8) == CANARY).all(), "a write to the rgb that was not asked for"
        assert want_rgba or (rgba == CANARY).all(), "a write to the rgba that was not asked for"
        return rgb if want_rgb else None, rgba if want_rgba else None
    finally:
        for b in (d_nodes, d_rgb, d_rgba, d_links, d_child):
            if b:
                b.close()


def fold_walk(lib, r, levels):
    """The levels of walk() folded bottom-up on the GPU -> the list's (rgb, rgba)."""
    rgb = rgba = None
    for lv in reversed(levels):
        rgb, rgba = fold(lib, r, lv["nodes"], lv["links"] if rgb is not None else None, rgb)
    return rgb, rgba


def walk(lib, r, rays, segs):
    """The list level by level through shade and spawn, `segs` levels at most: per level dict(nodes, rays, pix, path, root (the index of
    the list's ray the node descends from), links or None below the last level shaded)."""
    n = len(rays)
    cur = {"rays": np.asarray(rays, np.float64), "pix": None, "path": None, "root": np.arange(n)}
    levels = []
    for lv in range(segs):
        cur["nodes"] = shade(lib, r, cur["rays"], cur["pix"], cur["path"])
        cur["links"] = None
        levels.append(cur)
        if lv + 1 == segs:
            break
        sp = spawn(lib, r, cur["nodes"], cur["pix"], cur["path"])
        cur["links"] = sp["links"]
        if sp["count"] == 0:
            break
        root = np.empty(sp["count"], np.int64)
        for k in range(2):
            m = sp["links"][:, k] >= 0
            root[sp["links"][m, k]] = cur["root"][m]
        cur = {"rays": sp["rays"], "pix": sp["pix"], "path": sp["path"], "root": root}
    for lv in levels:
        if lv["pix"] is None:
            lv["pix"], lv["path"] = np.arange(len(lv["rays"]), dtype=np.uint32), np.ones(len(lv["rays"]), np.uint32)
    return levels


def same_bits(a, b):
    return np.ascontiguousarray(a, np.float64).tobytes() == np.ascontiguousarray(b, np.float64).tobytes()


# ------------------------------------------------------------------ walked nodes against the restatement's
def probe_uv(oracle):
    """hit.u / hit.v of main.js:446-447 from the restatement's normal (two successive divisions each, fdlibm): MicroOracle.hit_of's."""
    def uv(n):
        return (oracle.lib.oracle_fd_atan2(-n[2], -n[0]) / math.pi / 2 + 0.5, oracle.lib.oracle_fd_asin(-n[1]) / (math.pi / 2) / 2 + 0.5)
    return uv


def assert_nodes_are_the_restatements(levels, trees, oracle, objs, segs, tag):
    """Every node of walk()'s levels is the probe record of its (root ray, path), bit for bit: the ray it was shaded for, the hit record,
    u and v, sample, diffuse, the three weights, the children mask, and as many nodes per tree as the probe has.
    -> (nodes, hits, two-child nodes)."""
    albedo = np.array([o["mtl"]["albedo"] for o in objs], np.float64)
    per_tree = np.zeros(len(trees), np.int64)
    fd = probe_uv(oracle)
    n_nodes = n_hits = n_children = 0
    for depth, lv in enumerate(levels):
        nd, n = lv["nodes"], len(lv["nodes"])
        assert all(int(p) in trees[int(j)] for j, p in zip(lv["root"], lv["path"])), "a node the restatement does not have"
        Q = np.array([trees[int(j)][int(p)] for j, p in zip(lv["root"], lv["path"])])
        assert (Q[:, 17] == segs - depth).all()                                          # segs left: the level
        np.add.at(per_tree, lv["root"], 1)
        # the ray this node was shaded for: the list's (level 1), or the one spawn wrote
        assert same_bits(lv["rays"][:, 0:3], Q[:, 19:22]) and same_bits(lv["rays"][:, 3:6], Q[:, 9:12]), (tag, segs, depth)
        code = Q[:, 1].astype(int)
        hit = code >= 0
        assert (nd["object"] == np.where(hit, code >> 1, -1)).all() and (nd["inside"] == np.where(hit, code & 1, 0)).all()
        assert same_bits(nd["t"], Q[:, 2])
        assert same_bits(nd["point"], Q[:, 3:6]) and same_bits(nd["normal"], Q[:, 6:9])
        uv = np.array([fd(q[6:9]) if c >= 0 else (0.0, 0.0) for q, c in zip(Q, code)]).reshape(n, 2)
        assert same_bits(nd["u"], uv[:, 0]) and same_bits(nd["v"], uv[:, 1])
        want_sample = np.where(hit[:, None], Q[:, 12:15], np.array(oracle.miss_color)[None, :])
        assert same_bits(nd["sample"], want_sample), (tag, segs, depth, int((nd["sample"] != want_sample).sum()))
        assert same_bits(nd["diffuse"], Q[:, 15]), (tag, segs, depth, int((nd["diffuse"] != Q[:, 15]).sum()))
        a = albedo[np.where(hit, code >> 1, 0)] * hit[:, None]
        assert same_bits(nd["ambient"], a[:, 0]) and same_bits(nd["reflect_weight"], a[:, 3]) and same_bits(nd["refract_weight"], a[:, 4])
        assert (nd["specular"][a[:, 2] == 0] == 0).all() and (nd["reserved"] == 0).all()
        if depth + 1 < segs:
            assert (nd["children"] == Q[:, 22].astype(int)).all()
        assert (nd["children"][~hit] == 0).all()
        assert not nd["reflect_dir"][(nd["children"] & 1) == 0].any() and not nd["refract_dir"][(nd["children"] & 2) == 0].any()
        n_nodes, n_hits, n_children = n_nodes + n, n_hits + int(hit.sum()), n_children + int((nd["children"] == 3).sum())
    assert (per_tree == np.array([len(t) for t in trees])).all()                        # the number of nodes per tree is the probe's
    return n_nodes, n_hits, n_children


def trace_wavefront_abi(lib, scene, rays, segs=0, want=("rgb", "rgba"), with_stats=False, order_levels=False):
    """rt_trace_rays_wavefront through ctypes, with an RtStats where asked (rt_host.trace_rays passes none)
    -> dict(rgb, rgba (those wanted), level_counts, stats or None)."""
    blob = scene if isinstance(scene, (bytes, bytearray)) else rt_host.flatten_scene(scene)
    rays = np.asarray(rays, np.float64)
    n = len(rays)
    aligned = np.empty(n * 6 + 2, np.float64)             # a contiguous copy on a 16-byte boundary
    aligned = aligned[(aligned.ctypes.data >> 3) & 1:][:n * 6]
    aligned[:] = rays.reshape(-1)
    out = {"level_counts": np.zeros(rt_host.RT_MAX_SEGS, np.uint64), "stats": rt_host.RtStats() if with_stats else None}
    if "rgb" in want:
        out["rgb"] = np.empty((n, 3), np.float64)
    if "rgba" in want:
        out["rgba"] = np.empty((n, 4), np.uint8)
    bufs = rt_host.RtRayOutputs(out["rgb"].ctypes.data if "rgb" in out else None, out["rgba"].ctypes.data if "rgba" in out else None, None)
    buf = C.create_string_buffer(bytes(blob), len(blob))
    rc = lib.rt_trace_rays_wavefront(buf, len(blob), n, C.c_void_p(aligned.ctypes.data), segs, 1 if order_levels else 0, C.byref(bufs),
                                     C.byref(out["stats"]) if with_stats else None, out["level_counts"].ctypes.data_as(C.POINTER(C.c_uint64)))
    assert rc == 0, lib.rt_last_error()
    return out
