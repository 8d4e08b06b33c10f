"""TEST INFRASTRUCTURE for the primary-hit tests (tests/test_hits.py, tests/test_gpu_hits.py): the C restatement's per-sample probe
(oracle/rt_oracle.c oracle_probe_sample) as the expected id / depth / normal / hit record of a sample."""
import ctypes as C
import math

import numpy as np

import oracle_util as ou
import rt_host

PROBE_NODES, PROBE_WORDS = 64, 24


def oracle_lib():
    lib = ou.c_oracle()
    lib.oracle_probe_sample.restype = C.c_int
    lib.oracle_probe_sample.argtypes = [C.c_void_p, C.c_size_t, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p]
    lib.oracle_fd_atan2.restype = C.c_double
    lib.oracle_fd_atan2.argtypes = [C.c_double, C.c_double]
    lib.oracle_fd_asin.restype = C.c_double
    lib.oracle_fd_asin.argtypes = [C.c_double]
    return lib


def primary_blob(scene):
    """The scene flattened with depth 1 for the probe.  The primary hit does not depend on the depth (the hit loop and hit.p / hit.n
    of main.js:220-231, 440-449 come before any recursion), and at depth 1 the probe's record list never overflows its 64 nodes - its
    root record, written after the subtree's, would be lost in a deep refracting tree."""
    s = dict(scene)
    s["segs"] = 1
    return rt_host.flatten_scene(s)


class Probe:
    def __init__(self, scene, w, h):
        self.lib = oracle_lib()
        self.blob = primary_blob(scene)
        self.buf = C.create_string_buffer(self.blob, len(self.blob))
        self.w, self.h = w, h
        self.rec = np.zeros((PROBE_NODES, PROBE_WORDS), np.float64)

    def root(self, sx, sy):
        """The root record (path 1) of sample (sx, sy): q[1] = 2 hit_i + inside or -1, q[2] = t, q[3..5] = p, q[6..8] = n."""
        rc = self.lib.oracle_probe_sample(self.buf, len(self.blob), self.w, self.h, sx, sy, self.rec.ctypes.data)
        assert rc == 0
        roots = [q for q in self.rec if q[23] == 1 and q[0] == 1]
        assert len(roots) == 1
        return roots[0].copy()

    def expected(self, samples):
        """(id int32, depth float64, normal float32 x 3) arrays for [(sx, sy), ...], with the buffers' encoding."""
        n = len(samples)
        ids, depth, normal = np.empty(n, np.int32), np.empty(n, np.float64), np.zeros((n, 3), np.float32)
        for j, (sx, sy) in enumerate(samples):
            q = self.root(sx, sy)
            code = int(q[1])
            ids[j] = -1 if code < 0 else (code >> 1) | ((code & 1) << 16)
            depth[j] = q[2]
            normal[j] = np.float32(q[6:9]) if code >= 0 else 0.0
        return ids, depth, normal

    def uv(self, n):
        """hit.u / hit.v of main.js:446-447 from the oracle's normal, in Python (two successive divisions each, fdlibm)."""
        u = self.lib.oracle_fd_atan2(-n[2], -n[0]) / math.pi / 2 + 0.5
        v = self.lib.oracle_fd_asin(-n[1]) / (math.pi / 2) / 2 + 0.5
        return u, v
