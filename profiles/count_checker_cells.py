"""Count, with the HOST build of the launch table (no GPU), the waves whose checker cell the table states (rt_block.h: rt_column_cell).

    python3 profiles/count_checker_cells.py [scene] [w] [h]        default: h8 3840 2160
    python3 profiles/count_checker_cells.py --frames               h8 at 3840x2160, 7680x4320 and 1001x563, one line each

Prints the one-candidate entries' waves (the uniform-material path's candidates), how many of them carry the whole-cell flag, and how
many of the others have ONE axis of the checker stated (rt_block.h: rt_cells_word), per axis.  (What the whole-cell statement flagged
while it bounded a column's hits by a ball instead of per axis is on record in docs/EVIDENCE.md: 26 638 waves of h8 at 3840x2160.)"""
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "html5-canvas-raytracer_amd"))
import rt_host  # noqa: E402

CELLS = 1 | 2 | 4 | 32          # ranked, sky marks, masks + candidates, checker cells
AXES = CELLS | 64               # ... and the per-axis statements


def table(lib, blob, w, h, flags=AXES, tiles=None):
    t = rt_host.RtTiles(*(tiles or (h, 0, 1, 1)))
    buf = C.create_string_buffer(blob, len(blob))
    n, nb = C.c_uint32(), C.c_uint32()
    assert lib.rt_scene_launch_table(buf, len(blob), w, h, C.byref(t), flags, None, C.byref(n), C.byref(nb)) == 0, lib.rt_last_error()
    out = (C.c_uint32 * (4 * 8 * ((nb.value + 7) // 8)))()
    assert lib.rt_scene_launch_table(buf, len(blob), w, h, C.byref(t), flags, out, C.byref(n), C.byref(nb)) == 0, lib.rt_last_error()
    return np.frombuffer(out, dtype=np.uint32).reshape(-1, 4).copy()


def counts(tab):
    live = tab[(tab[:, 0] >> 11) & 15 != 0]
    live = live[live[:, 1] >> 31 == 0]
    one = live[(live[:, 3] >> 16) & 3 == 1]
    flagged = sum(int(((one[:, 3] >> (18 + c)) & 1).sum()) for c in range(4))
    axis = sum(((one[:, 3] >> (26 + c)) & 1) for c in range(4))          # columns with ONE axis stated; bit 30: which axis, per entry
    which = (one[:, 3] >> 30) & 1
    return {"entries": len(live), "one_candidate_waves": 4 * len(one), "flagged_waves": flagged,
            "u_only_waves": int(axis[which == 0].sum()), "v_only_waves": int(axis[which == 1].sum())}


def report(lib, name, w, h):
    c = counts(table(lib, rt_host.flatten_scene(rt_host.load_scene(name)), w, h))
    c["share"] = round(c["flagged_waves"] / max(1, c["one_candidate_waves"]), 4)
    print(name, w, h, c)


if __name__ == "__main__":
    lib = rt_host.load_library()
    if sys.argv[1:2] == ["--frames"]:
        for w, h in ((3840, 2160), (7680, 4320), (1001, 563)):
            report(lib, "h8", w, h)
        sys.exit(0)
    name = sys.argv[1] if len(sys.argv) > 1 else "h8"
    w, h = (int(sys.argv[2]), int(sys.argv[3])) if len(sys.argv) > 3 else (3840, 2160)
    report(lib, name, w, h)
