"""Per-axis checker statements, the GPU build of the table (rt_tables_gpu.hip; rt_block.h: rt_column_cell, rt_cells_word): the launch
table as the library builds it on the GPU with bit 6 of `ranked` - the per-axis statements of the columns that are not inside one
checker cell - is the host build's word for word.  (The host build's statements are held to the C restatement's probe by
test_checker_axes.py.  The trace kernels do not read the per-axis bits and product launches do not ask for them: docs/EVIDENCE.md.)"""
import pytest

import rt_host
from objects_util import gpu_table, host_table, tlib  # noqa: F401  (fixture: the test library)
from test_checker_axes import AXES, axis_columns
from test_checker_cells import h8, pole_scene, table

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name,wh,ss", [("h8", (1280, 720), 1), ("h8", (1001, 563), 2), ("pole", (1280, 720), 1)])
def test_the_gpu_build_states_the_hosts_words(tlib, name, wh, ss):  # noqa: F811
    s = pole_scene() if name == "pole" else h8(supersample=ss)
    blob = rt_host.flatten_scene(s)
    assert len(axis_columns(table(tlib, blob, *wh, AXES))) > 0          # not vacuous: the frame has such columns
    r = rt_host.Renderer(blob, 0, tlib)
    try:
        for tiles in ((wh[1], 0, 1, 1), (16, 1, 2, (wh[1] // 16) // 2)):
            assert gpu_table(tlib, r, *wh, tiles, AXES, ss) == host_table(tlib, blob, *wh, tiles, AXES)
    finally:
        r.close()
