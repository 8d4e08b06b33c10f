"""The register budget of six waves per SIMD (CPU test: reads the gfx950 code object, as tests/test_kernel_resources.py does).

The few-sphere one-wave trace kernels, rt_trace<0,0,0,0,1> and <0,0,1,0,1>, run six waves per SIMD: 512 / 6 rounded down to the
allocation granule of 8 is 80 VGPRs, and neither a spilled register nor a byte of scratch - a spill would put scratch set-up into every
one of the headline's 66 592 waves.  An 81st register silently costs the sixth wave and what it bought (docs/EVIDENCE.md, "Six waves per SIMD").
Every other instantiation keeps the budget tests/test_kernel_resources.py states: five waves, 96 VGPRs."""
import os

from test_kernel_resources import CSRC, kernel_notes, pytestmark  # noqa: F401  (skipped without the ROCm LLVM tools)

SIX = [(0, 0, 0, 0, 1), (0, 0, 1, 0, 1)]      # <REFRACT, COUNT, SS2, GRID, W1>


def test_few_sphere_one_wave_kernels_fit_six_waves(built, tmp_path):
    k = kernel_notes(os.path.join(CSRC, "rt_kernel_fast.o"), tmp_path)
    for key in SIX:
        r = k[key]
        assert r["vgpr_count"] <= 80, (key, r)
        assert r["vgpr_spill_count"] == 0 and r["sgpr_spill_count"] == 0, (key, r)
        assert r["private_segment_fixed_size"] == 0, (key, r)
        assert r["max_flat_workgroup_size"] == 64, (key, r)


def test_the_other_kernels_keep_their_budget(built, tmp_path):
    k = kernel_notes(os.path.join(CSRC, "rt_kernel_fast.o"), tmp_path)
    assert len(k) == 16
    for key, r in k.items():
        refract, count, ss2, grid, w1 = key
        if key in SIX or count:                       # (the counting kernels are a test aid, not a product path)
            continue
        may_spill = (refract, count, ss2, grid) == (0, 0, 1, 1) or (w1 and grid)      # tests/test_kernel_resources.py says why
        assert r["vgpr_count"] <= 96, (key, r)
        assert r["vgpr_spill_count"] <= (1 if may_spill else 0) and r["sgpr_spill_count"] <= (4 if may_spill else 0), (key, r)
        if not refract:
            assert r["private_segment_fixed_size"] <= (16 if may_spill else 0), (key, r)
