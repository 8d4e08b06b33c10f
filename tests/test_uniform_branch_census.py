"""Wave-uniform decisions that go through lane masks in the six-wave trace kernels (CPU test: disassembles the gfx950 code object, as
tests/test_kernel_resources.py reads its notes; skipped without the ROCm LLVM tools).

profiles/uniform_branch_census.py counts, per kernel, the compiler's long forms of a decision that is the same for every lane:
s_cselect_b64 .., -1, 0 (a scalar condition made a lane mask), s_cbranch_vcc* fed by s_and_b64 / s_andn2_b64 vcc, exec, <mask> (a uniform
branch on such a mask) and v_cmp_* of scalar operands.  Every feature that added a wave-uniform decision to rt_trace<0,0,*,0,1> used to add
some (docs/EVIDENCE.md, "Scalar forms"); the counts of the committed build are recorded here, and a change that adds a long form to these two
kernels has to say so by raising them.  They stay strictly below the counts of the build before the scalar forms (PARENT: taken with the same
tool from that commit's rt_kernel_fast.o; its listing gave the same 49 s_cselect_b64 and 70 s_cbranch_vcc* in all)."""
import importlib.util
import os
import subprocess

from test_kernel_resources import CSRC, LLVM, TOOLS, pytestmark  # noqa: F401  (skipped without the ROCm LLVM tools)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = ("cselect", "vcc_branch", "scalar_cmp")
SIX = ("rt_traceILb0ELb0ELb0ELb0ELb1E", "rt_traceILb0ELb0ELb1ELb0ELb1E")      # <REFRACT, COUNT, SS2, GRID, W1>
PARENT = {SIX[0]: (49, 64, 13), SIX[1]: (49, 64, 13)}
COMMITTED = {SIX[0]: (39, 47, 3), SIX[1]: (39, 47, 3)}


def tool():
    spec = importlib.util.spec_from_file_location("uniform_branch_census", os.path.join(ROOT, "profiles", "uniform_branch_census.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def disassembly(obj, tmp_path):
    fat, co, dis = tmp_path / "k.bin", tmp_path / "k.co", tmp_path / "k.dis"
    subprocess.run([TOOLS[0], "--dump-section", ".hip_fatbin=%s" % fat, obj], check=True)
    subprocess.run([TOOLS[1], "--unbundle", "--type=o", "--input=%s" % fat, "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", "--output=%s" % co], check=True)
    with open(dis, "w") as f:
        subprocess.run([os.path.join(LLVM, "llvm-objdump"), "-d", "--no-show-raw-insn", str(co)], check=True, stdout=f)
    return str(dis)


def test_the_tool_counts_the_three_forms(tmp_path):
    """a listing written by hand: each form once, and the look-alikes that are none of them"""
    text = """
kernel_a:
\ts_cmp_eq_u32 s0, 1
\ts_cselect_b64 s[2:3], -1, 0
\ts_and_b64 vcc, exec, s[2:3]
\ts_cbranch_vccnz .LBB0_1
\ts_cselect_b32 s4, 0, 24
\tv_cmp_gt_f64_e64 s[4:5], s[6:7], 0
\tv_cmp_gt_f64_e32 vcc, 0, v[0:1]
\ts_cbranch_vccz .LBB0_1
\tv_cmp_lt_f64_e64 s[4:5], s[6:7], v[2:3]
\ts_andn2_b64 vcc, exec, s[4:5]
\tv_cmp_lt_u32_e32 vcc, s1, v0
\ts_cbranch_vccnz .LBB0_1
\ts_cmp_lg_u32 s0, 0
\ts_cbranch_scc1 .LBB0_1
.LBB0_1:
\ts_endpgm
.Lfunc_end0:
"""
    p = tmp_path / "hand.s"
    p.write_text(text)
    c = tool().census(str(p))["kernel_a"]
    assert [len(c[k]) for k in KEYS] == [1, 1, 1]
    assert c["all_vcc_branches"] == 3 and c["all_scc_branches"] == 1 and c["instructions"] == 15


def test_six_wave_kernels_keep_their_uniform_decisions_on_the_condition_code(built, tmp_path):
    mod = tool()
    res = mod.census(disassembly(os.path.join(CSRC, "rt_kernel_fast.o"), tmp_path))
    for sub in SIX:
        names = [k for k in res if sub in k]
        assert len(names) == 1, (sub, names)
        got = tuple(len(res[names[0]][k]) for k in KEYS)
        print(sub, dict(zip(KEYS, got)), "committed", COMMITTED[sub], "parent", PARENT[sub])
        for g, c, p, k in zip(got, COMMITTED[sub], PARENT[sub], KEYS):
            assert g <= c, (sub, k, g, "more than the committed build's", c)
            assert g < p, (sub, k, g, "not below the parent's", p)
