"""tools/dep_pairs.py on a few hand-written gfx950 assembly lines: what it takes for a write and a read (implicit vcc of the
e32 compares and selects, scalar pairs of the e64 forms, SDWA and DPP operands with their modifiers, register ranges), that a
pad does not break the pair around it, the wait states of s_nop N, the longest run, and the split into basic blocks."""
import importlib.util
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "tools", "dep_pairs.py")

spec = importlib.util.spec_from_file_location("dep_pairs", TOOL)
dep_pairs = importlib.util.module_from_spec(spec)
spec.loader.exec_module(dep_pairs)

KERNEL = """\t.text
_ZN7alacdev6k_demoEv:                   ; @_ZN7alacdev6k_demoEv
; %bb.0:
\tv_mul_i32_i24_sdwa v16, sext(v24), v181 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:WORD_0 src1_sel:DWORD
\tv_add3_u32 v16, v16, v93, v17
\ts_nop 1
\tv_add_u32_dpp v16, v16, v16 quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf bound_ctrl:1
\tv_lshrrev_b32_e32 v18, 9, v16
\t;;#ASMSTART
\tv_med3_i32 v87, v179, -1, 1
\t;;#ASMEND
\tv_add_u32_e32 v19, v182, v18
\ts_cbranch_scc1 .LBB0_2
.LBB0_1:                                ; %loop
\tv_cmp_gt_i32_e32 vcc, v17, v85
\ts_nop 0
\ts_nop 1
\tv_cndmask_b32_e32 v79, 0, v18, vcc
\tv_cmp_gt_i32_e64 s[2:3], v17, v73
\tv_cmp_gt_i32_e64 s[28:29], v17, v74
\tv_cndmask_b32_e64 v80, 0, v18, s[2:3]
\tv_mad_i32_i24 v24, v80, v75, v24
\tds_write2_b32 v158, v16, v24 offset0:8 offset1:9
\tglobal_load_dwordx4 v[4:7], v1, s[8:9]
\tv_add_u32_e32 v9, v6, v2
.LBB0_2:
\ts_endpgm
.Lfunc_end0:
_ZN7alacdev7k_otherEv:
\tv_mov_b32_e32 v1, v0
\tv_mov_b32_e32 v2, v1
\ts_endpgm
.Lfunc_end1:
"""


def test_defs_and_uses():
    du = dep_pairs.defs_uses
    assert du("v_add3_u32 v16, v16, v93, v17") == ("v_add3_u32", {("v", 16)}, {("v", 16), ("v", 93), ("v", 17)})
    m, d, u = du("v_mul_i32_i24_sdwa v16, sext(v24), v181 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:WORD_0 src1_sel:DWORD")
    assert d == {("v", 16)} and u == {("v", 24), ("v", 181)}
    m, d, u = du("v_add_u32_dpp v16, v15, v14 quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf bound_ctrl:1")
    assert d == {("v", 16)} and u == {("v", 15), ("v", 14)}
    m, d, u = du("v_cmp_gt_i32_e32 vcc, v17, v85")
    assert d == {("vcc", 0)} and u == {("v", 17), ("v", 85)}
    m, d, u = du("v_cndmask_b32_e32 v79, 0, v18, vcc")
    assert d == {("v", 79)} and u == {("v", 18), ("vcc", 0)}
    m, d, u = du("v_cmp_gt_i32_e64 s[2:3], v17, v73")
    assert d == {("s", 2), ("s", 3)} and u == {("v", 17), ("v", 73)}
    m, d, u = du("v_cndmask_b32_e64 v80, 0, v18, s[2:3]")
    assert d == {("v", 80)} and u == {("v", 18), ("s", 2), ("s", 3)}
    m, d, u = du("ds_write2_b32 v158, v16, v24 offset0:8 offset1:9")
    assert d == set() and u == {("v", 158), ("v", 16), ("v", 24)}
    m, d, u = du("global_load_dwordx4 v[4:7], v1, s[8:9]")
    assert d == {("v", 4), ("v", 5), ("v", 6), ("v", 7)} and u == {("v", 1), ("s", 8), ("s", 9)}
    assert du("s_nop 1") == ("s_nop", set(), set())
    assert du("s_cbranch_vccnz .LBB26_1171")[2] == {("vcc", 0)}


def test_blocks_and_counts():
    blocks = dep_pairs.kernel_blocks(KERNEL.splitlines(), "k_demo")
    assert [n for n, _ in blocks] == ["entry", ".LBB0_1", ".LBB0_2"]
    assert [len(b) for _, b in blocks] == [8, 11, 1]  # the other kernel's lines are not counted
    entry = dep_pairs.block_stats(blocks[0][1])
    # mul -> add3 -> (pad) -> dpp -> lshr: a run of three; med3 reads nothing lshr wrote, add reads v18 two back: no pair
    assert entry == {"instr": 8, "nops": 1, "wait_states": 2, "pairs": 3, "longest_run": 3}
    loop = dep_pairs.block_stats(blocks[1][1])
    # cmp -> (two pads) -> cndmask through vcc; cmp s[2:3] -> cmp s[28:29] is none; cmp s[28:29] -> cndmask s[2:3] is none;
    # cndmask -> mad, mad -> ds_write (v24), load v[4:7] -> add (v6)
    assert loop == {"instr": 11, "nops": 2, "wait_states": 3, "pairs": 4, "longest_run": 2}
    other = dep_pairs.kernel_blocks(KERNEL.splitlines(), "k_other")
    assert dep_pairs.block_stats(other[0][1])["pairs"] == 1


def test_command_line(tmp_path):
    f = tmp_path / "demo.s"
    f.write_text(KERNEL)
    out = subprocess.run([sys.executable, TOOL, str(f), "k_demo", "2"], check=True, capture_output=True, text=True).stdout
    lines = out.splitlines()
    assert lines[0] == "instructions 20 blocks 3"
    assert lines[1] == ".LBB0_1: 11 instr  s_nop 2 (3 wait states)  dependent pairs 4  longest run 2"
    assert lines[2] == "entry: 8 instr  s_nop 1 (2 wait states)  dependent pairs 3  longest run 3"
