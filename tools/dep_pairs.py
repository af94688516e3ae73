#!/usr/bin/env python3
"""Dependent-neighbour and hazard-pad count per basic block of one kernel in a hipcc -S dump:
tools/dep_pairs.py FILE.s KERNEL_SUBSTR [top]

What a fixed instruction order is judged by (lms_step_lone, alac_lms.hpp; DESIGN 4.0 has what the two counts proved to be
worth on a wave that has its SIMD to itself: the pads their 4 cycles each, the dependent neighbours nothing).  Per block: instructions, s_nop count and their wait states (s_nop N = N + 1), adjacent pairs where the second
instruction reads a VGPR, an SGPR or vcc that the first writes (pads are skipped: the pair around a pad still counts), and
the longest run of such pairs."""
import re, sys

REG = re.compile(r"\b([vsa])(\d+)\b|\b([vsa])\[(\d+):(\d+)\]|\b(vcc|exec)(_lo|_hi)?\b")
# instructions without a destination operand: every operand is a source
NO_DST = ("s_nop", "s_waitcnt", "s_cbranch", "s_branch", "s_barrier", "s_endpgm", "s_sleep", "s_cmp", "s_bitcmp", "s_setprio",
          "ds_write", "buffer_wbl2", "buffer_inv", "s_sethalt")
VCC_CARRY_IN = ("v_cndmask_b32_e32", "v_cndmask_b32_sdwa", "v_cndmask_b32_dpp", "v_addc_co_u32_e32", "v_subb_co_u32_e32",
                "v_subbrev_co_u32_e32", "v_div_fmas")
VCC_OUT = ("v_addc_co_u32_e32", "v_subb_co_u32_e32", "v_subbrev_co_u32_e32", "v_add_co_u32_e32", "v_sub_co_u32_e32",
           "v_subrev_co_u32_e32")


def regs(text):
    """the registers an operand string names, as a set of (file, index); vcc and exec are ('vcc', 0) / ('exec', 0)"""
    out = set()
    for m in REG.finditer(text):
        if m.group(1):
            out.add((m.group(1), int(m.group(2))))
        elif m.group(3):
            out.update((m.group(3), i) for i in range(int(m.group(4)), int(m.group(5)) + 1))
        else:
            out.add((m.group(6), 0))
    return out


def split_operands(rest):
    """top-level comma split (brackets such as quad_perm:[1,0,3,2] and s[4:5] stay whole)"""
    parts, depth, cur = [], 0, ""
    for ch in rest:
        if ch in "[(":
            depth += 1
        elif ch in "])":
            depth -= 1
        if ch == "," and depth == 0:
            parts.append(cur.strip())
            cur = ""
        else:
            cur += ch
    if cur.strip():
        parts.append(cur.strip())
    return parts


def defs_uses(line):
    """(mnemonic, registers written, registers read) of one instruction line"""
    line = line.split(";")[0].strip()
    mnem, _, rest = line.partition(" ")
    mnem = mnem.strip()
    ops = split_operands(rest.replace("\t", " "))
    # modifiers after the last register operand (dst_sel:DWORD, row_mask:0xf, offset0:8 ...) name no registers
    if ops:
        ops[-1] = re.split(r"\s+(?=[a-z_0-9]+:)", ops[-1])[0]
    if mnem.startswith(NO_DST) or "_store" in mnem or not ops:  # (vector memory stores: address and data are sources)
        d, u = set(), set().union(*[regs(o) for o in ops]) if ops else set()
    else:
        ndst = 1
        # a VOP3 compare or carry-out names its scalar destination first; v_mad_u64_u32 and the _co_ forms name two
        if re.match(r"v_(mad_[ui]64_[ui]32|add_co|sub_co|subrev_co|addc_co|subb_co|subbrev_co)_?.*_e64|v_mad_[ui]64_[ui]32|v_div_scale", mnem):
            ndst = 2
        d = set().union(*[regs(o) for o in ops[:ndst]])
        u = set().union(*[regs(o) for o in ops[ndst:]]) if len(ops) > ndst else set()
    if mnem.startswith("v_cmp") and mnem.endswith(("_e32", "_sdwa")) and not (d & {("vcc", 0)}):
        # e32 compares write vcc implicitly: every operand is a source
        u |= {r for r in d if r != ("vcc", 0)}
        d = {("vcc", 0)}
    if mnem.startswith("v_cmpx"):
        d |= {("exec", 0)}
    if mnem.startswith(VCC_CARRY_IN):
        u.add(("vcc", 0))
    if mnem.startswith(VCC_OUT):
        d.add(("vcc", 0))
    if mnem.startswith("s_cbranch_vcc"):
        u.add(("vcc", 0))
    if mnem.startswith("s_cbranch_exec"):
        u.add(("exec", 0))
    if mnem.startswith(("s_cmp", "s_bitcmp")):
        d.add(("scc", 0))
    if mnem.startswith(("s_cbranch_scc", "s_cselect", "s_addc", "s_subb")):
        u.add(("scc", 0))
    return mnem, d, u


def kernel_blocks(lines, key):
    """[(block name, [instruction lines])] of the first kernel whose mangled name holds `key`"""
    start = next(i for i, l in enumerate(lines) if l.startswith("_Z") and key in l and ":" in l)
    end = next((i for i in range(start + 1, len(lines)) if lines[i].startswith(("\t.end_amdhsa_kernel", ".Lfunc_end"))), len(lines))
    blocks, cur, name = [], [], "entry"
    for l in lines[start + 1:end]:
        t = l.strip()
        m = re.match(r"^(\.LBB\d+_\d+):", l)
        if m:
            blocks.append((name, cur))
            cur, name = [], m.group(1)
            continue
        if not t or t.startswith((";", ".")):
            continue
        cur.append(t)
    blocks.append((name, cur))
    return blocks


def block_stats(instrs):
    """dict: instr, nops, wait_states, pairs, longest_run for one block's instruction lines"""
    nops = waits = pairs = run = longest = 0
    prev = None
    for t in instrs:
        mnem, d, u = defs_uses(t)
        if mnem == "s_nop":
            nops += 1
            waits += int(t.split()[1], 0) + 1
            continue  # a pad keeps the pair around it
        if prev is not None and (prev & u):
            pairs += 1
            run += 1
            longest = max(longest, run)
        else:
            run = 0
        prev = d
    return {"instr": len(instrs), "nops": nops, "wait_states": waits, "pairs": pairs, "longest_run": longest}


def main(argv):
    path, key = argv[1], argv[2]
    top = int(argv[3]) if len(argv) > 3 else 4
    blocks = kernel_blocks(open(path).read().splitlines(), key)
    print("instructions", sum(len(b) for _, b in blocks), "blocks", len(blocks))
    for name, b in sorted(blocks, key=lambda x: -len(x[1]))[:top]:
        s = block_stats(b)
        print(f"{name}: {s['instr']} instr  s_nop {s['nops']} ({s['wait_states']} wait states)  dependent pairs {s['pairs']}  longest run {s['longest_run']}")


if __name__ == "__main__":
    main(sys.argv)
