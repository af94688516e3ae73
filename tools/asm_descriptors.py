#!/usr/bin/env python3
"""Per-kernel table of two device-only assembly files (hipcc --offload-arch=gfx950 --cuda-device-only -S), parent against
branch: the descriptor's VGPRs (and the waves per SIMD they allow), private segment and LDS bytes, and opcode-prefix counts of
the kernel's body: global loads, global stores, global atomics, LDS instructions, all instructions.

    tools/asm_descriptors.py before.s after.s [--free SUBSTRING ...]  > table.md

Prints a markdown table, one row per kernel both sides have, `parent -> branch` where a figure moved, and under it the rows
that miss a bar: more VGPRs than the parent's occupancy step allows, a private segment, more LDS, or another count of memory
instructions.  A kernel whose demangled name holds a --free substring is reported without the bar on its counts.  Exit
status 1 when a row misses a bar."""
import argparse
import re
import subprocess
import sys

FUNC = re.compile(r"^\s*\.type\s+(\S+),@function")
KERNEL = re.compile(r"^\s*\.amdhsa_kernel\s+(\S+)")
FIELD = re.compile(r"^\s*\.amdhsa_(next_free_vgpr|private_segment_fixed_size|group_segment_fixed_size)\s+(\d+)")
OPCODE = re.compile(r"^\s+([a-z][a-z0-9_]+)(\s|$)")
COUNTS = (("gload", "global_load"), ("gstore", "global_store"), ("gatomic", "global_atomic"), ("lds", "ds_"))


def kernels(path):
    out, name, kd = {}, None, None
    with open(path, errors="replace") as f:
        for line in f:
            m = FUNC.match(line)
            if m:
                name = m.group(1)
                out.setdefault(name, {}).update({k: 0 for k, _ in COUNTS}, total=0)
                continue
            if name and line.startswith(".Lfunc_end"):
                name = None
                continue
            m = KERNEL.match(line)
            if m:
                kd = out.setdefault(m.group(1), {})
                continue
            if kd is not None:
                if ".end_amdhsa_kernel" in line:
                    kd = None
                    continue
                m = FIELD.match(line)
                if m:
                    kd[m.group(1)] = int(m.group(2))
                continue
            if name:
                m = OPCODE.match(line.split(";", 1)[0])
                if m:
                    out[name]["total"] += 1
                    for k, prefix in COUNTS:
                        out[name][k] += m.group(1).startswith(prefix)
    return {n: k for n, k in out.items() if "next_free_vgpr" in k}


def waves(vgprs):
    return min(8, 512 // max(8, (vgprs + 7) // 8 * 8))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("before")
    ap.add_argument("after")
    ap.add_argument("--free", action="append", default=[])
    a = ap.parse_args()
    A, B = kernels(a.before), kernels(a.after)
    names = sorted(set(A) & set(B))
    dem = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True).stdout.splitlines()

    def cell(x, y):
        return str(x) if x == y else "%d -> %d" % (x, y)

    print("| kernel | VGPRs | waves/SIMD | private | LDS bytes | global loads | global stores | global atomics | LDS instr. | instructions |")
    print("|---|---|---|---|---|---|---|---|---|---|")
    bad = []
    for n, d in zip(names, dem):
        p, b = A[n], B[n]
        d = d.replace("void ", "").replace("alacdev::", "")
        va, vb = p["next_free_vgpr"], b["next_free_vgpr"]
        print("| `%s` | %s |" % (d, " | ".join(
            [cell(va, vb), cell(waves(va), waves(vb)), cell(p["private_segment_fixed_size"], b["private_segment_fixed_size"]),
             cell(p["group_segment_fixed_size"], b["group_segment_fixed_size"])] +
            [cell(p[k], b[k]) for k, _ in COUNTS] + [cell(p["total"], b["total"])])))
        miss = []
        if waves(vb) < waves(va):
            miss.append("VGPRs")
        if b["private_segment_fixed_size"]:
            miss.append("private segment")
        if b["group_segment_fixed_size"] > p["group_segment_fixed_size"]:
            miss.append("LDS bytes")
        if not any(s in d for s in a.free):
            miss += [k for k, _ in COUNTS if p[k] != b[k]]
        if miss:
            bad.append("* `%s`: %s" % (d, ", ".join(miss)))
    print("\n%d kernels; only the parent has %d, only the branch %d.\n" % (len(names), len(set(A) - set(B)), len(set(B) - set(A))))
    print("Rows that miss a bar: %s" % ("none" if not bad else "\n\n" + "\n".join(bad)))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
