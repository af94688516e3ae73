#!/usr/bin/env python3
"""Compare two device-only assembly files (hipcc --offload-arch=gfx950 --cuda-device-only -S) function by function.

    tools/asm_compare.py before.s after.s [mangled-argument ...]

A kernel that gained a trailing argument, or whose argument's type was renamed, has another mangled name: give the argument's
mangling (NS_11PcmModeArgsE for alacdev::PcmModeArgs; both spellings for a rename) and it is dropped from every name before
the two sides are matched.

Labels are renumbered by order of first appearance and comments dropped, so that a function whose code did not move compares
equal whatever was added around it.  Prints the functions only one side has, the ones whose bodies differ (with the count of
differing lines, and whether every difference is the offset of a scalar load from the kernel-argument segment), and a
summary.  Exit status 1 when a function both sides have differs in more than kernel-argument offsets."""
import re
import sys

DROP = []
FUNC = re.compile(r"^\s*\.type\s+(\S+),@function")
LABEL = re.compile(r"\.L[A-Za-z_]*\d+(?:_\d+)?")
# a scalar load from the kernel-argument segment, or the address of the hidden arguments behind the explicit ones
KERNARG = re.compile(r"^(\s*(?:s_load_\w+\s+\S+\s+s\[\d+:\d+\]|s_add_u32\s+s\d+,\s*s\d+),\s*)(0x[0-9a-f]+|\d+)\s*$")


def functions(path):
    out, name, body = {}, None, []
    with open(path, errors="replace") as f:
        for line in f:
            m = FUNC.match(line)
            if m:
                name, body = m.group(1), []
                for d in DROP:
                    name = name.replace(d, "")
                continue
            if name is None:
                continue
            if line.startswith(".Lfunc_end"):
                out[name] = normalise(body)
                name = None
                continue
            body.append(line)
    return out


def normalise(body):
    names = {}

    def renumber(m):
        return names.setdefault(m.group(0), ".L%d" % len(names))

    lines = []
    for line in body:
        line = line.split(";", 1)[0].rstrip()
        for d in DROP:
            line = line.replace(d, "")
        # the kernel descriptor's argument-segment size follows the argument list, not the code
        if not line.strip() or line.strip().startswith((".p2align", ".globl", ".protected", ".weak", ".section", ".hidden",
                                                        ".amdhsa_kernarg_size")):
            continue
        lines.append(LABEL.sub(renumber, line))
    return lines


def main(a, b):
    fa, fb = functions(a), functions(b)
    gone, new = sorted(set(fa) - set(fb)), sorted(set(fb) - set(fa))
    same = offsets = 0
    moved = []
    for name in sorted(set(fa) & set(fb)):
        x, y = fa[name], fb[name]
        if x == y:
            same += 1
            continue
        if len(x) == len(y):
            diff = [(p, q) for p, q in zip(x, y) if p != q]
            if all(KERNARG.match(p) and KERNARG.match(q) and KERNARG.match(p).group(1) == KERNARG.match(q).group(1) for p, q in diff):
                offsets += 1
                print("kernel-argument offsets only (%d loads): %s" % (len(diff), name))
                continue
            moved.append((name, len(diff)))
        else:
            moved.append((name, abs(len(x) - len(y))))
    for name in gone:
        print("only in %s: %s" % (a, name))
    for name, n in moved:
        print("BODY DIFFERS (%d lines): %s" % (n, name))
    print("%d functions in both: %d identical, %d differ in kernel-argument offsets only, %d differ otherwise; %d new, %d gone"
          % (len(set(fa) & set(fb)), same, offsets, len(moved), len(new), len(gone)))
    return 1 if moved else 0


if __name__ == "__main__":
    DROP[:] = sys.argv[3:]
    sys.exit(main(sys.argv[1], sys.argv[2]))
