#!/usr/bin/env python3
"""Compare two `make asm` outputs (em-spec_amd/csrc/kernels.s) kernel by kernel: for every kernel name of the first file,
is its text (the .globl .. .Lfunc_end block and its .amdhsa descriptor) the same in the second?  Used to show that a change
which only ADDS kernels left every existing one alone.

    python tools/kernel_isa_diff.py parent_kernels.s kernels.s
prints one line: "<n> kernels of A: <k> identical in B, <m> changed, <a> only in B" and the names that changed; exit 1 if any.
"""
import re
import sys


def kernels(path):
    text = open(path).read()
    out = {}
    # the body: from the symbol's label to its .Lfunc_end; the descriptor: its .amdhsa_kernel block
    for m in re.finditer(r"^(\w+):\s*; @\1\n(.*?)^\.Lfunc_end\d+:", text, re.S | re.M):
        out[m.group(1)] = [m.group(2)]
    for m in re.finditer(r"^\s*\.amdhsa_kernel (\w+)\n(.*?)^\s*\.end_amdhsa_kernel", text, re.S | re.M):
        if m.group(1) in out:
            out[m.group(1)].append(m.group(2))
    # basic blocks are numbered per file (.LBB<function>_<block>): a kernel added in front shifts the function number, and
    # the comments behind a label quote it (and are padded to a column): compare labels without it, and no comments
    norm = lambda s: re.sub(r"BB\d+_", "BB_", re.sub(r"\s*;.*$", "", s, flags=re.M))
    return {k: tuple(norm(p) for p in v) for k, v in out.items()}


def main():
    a, b = kernels(sys.argv[1]), kernels(sys.argv[2])
    changed = sorted(k for k in a if k in b and a[k] != b[k])
    missing = sorted(k for k in a if k not in b)
    added = sorted(k for k in b if k not in a)
    same = len(a) - len(changed) - len(missing)
    print(f"{len(a)} kernels of A: {same} identical in B, {len(changed)} changed, {len(missing)} missing, {len(added)} only in B")
    for k in changed:
        print("changed:", k)
    for k in missing:
        print("missing:", k)
    return 1 if changed or missing else 0


if __name__ == "__main__":
    sys.exit(main())
