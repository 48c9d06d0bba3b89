#!/usr/bin/env python3
"""Compare two assembly listings of the kernels kernel by kernel: for every kernel name of the first file, is its text (the
.globl .. .Lfunc_end block and its .amdhsa descriptor) the same in the second?  Used to show that a change that must not alter
generated code (one that only adds kernels, or a refactor of shared device code) left every existing kernel alone.

The listings come from `make -C em-spec_amd/csrc asm` (the product build, kernels.s) and `make -C em-spec_amd/csrc asm-diag`
(the diagnostic build with its A/B form and stamped kernels, kernels_diag.s); compare like with like:

    python tools/kernel_isa_diff.py parent_kernels.s kernels.s
    python tools/kernel_isa_diff.py parent_kernels_diag.s kernels_diag.s
prints one line: "<n> kernels of A: <k> identical in B, <m> changed, <x> missing, <a> only in B", then a second comparison of
every kernel both files have, by its MNEMONIC SEQUENCE (each instruction cut to its opcode; labels kept; registers and
literal offsets dropped) together with its descriptor block:
    identical    the same text
    renamed      the same opcodes in the same order and the same descriptor: only register names / literals moved
    rescheduled  anything else (the instruction order, the instructions or the resources differ)
with a count of each, the names that are not identical, and for the rescheduled ones old -> new VGPR, SGPR, scratch and line
counts.  Exit 1 if any kernel changed or is missing.
"""
import re
import sys

_KERNEL = re.compile(r"^(\w+):\s*; @\1\n(.*?)^\.Lfunc_end\d+:", re.S | re.M)
_DESC = re.compile(r"^\s*\.amdhsa_kernel (\w+)\n(.*?)^\s*\.end_amdhsa_kernel", re.S | re.M)


def _norm(s):
    # basic blocks are numbered per file (.LBB<function>_<block>): a kernel added in front shifts the function number, and
    # the comments behind a label quote it (and are padded to a column): compare labels without it, and no comments
    return re.sub(r"BB\d+_", "BB_", re.sub(r"\s*;.*$", "", s, flags=re.M))


def kernels_text(text):
    out = {}
    # the body: from the symbol's label to its .Lfunc_end; the descriptor: its .amdhsa_kernel block
    for m in _KERNEL.finditer(text):
        out[m.group(1)] = [m.group(2)]
    for m in _DESC.finditer(text):
        if m.group(1) in out:
            out[m.group(1)].append(m.group(2))
    return {k: tuple(_norm(p) for p in v) for k, v in out.items()}


def kernels(path):
    return kernels_text(open(path).read())


def mnemonics(body):
    """The body's instruction lines cut to their opcode; label lines kept whole; empty lines dropped."""
    out = []
    for line in body.splitlines():
        line = line.strip()
        if line:
            out.append(line if line.endswith(":") else line.split()[0])
    return out


def classify(a, b):
    """a, b: one kernel's (body, descriptor) as kernels_text gives them."""
    if a == b:
        return "identical"
    if mnemonics(a[0]) == mnemonics(b[0]) and a[1:] == b[1:]:
        return "renamed"
    return "rescheduled"


def resources(k):
    """(next_free_vgpr, next_free_sgpr, private segment bytes, body lines) of one kernel."""
    desc = k[1] if len(k) > 1 else ""
    def field(name):
        m = re.search(r"\.amdhsa_" + name + r"\s+(\S+)", desc)
        return m.group(1) if m else "?"
    return (field("next_free_vgpr"), field("next_free_sgpr"), field("private_segment_fixed_size"), len(k[0].splitlines()))


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
    for k in added:
        print("only in B:", k)
    cls = {k: classify(a[k], b[k]) for k in a if k in b}
    count = lambda c: sum(1 for v in cls.values() if v == c)
    print(f"by mnemonic sequence + descriptor: {count('identical')} identical, {count('renamed')} renamed, "
          f"{count('rescheduled')} rescheduled")
    for k in sorted(cls):
        if cls[k] == "renamed":
            print("renamed:", k)
    for k in sorted(cls):
        if cls[k] == "rescheduled":
            ra, rb = resources(a[k]), resources(b[k])
            print(f"rescheduled: {k}  vgpr {ra[0]} -> {rb[0]}  sgpr {ra[1]} -> {rb[1]}  scratch {ra[2]} -> {rb[2]}  "
                  f"lines {ra[3]} -> {rb[3]}")
    return 1 if changed or missing else 0


if __name__ == "__main__":
    sys.exit(main())
