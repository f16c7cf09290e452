#!/usr/bin/env python3
"""Compare kernels of two device listings (build/<file>.isa.s) instruction by instruction.

    tools/isa_kernel_diff.py PARENT.isa.s TREE.isa.s kernel_name [kernel_name ...]

A kernel is every symbol whose demangled-free name contains `kernel_name` (all template instantiations).  A symbol of the tree is paired with
the parent's symbol of the same name, or - where a template gained a trailing parameter - with the parent's name once `--drop-arg TEXT` is removed from
the tree's (e.g. `Li0EEEv` -> `EEEv` for a new trailing `int = 0`).  Bodies are compared after comments, labels' numbers and the symbol names themselves are
taken out; `--ignore-kernarg-offsets` also masks the immediate offsets of scalar loads from the kernel argument pointer (s[0:1] .. s[4:5]), which move
when a parameter struct grows.  Prints one line per kernel: instructions, md5 of the normalised body on each side, equal / DIFFERENT - or, where the bodies differ but
the sequence of mnemonics is the same once scalar loads, waits and no-ops are left out, "same-operations": a weaker statement that compares no operand."""
import argparse
import hashlib
import re
import sys


def bodies(path):
    out, name, cur = {}, None, []
    for line in open(path):
        m = re.match(r"^(_Z\w+):\s*(;.*)?$", line)
        if m and name is None:
            name, cur = m.group(1), []
            continue
        if name is not None:
            if line.startswith(".Lfunc_end"):
                out[name] = cur
                name = None
                continue
            cur.append(line)
    return out


def normalise(lines, name, mask_kernarg):
    res = []
    for line in lines:
        line = line.split(";")[0].rstrip()
        if not line.strip() or line.strip().startswith("."):
            if not re.match(r"^\.LBB", line.strip()):
                continue
        line = line.replace(name, "KERNEL")
        line = re.sub(r"\.LBB\d+_", ".LBB_", line)
        if mask_kernarg and re.match(r"^\s*s_load_dword", line) and re.search(r"s\[[0-9]+:[0-9]+\], (0x[0-9a-f]+|\d+)\s*$", line):
            line = re.sub(r"(0x[0-9a-f]+|\d+)\s*$", "OFF", line)
        # the pointer to the implicit arguments behind the explicit ones: kernarg pointer + their size
        if mask_kernarg and re.match(r"^\s*s_add_u32 s\d+, s[0-9]+, 0x[0-9a-f]+\s*$", line):
            line = re.sub(r"0x[0-9a-f]+\s*$", "OFF", line)
        res.append(line.strip())
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("parent")
    ap.add_argument("tree")
    ap.add_argument("kernels", nargs="+")
    ap.add_argument("--drop-arg", action="append", default=[], help="OLD=NEW: text replaced in a tree symbol to find its parent symbol")
    ap.add_argument("--ignore-kernarg-offsets", action="store_true")
    a = ap.parse_args()
    pb, tb = bodies(a.parent), bodies(a.tree)
    bad = 0
    for k in a.kernels:
        for tname in sorted(n for n in tb if k in n):
            pname = tname if tname in pb else None
            for d in a.drop_arg:
                old, new = d.split("=")
                if pname is None and tname.replace(old, new) in pb:
                    pname = tname.replace(old, new)
            if pname is None:
                continue                                           # an instantiation the parent does not have: new code
            p = normalise(pb[pname], pname, a.ignore_kernarg_offsets)
            t = normalise(tb[tname], tname, a.ignore_kernarg_offsets)
            hp, ht = (hashlib.md5("\n".join(x).encode()).hexdigest() for x in (p, t))
            same = p == t
            verdict = "equal" if same else "DIFFERENT"
            if not same:                                           # a weaker verdict: the same sequence of mnemonics (operands, registers and immediates NOT compared) behind differently merged argument loads
                ops = [[x.split()[0] for x in side if not x.startswith(("s_load_dword", ".LBB", "s_waitcnt", "s_nop"))] for side in (p, t)]
                loads = [sum(x.startswith("s_load_dword") for x in side) for side in (p, t)]
                if ops[0] == ops[1]:
                    same, verdict = True, f"same-operations (mnemonic sequence only, operands not compared; kernel-argument loads {loads[0]} -> {loads[1]})"
            bad += not same
            print(f"{tname} {len(p)} {len(t)} {hp} {ht} {verdict}")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
