#!/usr/bin/env python3
"""Compare the kernels of two builds by their instruction streams.

    python tools/isa_kernel_bodies.py OLD_DIR NEW_DIR [file.isa.s ...]

OLD_DIR and NEW_DIR hold the device listings the Makefile leaves next to the objects (build/<file>.isa.s).  A kernel's body is the text between its entry label
and its .Lfunc_end label, with the function index taken out of the local labels (.LBB12_3 -> .LBB_3: the index counts the functions in front, not the code) and
comment-only lines dropped.  For every listing the script prints how many kernels of OLD_DIR exist in NEW_DIR with the same body - under the same mangled name,
or, where a kernel gained template parameters and so another name, under the one new name that starts like the old one up to the kernel's source name -, names
every kernel that changed or disappeared, and counts the kernels that are new.  It compares instructions only: a kernel's descriptor (register counts, kernarg
size) is metadata behind the body.  Exit status 1 if a kernel of OLD_DIR changed or is gone.
(tools/isa_kernel_diff.py compares named kernels of two listings and can mask moved kernel-argument offsets; this one walks whole build directories and finds the
renamed twins itself.)
"""
from __future__ import annotations

import hashlib
import os
import re
import sys


def kernel_bodies(path: str) -> dict:
    kernels = set()
    text = open(path).read()
    for m in re.finditer(r"^\s*\.amdhsa_kernel\s+(\S+)", text, re.M):
        kernels.add(m.group(1))
    bodies, name, lines = {}, None, []
    for line in text.split("\n"):
        if name is None:
            m = re.match(r"^([A-Za-z_$][\w$.]*):", line)
            if m and m.group(1) in kernels:
                name, lines = m.group(1), []
            continue
        if re.match(r"^\s*(\.Lfunc_end\d+:|\.section|\.rodata|\.p2align\s+6)", line):
            bodies[name] = "\n".join(lines)
            name = None
            continue
        s = line.strip()
        if not s or s.startswith(";"):
            continue
        lines.append(re.sub(r"\.LBB\d+_", ".LBB_", re.sub(r"\s*;.*$", "", line)).replace(name, "<this kernel>"))
    return bodies


def main() -> int:
    if len(sys.argv) < 3:
        print(__doc__)
        return 2
    old_dir, new_dir = sys.argv[1], sys.argv[2]
    files = sys.argv[3:] or sorted(f for f in os.listdir(old_dir) if f.endswith(".isa.s"))
    bad = 0
    for f in files:
        old, new = kernel_bodies(os.path.join(old_dir, f)), kernel_bodies(os.path.join(new_dir, f))
        same, changed, gone, renamed = [], [], [], {}
        for k in old:
            if k in new:
                (same if old[k] == new[k] else changed).append(k)
                continue
            # a kernel that gained template parameters keeps its mangled name up to the end of its source name ("..._kernel")
            stem = k[: k.find("kernel") + len("kernel")] if "kernel" in k else k
            twins = [n for n in new if n not in old and n not in renamed.values() and n.startswith(stem) and new[n] == old[k]]
            if len(twins) == 1:
                renamed[k] = twins[0]
                same.append(k)
            else:
                gone.append(k)
        added = [k for k in new if k not in old and k not in renamed.values()]
        digest = hashlib.sha256("\n".join(k + "\n" + old[k] for k in sorted(same)).encode()).hexdigest()[:16]
        print("%-24s %3d kernels, %3d identical (sha256 of their bodies %s), %d changed, %d gone, %d new" % (f, len(old), len(same), digest, len(changed), len(gone), len(added)))
        for k, n in renamed.items():
            print("    same body, renamed", k, "->", n)
        for k in changed:
            print("    CHANGED", k)
        for k in gone:
            print("    GONE   ", k)
        bad += len(changed) + len(gone)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
