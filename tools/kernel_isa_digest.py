#!/usr/bin/env python3
"""tools/kernel_isa_digest.py FILE.s -- one line per kernel of a gfx950 assembly file: `digest  n_instructions  name`.

FILE.s is what `hipcc <flags of csrc/build.sh> -save-temps=obj -c X.hip` leaves as X-hip-amdgcn-amd-amdhsa-gfx950.s.  A kernel's digest
covers its instruction lines (comments stripped; local labels .LBB<n>_<m> without <n>, the function's number in the file) and its
.amdhsa_* resource block, so two builds whose outputs `diff` empty run the same device code with the same registers, LDS and scratch:
the check a host-only change of a .hip file has to pass.  Sorted by name; a kernel that is missing or new shows up in the diff as well.

profiles/raster_isa_digest.txt is this tool's output for csplat_raster.hip (with its parts, csrc/csplat_raster_*.h) as committed, under two
`#` heading lines that name the commit and the flags: a change that must not touch device code diffs its own output against that file
(`grep -v "^#"`) instead of rebuilding its parent, and a change that does touch it commits the new listing.
"""
import hashlib
import re
import sys

LOCAL = re.compile(r"\.L(BB|JTI|func_end|func_begin)\d+")


def kernels(path):
    lines = open(path).read().splitlines()
    start = {}                                       # label -> index of the line behind it
    for i, ln in enumerate(lines):
        m = re.match(r"^([A-Za-z_$][\w$.]*):", ln)
        if m:
            start[m.group(1)] = i + 1
    out = []
    for i, ln in enumerate(lines):
        m = re.match(r"^\s*\.amdhsa_kernel\s+(\S+)", ln)
        if not m:
            continue
        name = m.group(1)
        res = []
        for r in lines[i + 1:]:
            if ".end_amdhsa_kernel" in r:
                break
            res.append(" ".join(r.split()))
        code = []
        for c in lines[start[name]:]:
            c = c.split(";", 1)[0].strip()
            if c.startswith(".Lfunc_end"):
                break
            if not c or (c.startswith(".") and not c.startswith(".LBB")):
                continue                             # directives (.p2align, .section ...) are not instructions
            code.append(LOCAL.sub(lambda t: ".L" + t.group(1), " ".join(c.split())))
        n = sum(1 for c in code if not c.endswith(":"))
        h = hashlib.sha256("\n".join(code + ["--"] + res).encode()).hexdigest()[:16]
        out.append((name, h, n))
    return sorted(out)


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    for name, h, n in kernels(sys.argv[1]):
        print(h, "%7d" % n, name)
