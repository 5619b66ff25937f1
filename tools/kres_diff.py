#!/usr/bin/env python3
"""Two builds of one kernel source, kernel by kernel, from their gfx950 assembly (tools/kres.py
--save-asm, or hipcc --cuda-device-only -S).  Not product code.

    python tools/kres_diff.py PARENT.s NEW.s

Reads only each kernel's instruction stream (comments, labels and directives stripped) and the
resource comments after it.  Prints, parent | new: instructions, NumVgprs, NumAgprs, TotalNumSgprs,
ScratchSize, LDSByteSize, Occupancy, and whether the two streams are identical.  Exits 1 when the
two builds do not define the same kernel symbols.
"""

from __future__ import annotations

import re
import sys

from kres import demangle

FIELDS = ("NumVgprs", "NumAgprs", "TotalNumSgprs", "ScratchSize", "LDSByteSize", "Occupancy")


def kernels(path: str) -> dict:
    """symbol -> (instruction lines, {field: value})"""
    out, sym, body, res = {}, None, None, None
    for ln in open(path):
        m = re.match(r"(_Z\w+):", ln)
        if m:
            sym, body, res = m.group(1), [], {}
            out[sym] = (body, res)
            continue
        if sym is None:
            continue
        t = ln.split(";", 1)[0].strip()
        if body is not None:
            if t.startswith((".section", ".amdhsa_kernel")):
                body = None  # the kernel descriptor follows the code
            elif t and not t.startswith(".") and not re.fullmatch(r"[\w.$]+:", t):
                # (a branch target keeps its block number, not the function's position in the file,
                # and a long branch's anchor label no number: it counts the file's long branches)
                t = re.sub(r"\.LBB\d+_", ".LBB_", " ".join(t.split()))
                out[sym][0].append(re.sub(r"\.Lpost_getpc\d+", ".Lpost_getpc", t))
            continue
        m = re.match(r"; (\w+): (\d+)", ln)
        if m and m.group(1) in FIELDS:
            res[m.group(1)] = int(m.group(2))
            if m.group(1) == "Occupancy":
                sym = None
    return out


def main():
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    a, b = kernels(sys.argv[1]), kernels(sys.argv[2])
    print(f"{'kernel (parent | new)':44s} {'insts':>13s} " + " ".join(f"{f[:9]:>9s}" for f in FIELDS) + "  stream")
    same = 0
    for sym in sorted(set(a) & set(b), key=demangle):
        (ia, ra), (ib, rb) = a[sym], b[sym]
        ident = ia == ib
        same += ident
        cols = " ".join(f"{str(ra.get(f, '?')) + '|' + str(rb.get(f, '?')):>9s}" for f in FIELDS)
        print(f"{demangle(sym):44s} {str(len(ia)) + '|' + str(len(ib)):>13s} {cols}  "
              + ("identical" if ident else f"differs ({len(ib) - len(ia):+d})"))
    for sym in sorted(set(a) ^ set(b), key=demangle):
        print(f"{demangle(sym):44s} only in {'parent' if sym in a else 'new'}")
    print(f"{len(a)} | {len(b)} kernels, {len(set(a) & set(b))} in both, {same} identical")
    sys.exit(0 if set(a) == set(b) else 1)


if __name__ == "__main__":
    main()
