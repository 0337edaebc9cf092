#!/usr/bin/env python3
"""Instruction histogram of a kernel's device assembly, loop by loop.

    hipcc --offload-arch=gfx950 --cuda-device-only -S <unit's flags> unit.hip -o unit.s      (or the .s that the
    python3 isa_hist.py unit.s 'fused_mlp_res_kernel.*Lb0'                                   Makefile's -save-temps leaves)

For every kernel whose (mangled or demangled) name matches the pattern, the script finds the loops by their backward
branches (a branch whose target label stands earlier in the kernel), nests them by containment and prints, for each loop
and for the straight-line remainder of the kernel, how many vector, MFMA, LDS, memory and scalar instructions it holds
itself (instructions of a nested loop count for that loop only) and the histogram of their mnemonics.  The counts are
static: one execution of the loop body, every side of a forward branch included.

It is a diagnostic for reading the code around the hot loops (the zero-fills, conversions and address arithmetic a tile
pays once), not a build gate: isa_report.py holds the checks that fail a build.
"""
from __future__ import annotations

import argparse
import collections
import re
import subprocess
import sys

LABEL = re.compile(r"^([.\w$]+):")
INSN = re.compile(r"^\s+([a-z][a-z0-9_]+)(?:\s|$)")
BRANCH = re.compile(r"^\s+s_c?branch\w*\s+([.\w$]+)")
CLASSES = ("vector", "mfma", "lds", "mem", "scalar")


def classify(mn: str) -> str:
    if mn.startswith(("v_mfma", "v_smfmac")):
        return "mfma"
    if mn.startswith("v_"):
        return "vector"
    if mn.startswith("ds_"):
        return "lds"
    if mn.startswith(("global_", "buffer_", "flat_", "scratch_")):
        return "mem"
    return "scalar"


def demangle(names: list[str]) -> dict[str, str]:
    try:
        out = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True).stdout
        return dict(zip(names, out.splitlines()))
    except (OSError, subprocess.CalledProcessError):
        return {n: n for n in names}


def kernels(lines: list[str]) -> list[tuple[str, int, int]]:
    """(symbol, first line, line behind the last) of every kernel: from its label to its s_endpgm-terminated end marker."""
    amdhsa = {m.group(1) for l in lines if (m := re.match(r"^\s+\.amdhsa_kernel\s+(\S+)", l))}
    out = []
    for i, l in enumerate(lines):
        m = LABEL.match(l)
        if m and m.group(1) in amdhsa:
            end = next((j for j in range(i + 1, len(lines)) if lines[j].startswith(".Lfunc_end")), len(lines))
            out.append((m.group(1), i + 1, end))
    return out


def loops_of(body: list[str]) -> list[tuple[int, int]]:
    """[first, last] line index (inclusive) of every loop: header label .. its last backward branch."""
    label_at = {m.group(1): i for i, l in enumerate(body) if (m := LABEL.match(l))}
    span: dict[int, int] = {}
    for i, l in enumerate(body):
        m = BRANCH.match(l)
        if m and label_at.get(m.group(1), i + 1) <= i:
            h = label_at[m.group(1)]
            span[h] = max(span.get(h, i), i)
    return sorted(span.items())


def report(sym: str, pretty: str, body: list[str], top: int) -> None:
    loops = loops_of(body)
    # owner of a line: the innermost (shortest) loop that contains it, or -1
    owner = [-1] * len(body)
    for k, (a, b) in sorted(enumerate(loops), key=lambda t: -(t[1][1] - t[1][0])):
        for i in range(a, b + 1):
            owner[i] = k
    hist = collections.defaultdict(collections.Counter)
    for i, l in enumerate(body):
        m = INSN.match(l)
        if m and not l.lstrip().startswith((".", ";")):
            hist[owner[i]][m.group(1)] += 1

    def depth(k: int) -> int:
        a, b = loops[k]
        return sum(1 for (c, d) in loops if (c, d) != (a, b) and c <= a and b <= d)

    print(f"== {pretty}")
    print(f"   ({sym})")
    for k in [-1] + list(range(len(loops))):
        h = hist[k]
        tot = collections.Counter()
        for mn, n in h.items():
            tot[classify(mn)] += n
        if k < 0:
            head = "straight-line remainder"
        else:
            a, b = loops[k]
            head = f"loop {k} (depth {depth(k)}, header {LABEL.match(body[a]).group(1)}, {b - a + 1} lines)"
        print(f" {head}: " + "  ".join(f"{c} {tot[c]}" for c in CLASSES))
        for c in CLASSES:
            items = sorted(((n, mn) for mn, n in h.items() if classify(mn) == c), reverse=True)[:top]
            if items:
                print(f"     {c:7s}" + "  ".join(f"{mn} {n}" for n, mn in items))


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("asm", help="device assembly (.s) of one translation unit")
    ap.add_argument("pattern", help="regular expression searched in the mangled and the demangled kernel name")
    ap.add_argument("--top", type=int, default=12, help="mnemonics listed per class (default 12)")
    args = ap.parse_args()
    with open(args.asm) as f:
        lines = f.read().splitlines()
    ks = kernels(lines)
    pretty = demangle([k[0] for k in ks])
    pat = re.compile(args.pattern)
    found = 0
    for sym, a, b in ks:
        if pat.search(sym) or pat.search(pretty[sym]):
            report(sym, pretty[sym], lines[a:b], args.top)
            found += 1
    if not found:
        print(f"no kernel matches {args.pattern!r}; kernels of this file:", file=sys.stderr)
        for sym, _, _ in ks:
            print("   " + pretty[sym], file=sys.stderr)
        return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
