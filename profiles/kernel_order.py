#!/usr/bin/env python3
"""Compare the kernel sequences of two rocprofv3 --kernel-trace runs: per queue, the kernel names in dispatch order.

    python profiles/kernel_order.py <trace dir or kernel_trace.csv of run A> <... of run B> [label]

Prints one line per queue (kernels, whether the two runs list the same names in the same order) and exits 1 on a
difference.  Queue ids are not stable between processes: queues are matched by their order of first dispatch."""
import csv
import glob
import os
import sys


def sequences(path):
    if os.path.isdir(path):
        found = sorted(glob.glob(os.path.join(path, "**", "*kernel_trace.csv"), recursive=True))
        if not found:
            raise SystemExit(f"no *kernel_trace.csv under {path}")
        path = found[0]
    rows = list(csv.DictReader(open(path)))
    rows.sort(key=lambda r: int(r["Dispatch_Id"]))
    queues = {}
    for r in rows:
        queues.setdefault(r["Queue_Id"], []).append(r["Kernel_Name"])
    return list(queues.values())            # dicts keep insertion order: queues by first dispatch


def main():
    a, b = sequences(sys.argv[1]), sequences(sys.argv[2])
    label = sys.argv[3] if len(sys.argv) > 3 else ""
    same = len(a) == len(b)
    print(f"{label}: {len(a)} / {len(b)} queues, {sum(map(len, a))} / {sum(map(len, b))} kernels")
    for i, (qa, qb) in enumerate(zip(a, b)):
        eq = qa == qb
        same = same and eq
        first = next((k for k, (u, v) in enumerate(zip(qa, qb)) if u != v), min(len(qa), len(qb)))
        print(f"  queue {i}: {len(qa)} / {len(qb)} kernels, " + ("same names in the same order" if eq else
              f"DIFFER from dispatch {first}: {qa[first:first + 1]} vs {qb[first:first + 1]}"))
    print(f"{label}: " + ("identical" if same else "DIFFERENT"))
    sys.exit(0 if same else 1)


if __name__ == "__main__":
    main()
