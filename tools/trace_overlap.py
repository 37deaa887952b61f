#!/usr/bin/env python3
"""trace_overlap — how much of a kernel trace runs concurrently.

Reads the kernel-trace CSV that `rocprofv3 --kernel-trace --output-format
csv` writes for ONE solo worker (columns Kernel_Name, Start_Timestamp,
End_Timestamp, in ns) and prints, per training step and as the mean over
the steps kept:

  sum      the sum of kernel durations
  union    the length of the union of the kernel intervals: the time the
           GPU was busy with at least one kernel
  and for every NAME given on the command line (substring of the kernel
  name): calls, their total time, and the part of that time during which
  some other kernel was running as well.

With kernels on more than one stream the sum rises by what overlaps;
the union, and the worker's wall time, are what count.

Steps: a step ends with the optimizer's kernel(s). A boundary is put
after every run of consecutive dispatches (in start order) whose name
contains --step-kernel; what follows the last boundary (an unfinished
step, teardown) is dropped, and --skip drops leading steps (set-up and
warm-up land in the first).

  python tools/trace_overlap.py out/123_kernel_trace.csv \\
      --skip 5 SubTensorOpWithScalar1d SubTensorOpWithCastTensor1d igemm_wrw
"""
from __future__ import annotations

import argparse
import bisect
import csv
import sys


def load(path):
    """[(name, start_ns, end_ns)] sorted by start."""
    rows = []
    with open(path, newline="") as f:
        for r in csv.DictReader(f):
            rows.append((r["Kernel_Name"], int(r["Start_Timestamp"]),
                         int(r["End_Timestamp"])))
    rows.sort(key=lambda r: (r[1], r[2]))
    return rows


def split_steps(rows, marker):
    """Split start-ordered rows after every run of dispatches whose name
    contains `marker`; rows after the last run are dropped."""
    steps, cur, in_run = [], [], False
    for r in rows:
        hit = marker in r[0]
        if in_run and not hit:
            steps.append(cur)
            cur = []
        cur.append(r)
        in_run = hit
    if in_run:
        steps.append(cur)
    return steps


def _covered(rows, depth):
    """Disjoint sorted [start, end) intervals where at least `depth`
    kernels run."""
    ev = []
    for _, s, e in rows:
        if e > s:
            ev.append((s, 1))
            ev.append((e, -1))
    ev.sort()  # at equal times -1 sorts first: touching is not overlap
    out, n, begin = [], 0, None
    for t, d in ev:
        was = n >= depth
        n += d
        if not was and n >= depth:
            begin = t
        elif was and n < depth:
            if out and out[-1][1] == begin:
                out[-1][1] = t
            else:
                out.append([begin, t])
    return out


def _inside(ivs, starts, s, e):
    """Length of [s, e) that lies in the disjoint sorted intervals."""
    tot = 0
    i = max(bisect.bisect_right(starts, s) - 1, 0)
    while i < len(ivs) and ivs[i][0] < e:
        tot += max(0, min(e, ivs[i][1]) - max(s, ivs[i][0]))
        i += 1
    return tot


def analyse(rows, names):
    """{"dispatches", "sum", "union", "names": {name: {"calls", "total",
    "overlapped"}}}, times in ns. A kernel's overlapped part is where at
    least one OTHER kernel runs, i.e. where two or more kernels run."""
    busy = _covered(rows, 1)
    multi = _covered(rows, 2)
    mstarts = [iv[0] for iv in multi]
    per = {n: {"calls": 0, "total": 0, "overlapped": 0} for n in names}
    for name, s, e in rows:
        for n in names:
            if n in name:
                per[n]["calls"] += 1
                per[n]["total"] += e - s
                per[n]["overlapped"] += _inside(multi, mstarts, s, e)
    return {"dispatches": len(rows),
            "sum": sum(e - s for _, s, e in rows),
            "union": sum(b - a for a, b in busy),
            "names": per}


def _fmt(tag, a, names):
    us = 1e-3
    line = (f"{tag:>6} dispatches {a['dispatches']:8.1f}  sum "
            f"{a['sum'] * us:10.1f} us  union {a['union'] * us:10.1f} us  "
            f"overlapped {(a['sum'] - a['union']) * us:9.1f} us")
    for n in names:
        p = a["names"][n]
        line += (f"\n         {n}: calls {p['calls']:.1f}  total "
                 f"{p['total'] * us:.1f} us  of it beside another kernel "
                 f"{p['overlapped'] * us:.1f} us")
    return line


def mean(results, names):
    k = float(len(results))
    return {"dispatches": sum(r["dispatches"] for r in results) / k,
            "sum": sum(r["sum"] for r in results) / k,
            "union": sum(r["union"] for r in results) / k,
            "names": {n: {f: sum(r["names"][n][f] for r in results) / k
                          for f in ("calls", "total", "overlapped")}
                      for n in names}}


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("csv", help="kernel-trace CSV of one solo worker")
    ap.add_argument("names", nargs="*",
                    help="kernel-name substrings to report on")
    ap.add_argument("--step-kernel", default="sgd_mom",
                    help="substring of the kernel(s) that end a step")
    ap.add_argument("--skip", type=int, default=0,
                    help="leading steps to drop (set-up, warm-up)")
    ap.add_argument("--quiet", action="store_true",
                    help="print the mean only, not every step")
    # (names may follow the options: the docstring's own example)
    args = ap.parse_intermixed_args(argv)
    steps = split_steps(load(args.csv), args.step_kernel)[args.skip:]
    if not steps:
        print(f"no step found: no kernel named *{args.step_kernel}* "
              f"(after --skip {args.skip})", file=sys.stderr)
        return 1
    results = [analyse(s, args.names) for s in steps]
    if not args.quiet:
        for i, a in enumerate(results):
            print(_fmt(str(i + args.skip), a, args.names))
    print(_fmt("mean", mean(results, args.names), args.names))
    print(f"({len(results)} steps)")
    return 0


if __name__ == "__main__":
    sys.exit(main())
