#!/usr/bin/env python3
"""Dump the kernel statistics of a rocprofv3 rocpd database (or --stats CSV dir) as a
markdown table: name, calls, total ms, average us, % -- the summary kept under profiles/."""

import sqlite3
import sys


def per_step(path, steps):
    """Only the library's kernels (rcfm::), as time per hot-path step: the traced process ran `steps` steps of the
    path (warm-up + profile pass + timed steps), so calls / steps = launches per step and total / steps = us per step.
    Input synthesis (torch, rocFFT) and the other configurations are left out."""
    db = sqlite3.connect(path)
    rows = [r for r in db.execute("select name, total_calls, total_duration, average from top_kernels") if "rcfm::" in r[0]]
    total = sum(r[2] for r in rows)
    print("rcfm:: kernels only; %d steps of the path in the traced process; sum = %.1f us per step" % (steps, total / steps))
    print()
    print("| kernel | launches per step | us per launch | us per step | % of the step |")
    print("|---|---:|---:|---:|---:|")
    for name, calls, tot, avg in rows:
        short = name.replace("(anonymous namespace)::", "").split("(")[0].replace("void ", "").replace("rcfm::fftk::", "").replace("rcfm::", "")
        if len(short) > 100:
            short = short[:97] + "..."
        print("| `%s` | %.2f | %.2f | %.1f | %.1f |" % (short, calls / steps, avg, tot / steps, 100.0 * tot / total))


def main(path, limit=40, only=None):
    db = sqlite3.connect(path)
    rows = list(db.execute("select name, total_calls, total_duration, average, percentage from top_kernels"))
    print("| kernel | calls | total ms | avg us | % |")
    print("|---|---:|---:|---:|---:|")
    for name, calls, total, avg, pct in rows[:limit]:
        if only and only not in name:
            continue
        short = name.replace("(anonymous namespace)::", "").split("(")[0].replace("void ", "")
        if len(short) > 110:
            short = short[:107] + "..."
        print("| `%s` | %d | %.3f | %.2f | %.2f |" % (short, calls, total / 1e3, avg, pct))


def launches(path, pattern, skip=0):
    """Per-launch durations of every kernel whose name contains `pattern` (without each kernel's first `skip` launches --
    warm-up): what a margin on a per-launch time is sized by."""
    db = sqlite3.connect(path)
    q = ("select S.display_name, (K.end - K.start) / 1000.0 from rocpd_kernel_dispatch K inner join rocpd_info_kernel_symbol S "
         "on S.id = K.kernel_id and S.guid = K.guid order by K.start")
    by = {}
    for name, us in db.execute(q):
        if pattern in name:
            by.setdefault(name, []).append(us)
    print("| kernel | launches | min us | median us | mean us | max us | spread (max - min) us |")
    print("|---|---:|---:|---:|---:|---:|---:|")
    for name, v in by.items():
        short = name.replace("(anonymous namespace)::", "").split("(")[0].replace("void ", "").replace("rcfm::fftk::", "").replace("rcfm::", "")
        if len(short) > 100:
            short = short[:97] + "..."
        s = sorted(v[skip:])
        print("| `%s` | %d | %.2f | %.2f | %.2f | %.2f | %.2f |" % (short, len(s), s[0], s[len(s) // 2], sum(s) / len(s), s[-1], s[-1] - s[0]))


if __name__ == "__main__":
    if len(sys.argv) > 3 and sys.argv[2] == "--launches":
        launches(sys.argv[1], sys.argv[3], int(sys.argv[4]) if len(sys.argv) > 4 else 0)
        sys.exit(0)
    if len(sys.argv) > 3 and sys.argv[2] == "--per-step":
        per_step(sys.argv[1], int(sys.argv[3]))
        sys.exit(0)
    main(sys.argv[1], int(sys.argv[2]) if len(sys.argv) > 2 else 40, sys.argv[3] if len(sys.argv) > 3 else None)
