#!/usr/bin/env python3
"""Step-boundary timeline from a rocprofv3 `--kernel-trace --stats` sqlite result (rocpd .db) of a bench.py run.

usage: python tools/step_timeline.py DIR/NAME_results.db [last_n_steps]

A step starts at its dcx_conv1_kernel (the detector's conv1a) and ends with its dcx_refine_finalize_kernel.  Per step:
  conv1a_us     duration of conv1a
  c1a_lead_us   how long BEFORE the previous step's last kernel ended this step's conv1a started (> 0: it ran beside that step)
  bubble_us     idle time between the end of the previous step's last kernel and the start of this step's first kernel that is
                not conv1a (conv1b) -- what the step boundary costs: conv1a if it is not hidden, launch gaps, the result copy
  period_us     finalize end to finalize end
  convs_us      summed duration of the step's dcx_conv_* launches (the matrix work conv1a may run beside)
Medians over the last N steps (default 20: the timed region of `--steps 20`) follow the table.
"""
import os
import sqlite3
import statistics
import sys


def main(path, last_n=20):
    db = sqlite3.connect(path)
    cur = db.cursor()
    cols = [r[1] for r in cur.execute("pragma table_info(kernels)")]
    name_col = "name" if "name" in cols else [c for c in cols if "name" in c][0]
    rows = list(cur.execute(f"select {name_col}, start, end from kernels order by start"))
    rows = [(n, s, e) for n, s, e in rows if n.startswith("dcx_") or "dcx_" in n]
    def is_front(n):
        return "dcx_conv1_kernel" in n or "dcx_conv1_tile_kernel" in n

    fronts = [(s, e) for n, s, e in rows if is_front(n)]
    finals = [(s, e) for n, s, e in rows if "dcx_refine_finalize" in n]
    rest = [(n, s, e) for n, s, e in rows if not is_front(n)]
    k = min(len(fronts), len(finals))
    fronts, finals = fronts[-k:], finals[-k:]
    steps = []
    for i in range(1, k):
        prev_end, this_end = finals[i - 1][1], finals[i][1]
        body = [(n, s, e) for n, s, e in rest if prev_end <= s < this_end]     # the step's kernels behind conv1a
        if not body:
            continue
        steps.append({"conv1a_us": (fronts[i][1] - fronts[i][0]) / 1e3, "c1a_lead_us": (prev_end - fronts[i][0]) / 1e3,
                      "bubble_us": (body[0][1] - prev_end) / 1e3, "period_us": (this_end - prev_end) / 1e3,
                      "convs_us": sum(e - s for n, s, e in body if "dcx_conv_" in n) / 1e3})
    steps = steps[-last_n:]
    keys = ["conv1a_us", "c1a_lead_us", "bubble_us", "period_us", "convs_us"]
    print(f"# step timeline of {os.path.basename(path)}: last {len(steps)} steps")
    print("# " + " ".join(f"{c:>12}" for c in ["step"] + keys))
    for i, st in enumerate(steps):
        print("  " + " ".join([f"{i:12d}"] + [f"{st[c]:12.1f}" for c in keys]))
    for c in keys:
        v = [st[c] for st in steps]
        if v:
            print(f"# {c:>12}: median {statistics.median(v):9.1f}  min {min(v):9.1f}  max {max(v):9.1f}")


if __name__ == "__main__":
    main(sys.argv[1], int(sys.argv[2]) if len(sys.argv) > 2 else 20)
