#!/usr/bin/env python3
"""Who runs beside whom: reads the per-dispatch start / end times of a rocprofv3 --kernel-trace (csv) and reports

  * per triage_classify_kernel dispatch, the share of its run time that lies inside a realign_kernel dispatch of ANOTHER queue,
    and the dispatch's duration as a function of that share -- and the same for realign against classify;
  * the idle time between consecutive dispatches of one queue (a HIP stream keeps its hardware queue, so a queue stands for a stream;
    the trace of a replayed graph carries no stream id of its own).

    rocprofv3 --kernel-trace --output-format csv -d DIR -- python bench.py
    python profiles/dispatch_overlap.py DIR [tag]

The trace is taken on its own: no --pmc, no other tracing.  The first and last tenth of the dispatches (set-up, warm-up, drain) are
left out.  Times under the tracer are longer than the headline's (every dispatch is bracketed); read them as shares."""
import bisect
import csv
import glob
import os
import sys

BUCKETS = [(0.0, 0.05), (0.05, 0.25), (0.25, 0.5), (0.5, 0.75), (0.75, 0.95), (0.95, 1.0001)]


def load(d):
    paths = [d] if os.path.isfile(d) else sorted(glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True))
    rows = []
    for p in paths:
        with open(p, newline="") as f:
            for r in csv.DictReader(f):
                rows.append((r["Kernel_Name"], r.get("Queue_Id", "0"), int(r["Start_Timestamp"]), int(r["End_Timestamp"])))
    rows.sort(key=lambda r: r[2])
    return rows


def union(iv):
    """sorted, disjoint intervals covering the same time as iv"""
    out = []
    for s, e in sorted(iv):
        if out and s <= out[-1][1]:
            out[-1][1] = max(out[-1][1], e)
        else:
            out.append([s, e])
    return out


def covered(u, starts, s, e):
    """ns of [s, e) inside the disjoint sorted intervals u"""
    k = max(bisect.bisect_right(starts, s) - 1, 0)
    tot = 0
    while k < len(u) and u[k][0] < e:
        tot += max(0, min(e, u[k][1]) - max(s, u[k][0]))
        k += 1
    return tot


def beside(rows, mine, other, out):
    """duration of `mine` dispatches against the share of their run time inside `other` dispatches of another queue"""
    queues = sorted({q for _, q, _, _ in rows})
    per_q = {}
    for q in queues:       # what the other queues run of `other`, for a dispatch of queue q
        u = union([(s, e) for n, qq, s, e in rows if other in n and qq != q])
        per_q[q] = (u, [x[0] for x in u])
    got = []
    for n, q, s, e in rows:
        if mine in n and e > s:
            u, st = per_q[q]
            got.append((covered(u, st, s, e) / (e - s), (e - s) / 1e3))
    out.append("%s: %d dispatches, mean %.1f us; run time inside a %s dispatch of another queue: mean share %.2f"
               % (mine, len(got), sum(d for _, d in got) / max(len(got), 1), other, sum(f for f, _ in got) / max(len(got), 1)))
    out.append("  share inside      dispatches   mean us   median us")
    for lo, hi in BUCKETS:
        ds = sorted(d for f, d in got if lo <= f < hi)
        if ds:
            out.append("  %.2f - %.2f       %8d   %7.1f   %7.1f" % (lo, min(hi, 1.0), len(ds), sum(ds) / len(ds), ds[len(ds) // 2]))
    return got


def main():
    d = sys.argv[1]
    tag = sys.argv[2] if len(sys.argv) > 2 else ""
    rows = load(d)
    cut = len(rows) // 10
    rows = rows[cut:len(rows) - cut]
    out = ["%s %d dispatches in the window, %.1f ms" % (tag, len(rows), (rows[-1][3] - rows[0][2]) / 1e6)]
    n_step = sum(1 for n, _, _, _ in rows if "triage_classify_kernel" in n)
    out.append("classify dispatches (= steps) %d: %.1f us of wall time per step under the tracer" % (n_step, (rows[-1][3] - rows[0][2]) / 1e3 / max(n_step, 1)))
    beside(rows, "triage_classify_kernel", "realign_kernel", out)
    beside(rows, "realign_kernel", "triage_classify_kernel", out)
    # kernel time per step, by kernel
    tot = {}
    for n, _, s, e in rows:
        k = n.replace("(anonymous namespace)::", "").replace("void ", "").split("(")[0]
        tot[k] = tot.get(k, 0) + (e - s)
    out.append("kernel time per step, us:")
    for k, v in sorted(tot.items(), key=lambda kv: -kv[1]):
        out.append("  %-60s %7.1f" % (k[:60], v / 1e3 / max(n_step, 1)))
    # idle time between consecutive dispatches of one queue
    out.append("idle between consecutive dispatches of one queue:")
    for q in sorted({q for _, q, _, _ in rows}):
        mine = [(s, e) for _, qq, s, e in rows if qq == q]
        gaps = sorted(max(0, mine[k + 1][0] - mine[k][1]) / 1e3 for k in range(len(mine) - 1))
        if gaps:
            span = (mine[-1][1] - mine[0][0]) / 1e3
            out.append("  queue %s: %d dispatches, idle %.1f %% of its span; gap mean %.2f us, median %.2f, 90th percentile %.2f"
                       % (q, len(mine), 100.0 * sum(gaps) / span, sum(gaps) / len(gaps), gaps[len(gaps) // 2], gaps[len(gaps) * 9 // 10]))
    print("\n".join(out))


if __name__ == "__main__":
    main()
