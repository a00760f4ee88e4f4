"""depth_median_kernel (im_depth.hip) next to the sum query on the same intervals.

One contig of 6.25 Mb at the depth of configs[1] (30x of 100-base reads, as host-given intervals through im_depth_build; the
genome-wide form launches the same kernel on the same layout).  Two query sets, each timed as whole calls (copies in, one
launch, copy out, one wait -- what print_variants pays):
  flush   3 x 300 queries shaped like a flush's: insides of 50 .. 5000 bases with their two 1000-base flanks
  long    3 x 20 queries with insides of 100 kb .. 1 Mb
and next to each im_depth_query on the same intervals: that kernel reads the same bytes.  Both are times of WHOLE CALLS, not of
kernels: the median's call also numbers the slabs on the host and copies two more small arrays in ("call_ratio").  The
host-buffer entries stand in for im_depth_median_tid / im_depth_query_tid, which launch the same two kernels on the same layout
from other base pointers and would need a record stream to fill the array.

    python profiles/depth_median_probe.py [--reps 20]
prints one JSON line.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

CLEN = 6_250_000
FLANK = 1000


def triples(rng, n, lo, hi):
    pos = rng.integers(FLANK, CLEN - hi - FLANK, n)
    end = pos + rng.integers(lo, hi + 1, n)
    beg = np.stack([pos, pos - FLANK, end], 1).reshape(-1)
    stop = np.stack([end, pos, end + FLANK], 1).reshape(-1)
    return beg.astype(np.int32), stop.astype(np.int32)


def timed(fn, beg, end, reps):
    fn(beg, end)
    ts = []
    for _ in range(reps):
        t = time.perf_counter()
        fn(beg, end)
        ts.append((time.perf_counter() - t) * 1e6)
    ts.sort()
    return {"median_us": round(ts[len(ts) // 2], 1), "min_us": round(ts[0], 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()
    from indelminer_amd import capi
    rng = np.random.default_rng(1)
    n_reads = 30 * CLEN // 100
    start = np.sort(rng.integers(0, CLEN - 100, n_reads)).astype(np.int32)
    ctx = capi.Context(0)
    ctx.depth_build(CLEN, start, np.full(n_reads, 100, np.int32))
    out = {"contig": CLEN, "depth": 30, "reps": a.reps, "lds_form": "per-lane runs of equal neighbours, no combination across lanes"}
    for name, (n, lo, hi) in {"flush": (300, 50, 5000), "long": (20, 100_000, 1_000_000)}.items():
        beg, end = triples(rng, n, lo, hi)
        positions = int((np.minimum(end, CLEN) - np.maximum(beg, 0)).sum())
        out[name] = {"queries": len(beg), "positions": positions,
                     "median": timed(ctx.depth_median, beg, end, a.reps), "sum": timed(ctx.depth_query, beg, end, a.reps)}
        out[name]["call_ratio"] = round(out[name]["median"]["median_us"] / out[name]["sum"]["median_us"], 2)
    ctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
