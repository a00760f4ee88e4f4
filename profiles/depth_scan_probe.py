#!/usr/bin/env python3
"""depth_scan_tiled_kernel alone: im_depth_scan on a genome-wide depth array that was reset to zeros and then fed a few
thousand randomly placed reads by the triage's scatter, timed with HIP events around the scan(s) on a drained stream.
Twelve launches per shape, the first dropped.  Shapes: one contig of n = 1 000 001 entries, one of 6 250 001, and the
genome-wide form, eight contigs of 6 250 001 scanned back to back on one stream (eight launches in one timed window).

The scan reads and writes every entry once: bytes = 8 n.  `x_copy` is the time over bytes / the device-to-device copy rate
measured in the same process (bench.copy_peak_gbs, the figure bench.py reports as peak_measured_copy_gbs).

    python profiles/depth_scan_probe.py
    rocprofv3 --kernel-trace --stats -d <dir> -- python profiles/depth_scan_probe.py
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from indelminer_amd import capi  # noqa: E402
from tests.support.matchrecs import match_records  # noqa: E402

LAUNCHES = 12
SHAPES = [("1Mb", [1_000_000]), ("6.25Mb", [6_250_000]), ("8x6.25Mb", [6_250_000] * 8)]


def run(name, clens, copy_gbs):
    rng = np.random.default_rng(3)
    ctx = capi.Context(0)
    ctx.set_reference([b"A" * n for n in clens])
    ctx.set_insert_ranges(["generic"], [700])
    ctx.depth_enable()
    tid = np.repeat(np.arange(len(clens)), 4000)
    pos = np.concatenate([np.sort(rng.integers(0, n, 4000)) for n in clens])
    raw, off = match_records(tid, pos)
    pipe = capi.Pipeline(ctx, len(off) - 1, len(raw), cap_cand=len(off) - 1, want_depth=True)
    pipe.upload(raw, off)
    L = capi.lib()
    t = capi.Timer(ctx)
    us = []
    for _ in range(LAUNCHES):
        for k in range(len(clens)):
            ctx._check(L.im_depth_reset(ctx.h, k, ctx.stream))
        pipe.triage()
        pipe.sync()
        t.start(ctx.stream)
        for k in range(len(clens)):
            ctx._check(L.im_depth_scan(ctx.h, k, ctx.stream))
        t.stop(ctx.stream)
        pipe.sync()
        us.append(t.elapsed_ms() * 1e3)
    us = np.array(us[1:])
    nbytes = 8 * sum(n + 1 for n in clens)
    floor_us = nbytes / (copy_gbs * 1e9) * 1e6
    out = {"shape": name, "contigs": len(clens), "entries": [n + 1 for n in clens], "bytes": nbytes,
           "us_min": float(us.min()), "us_median": float(np.median(us)), "us_max": float(us.max()),
           "copy_rate_us": floor_us, "x_copy_min": float(us.min() / floor_us), "x_copy_median": float(np.median(us) / floor_us)}
    t.close()
    ctx.close()
    return out


def main():
    ctx = capi.Context(0)
    copy_gbs = bench.copy_peak_gbs(ctx)
    ctx.close()
    res = {"library": capi.library_path(), "peak_measured_copy_gbs": copy_gbs, "launches_timed": LAUNCHES - 1,
           "shapes": [run(name, clens, copy_gbs) for name, clens in SHAPES]}
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
