#!/usr/bin/env python3
"""im_dev_flush_groupby alone on the device: its three launches on the buffers one pass of bench.py's step leaves, at
configs[1] (12 k candidates, 4 flushes) and at the config-3 shard shape (76 k candidates, 19 flushes).  HIP events around
the call, the stream drained in front of it, 3 warm-ups, the median of 20 with the range.  The library is the tree's or the
one INDELMINER_AMD_LIB names.

    python profiles/flushwide_probe.py
"""
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

import bench  # noqa: E402
from indelminer_amd import capi, synth  # noqa: E402

SHAPES = {"configs[1]": dict(seed=1, ref_len=1_000_000, coverage=30, read_len=100),
          "shard_config3": dict(seed=2, ref_len=6_250_000, coverage=30, read_len=100, big_every=7)}


def probe(kw, warmup=3, reps=20):
    refs, rd = synth.simulate(**kw)
    ctx = capi.Context(0)
    try:
        ctx.set_reference([refs[0].tobytes()])
        ctx.set_insert_ranges(["generic"], [rd.range_max])
        ps = bench.PipeStep(ctx, rd, 1)
        ps.step(); ps.sync()                     # the buffers now hold a complete pass; the call below repeats its last stage
        cur = ps.sets[0]
        fn, args = next((f, a) for f, a in cur["calls"] if getattr(f, "__name__", "") == "im_dev_flush_groupby")
        counts0 = cur["pipe"].d_counts.download(np.int32, 2).tolist()
        tm = capi.Timer(ctx)
        us = []
        for k in range(warmup + reps):
            ps.sync()
            tm.start(cur["stream"])
            ctx._check(fn(*args))
            tm.stop(cur["stream"])
            ps.sync()
            if k >= warmup:
                us.append(tm.elapsed_ms() * 1e3)
        counts1 = cur["pipe"].d_counts.download(np.int32, 2).tolist()
        return {"candidates": int(cur["pipe"].d_counters.download(np.int32, 8)[0]), "flushes": len(ps.flushes),
                "clusters_nodes": counts1, "same_as_the_pass": counts0 == counts1,
                "us_median": statistics.median(us), "us_min": min(us), "us_max": max(us)}
    finally:
        ctx.close()


if __name__ == "__main__":
    print(json.dumps({"lib": os.environ.get("INDELMINER_AMD_LIB", "tree"), "shapes": {k: probe(v) for k, v in SHAPES.items()}}))
