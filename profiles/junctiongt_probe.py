#!/usr/bin/env python3
"""im_span_query_ends' time per call (-K, im_span.hip) next to im_span_query_tid's round trip in the same process, and the product with
-K next to the product without it.

Call: 24 contigs of 1 000 000 bases, the genome-wide span array enabled and every contig scanned (no records: the answers are zeros, the
loads are the same); 18, 1 856 (the 928 junctions of the soak of tests/test_gpu_splitjunction.py) and 100 000 ends drawn over all
contigs, slack 0 as the driver asks, and the 1 856 with slack 32 and 255.  The yardstick beside them is im_span_query_tid with one query
of one position.  The time is the host clock around the synchronous call.  3 warm-ups, then --reps calls; median, smallest and largest.

Product (--wall DIR): the planted data set of -N with its SA tags (tests/support/splitlinks.py, 18 junctions) is written into DIR when it
is not there; `-G -J f` and `-G -J f -K` run alternately, one warm-up each and --runs timed runs each, wall clock around the process.

    python profiles/junctiongt_probe.py [--reps 20]
    python profiles/junctiongt_probe.py --wall DIR [--runs 11]
prints one JSON line.
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from facing_probe import spread      # noqa: E402


def launch(a):
    sys.path.insert(0, ROOT)
    import numpy as np
    from indelminer_amd import capi
    n_contigs, clen = 24, 1_000_000
    ctx = capi.Context(0)
    ctx.set_reference([b"ACGT" * (clen // 4)] * n_contigs)
    ctx.span_enable(10, 10)
    for t in range(n_contigs):
        ctx.span_scan(t)
    ctx._check(capi.lib().im_stream_sync(ctx.h, ctx.stream))

    def timed(fn):
        ts = []
        for i in range(a.warm + a.reps):
            t = time.perf_counter()
            got = fn()
            dt = time.perf_counter() - t
            if i >= a.warm:
                ts.append(dt * 1e6)
        assert not got.any()
        return spread(ts)

    rng = np.random.default_rng(7)
    out = {"warm": a.warm, "reps": a.reps, "clock": "host clock around the synchronous call, us", "contigs": n_contigs, "contig length": clen}
    out["im_span_query_tid, 1 query"] = timed(lambda: ctx.span_query_tid(5, [123_456], [123_456]))
    for n, slack in ((18, 0), (1_856, 0), (100_000, 0), (1_856, 32), (1_856, 255)):
        tid = rng.integers(0, n_contigs, n).astype(np.int32)
        pos = rng.integers(0, clen + 1, n).astype(np.int32)
        out["im_span_query_ends, %d ends, slack %d" % (n, slack)] = timed(lambda: ctx.span_query_ends(tid, pos, slack))
    ctx.close()
    print(json.dumps(out))


def wall(a):
    d = os.path.abspath(a.wall)
    sys.path.insert(0, ROOT)
    if not os.path.exists(os.path.join(d, "aln.bam")):
        from tests.support import splitlinks as sl
        mod, refs, rd, _, _ = sl.planted("INV")
        os.makedirs(d, exist_ok=True)
        mod.write_planted(d, refs, rd)
    f = os.path.join(d, "junc.vcf")
    base = ["-i", "cfg.txt", "-s", "100", "-G", "-J", f]
    runs = {"-G -J": [a.bin] + base, "-G -J -K": [a.bin] + base + ["-K"]}
    ts = {k: [] for k in runs}
    records = {}
    for k in range(a.runs + 1):
        for name, cmd in runs.items():
            t = time.perf_counter()
            r = subprocess.run(cmd + ["ref.fa", "sample=aln.bam"], cwd=d, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
            dt = time.perf_counter() - t
            if r.returncode != 0:
                sys.exit("%s failed: %s" % (name, r.stderr.decode()[-500:]))
            records[name] = sum(1 for ln in open(f) if ln.strip() and not ln.startswith("#"))
            if k > 0:
                ts[name].append(dt * 1e3)
    print(json.dumps({"dataset": "the planted data set of -N with SA tags", "runs": a.runs, "clock": "wall clock around the process, ms, alternating, one warm-up each",
                      "ms": {k: spread(v) for k, v in ts.items()}, "records_in_the_FILE": records}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warm", type=int, default=3)
    ap.add_argument("--wall", default=None)
    ap.add_argument("--bin", default=os.path.join(ROOT, "indelminer_amd", "indelminer"))
    ap.add_argument("--runs", type=int, default=11)
    a = ap.parse_args()
    if a.wall:
        wall(a)
    else:
        launch(a)


if __name__ == "__main__":
    main()
