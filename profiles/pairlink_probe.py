#!/usr/bin/env python3
"""pairlink_scatter_kernel's time per chunk (-M, im_links.hip) next to cliptail_scatter_kernel's in the same process,
im_pairlink_count for the planted queries, and the product with -M next to the product without it.

Scatter: the configs[1] chunk (synth seed 1, 1 Mb at 30x, 300 000 records as the product's walkers deliver them).  Its pairs are all in
the normal orientation, so it holds NO link: every workgroup of the scatter ends at its early return, which is the usual chunk.  A second
chunk has one pair in a hundred turned everted in its flags (about 1 500 links).  Either table is reset and the stream waited for in
front of every timed launch; the time is the host clock around launch + wait.
Count: the links of the planted inversions and of the planted duplications (tests/support/pairlinks.py) through im_pairlink_add, then the
queries of their records -- 18 and 9 -- in one synchronous call each.
3 warm-ups, then --reps calls; median, smallest and largest.

Product (--wall DIR): synth_1mb_30x is written into DIR when it is not there; `--bin A -G -C -V -U f -N g -M`, `--bin A -G -C -V -U f -N g`
and `--parent-bin B -G -C -V -U f -N g` run alternately, one warm-up each and --runs timed runs each, wall clock around the whole process.

    python profiles/pairlink_probe.py [--reps 20]
    python profiles/pairlink_probe.py --wall DIR --parent-bin PATH [--runs 5]
prints one JSON line.
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from facing_probe import spread      # noqa: E402


def launch(a):
    sys.path.insert(0, ROOT)
    from indelminer_amd import capi, rawrec, synth
    from tests.support import pairlinks as pk
    L = capi.lib()
    refs, rd = synth.simulate(seed=1, ref_len=1_000_000, coverage=30, read_len=100)
    ctx = capi.Context(0)
    ctx.set_reference([refs[0].tobytes()])
    ctx.cliptail_enable(20, 10, 19)
    ctx.pairlink_enable(10, 15)
    sync = lambda: ctx._check(L.im_stream_sync(ctx.h, ctx.stream))

    def chunk():
        raw, off = rawrec.records(rd, qual=False)
        d_raw = capi.DevBuf(ctx, len(raw) + 64).upload(raw)
        d_off = capi.DevBuf(ctx, 4 * len(off)).upload(off)
        return capi.DevRecords(rd.n, d_raw.ptr, d_off.ptr, 0), (d_raw, d_off)

    def timed(reset, fn):
        ts = []
        for i in range(a.warm + a.reps):
            reset(); sync()
            t = time.perf_counter()
            r = fn()
            sync()
            dt = time.perf_counter() - t
            if i >= a.warm:
                ts.append(dt * 1e6)
        return spread(ts), r

    out = {"warm": a.warm, "reps": a.reps, "records": int(rd.n), "scatter_us": {"clock": "host clock around launch + wait"}}
    s = out["scatter_us"]
    plain, keep = chunk()
    s["im_dev_pairlink_scatter, no link in the chunk"], _ = timed(ctx.pairlink_reset, lambda: ctx.pairlink_scatter(plain))
    out["links_of_the_plain_chunk"] = ctx.pairlink_stats()[0]
    s["im_dev_cliptail_scatter"], _ = timed(ctx.cliptail_reset, lambda: ctx.cliptail_scatter(plain))
    out["clip_tail_entries"] = ctx.cliptail_stats()[0]
    # one pair in a hundred everted, in the flags alone
    left = np.nonzero(((rd.flag & (0x4 | 0x8)) == 0) & (rd.pos < rd.mpos) & ((rd.flag & 0x30) == 0x20))[0][::100]
    rd.flag[left] = (rd.flag[left] & ~0x20) | 0x10
    some, keep2 = chunk()
    s["im_dev_pairlink_scatter, one pair in a hundred a link"], _ = timed(ctx.pairlink_reset, lambda: ctx.pairlink_scatter(some))
    out["links_of_that_chunk"] = ctx.pairlink_stats()[0]
    s["im_dev_pairlink_scatter, no link in the chunk, again"], _ = timed(ctx.pairlink_reset, lambda: ctx.pairlink_scatter(plain))
    for b in keep + keep2:
        b.free()
    ctx.close()
    # the planted queries
    out["count_us"] = {"clock": "host clock around the synchronous call"}
    for svtype, reads in (("INV", pk.planted_inv_reads), ("DUP", pk.planted_dup_reads)):
        refs, rd2, planted = reads()
        ctx = capi.Context(0)
        ctx.set_reference([refs[0].tobytes()])
        ctx.pairlink_enable(10, 12)
        ctx.pairlink_add(0, [p for _, p, _ in planted], [m for _, _, m in planted], [k for k, _, _ in planted])
        from tests.support import crossedpiles as cp
        from tests.support import invertedpiles as ip
        q = [pk.window_of("DUP", None, pl, pl + n) for pl, n in cp.SITES] if svtype == "DUP" else [pk.window_of("INV", ct, x, x + n) for x, n in ip.SITES for ct in ("3to3", "5to5")]
        cols = [[w[k] for w in q] for k in range(5)]
        ts = []
        for i in range(a.warm + a.reps):
            t = time.perf_counter()
            got = ctx.pairlink_count(0, *cols, pk.MIN_SEP)
            dt = time.perf_counter() - t
            if i >= a.warm:
                ts.append(dt * 1e6)
        out["count_us"]["im_pairlink_count, the %d planted queries of %s" % (len(q), svtype)] = spread(ts)
        out["pe_" + svtype] = [int(x) for x in got]
        ctx.close()
    print(json.dumps(out))


def wall(a):
    d = os.path.abspath(a.wall)
    sys.path.insert(0, ROOT)
    if not os.path.exists(os.path.join(d, "aln.bam")):
        import importlib.util
        spec = importlib.util.spec_from_file_location("make_golden", os.path.join(ROOT, "tests", "golden", "make_golden.py"))
        mg = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mg)
        os.makedirs(d, exist_ok=True)
        mg.write_dataset(d, mg.SYNTH_E2E["synth_1mb_30x"])
    f, g = os.path.join(d, "dup.vcf"), os.path.join(d, "inv.vcf")
    base = ["-i", "cfg.txt", "-G", "-C", "-V", "-U", f, "-N", g]
    runs = {"-G -C -V -U -N -M": [a.bin] + base + ["-M"], "parent -G -C -V -U -N": [a.parent_bin] + base, "-G -C -V -U -N": [a.bin] + base}
    ts = {k: [] for k in runs}
    sizes = {}
    for k in range(a.runs + 1):
        for name, cmd in runs.items():
            t = time.perf_counter()
            r = subprocess.run(cmd + ["ref.fa", "sample=aln.bam"], cwd=d, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
            dt = time.perf_counter() - t
            if r.returncode != 0:
                sys.exit("%s failed: %s" % (name, r.stderr.decode()[-500:]))
            sizes[name] = len(r.stdout)
            if k > 0:
                ts[name].append(dt * 1e3)
    records = [sum(1 for ln in open(p) if ln.strip() and not ln.startswith("#")) for p in (f, g)]
    print(json.dumps({"dataset": "synth_1mb_30x", "runs": a.runs, "clock": "wall clock around the process, ms, alternating, one warm-up each",
                      "ms": {k: spread(v) for k, v in ts.items()}, "stdout_bytes": sizes, "records_in_the_FILEs": records}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warm", type=int, default=3)
    ap.add_argument("--wall", default=None)
    ap.add_argument("--bin", default=os.path.join(ROOT, "indelminer_amd", "indelminer"))
    ap.add_argument("--parent-bin", default=None)
    ap.add_argument("--runs", type=int, default=5)
    a = ap.parse_args()
    if a.wall:
        if not a.parent_bin:
            sys.exit("--wall needs --parent-bin")
        wall(a)
    else:
        launch(a)


if __name__ == "__main__":
    main()
