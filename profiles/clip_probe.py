#!/usr/bin/env python3
"""clip_scatter_kernel (-C, im_span.hip) next to span_scatter_kernel on the same chunk, and the product with -G -C next to -G.

Kernels: the configs[1] chunk (synth seed 1, 1 Mb at 30x of 100-base reads, 300 000 records without base qualities, as the
product's walkers deliver them).  Each scatter is launched --warm times, then --reps times between two HIP events with a stream
synchronise in front of each launch; the median, the smallest and the largest of those are printed.  --tree PATH imports
indelminer_amd from another checkout (the parent commit, built), --only span leaves the clip entries alone there.

Product (--wall DIR): synth_1mb_30x is written into DIR when it is not there; `--bin A -G -C` and `--parent-bin B -G` run
alternately, one warm-up each and --runs timed runs each, wall clock around the whole process; medians and spread are printed.

    python profiles/clip_probe.py [--reps 20] [--tree PATH --only span]
    python profiles/clip_probe.py --wall DIR --parent-bin PATH [--runs 5]
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


def spread(ts):
    ts = sorted(ts)
    return {"median": round(ts[len(ts) // 2], 2), "min": round(ts[0], 2), "max": round(ts[-1], 2)}


def kernels(a):
    sys.path.insert(0, a.tree or ROOT)
    from indelminer_amd import capi, rawrec, synth
    L = capi.lib()
    refs, rd = synth.simulate(seed=1, ref_len=1_000_000, coverage=30, read_len=100)
    raw, off = rawrec.records(rd, qual=False)
    valid = np.arange(rd.cig_op.shape[1])[None, :] < rd.ncig[:, None]
    last = np.maximum(rd.ncig.astype(np.int64) - 1, 0)
    rows = np.arange(rd.n)
    clipped = (rd.ncig > 1) & (((rd.cig_op[:, 0] == 4) & (rd.cig_len[:, 0] >= 20)) | ((rd.cig_op[rows, last] == 4) & (rd.cig_len[rows, last] >= 20)))
    ctx = capi.Context(0)
    ctx.set_reference([refs[0].tobytes()])
    ctx.span_enable(10, 10)
    calls = {"span_scatter_kernel": lambda: L.im_dev_span_scatter(ctx.h, recs_ref, ctx.stream)}
    if a.only != "span":
        ctx.clip_enable(20, 10)
        calls["clip_scatter_kernel"] = lambda: L.im_dev_clip_scatter(ctx.h, recs_ref, ctx.stream)
    d_raw = capi.DevBuf(ctx, len(raw) + 64).upload(raw)
    d_off = capi.DevBuf(ctx, 4 * len(off)).upload(off)
    recs = capi.DevRecords(rd.n, d_raw.ptr, d_off.ptr, 0)
    import ctypes as C
    recs_ref = C.byref(recs)
    tm = capi.Timer(ctx)
    out = {"tree": a.tree or ROOT, "records": int(rd.n), "bytes": int(len(raw)), "clipped_records": int(clipped.sum()), "cigar_ops_valid": int(valid.sum()),
           "warm": a.warm, "reps": a.reps, "clock": "HIP events around one launch, stream synchronised in front of it", "us": {}}
    for name, call in calls.items():
        ts = []
        for k in range(a.warm + a.reps):
            ctx._check(L.im_stream_sync(ctx.h, ctx.stream))
            tm.start(ctx.stream)
            ctx._check(call())
            tm.stop(ctx.stream)
            if k >= a.warm:
                ts.append(tm.elapsed_ms() * 1e3)
        out["us"][name] = spread(ts)
    if a.only != "span":
        # what the launches left: warm + reps times the chunk's clipped reads
        p = np.arange(len(refs[0]) + 1, dtype=np.int32)
        n = a.warm + a.reps
        out["events_per_launch"] = [int(ctx.clip_query_tid(0, np.full(len(p), s, np.uint8), p, p)[0].astype(np.int64).sum()) // n for s in (0, 1)]
    d_raw.free(); d_off.free()
    ctx.close()
    print(json.dumps(out))


def wall(a):
    d = a.wall
    if not os.path.exists(os.path.join(d, "aln.bam")):
        import importlib.util
        sys.path.insert(0, ROOT)
        spec = importlib.util.spec_from_file_location("make_golden", os.path.join(ROOT, "tests", "golden", "make_golden.py"))
        mg = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mg)
        os.makedirs(d, exist_ok=True)
        mg.write_dataset(d, mg.SYNTH_E2E["synth_1mb_30x"])
    runs = {"-G -C": [a.bin, "-i", "cfg.txt", "-G", "-C"], "parent -G": [a.parent_bin, "-i", "cfg.txt", "-G"], "-G": [a.bin, "-i", "cfg.txt", "-G"]}
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
    print(json.dumps({"dataset": "synth_1mb_30x", "runs": a.runs, "clock": "wall clock around the process, ms, alternating, one warm-up each",
                      "ms": {k: spread(v) for k, v in ts.items()}, "stdout_bytes": sizes}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warm", type=int, default=3)
    ap.add_argument("--tree", default=None)
    ap.add_argument("--only", default=None)
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
        kernels(a)


if __name__ == "__main__":
    main()
