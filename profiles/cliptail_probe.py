#!/usr/bin/env python3
"""cliptail_scatter_kernel and cliptail_verify_kernel (-V, im_cliptail.hip) next to clip_scatter_kernel and the clip arg-max call,
and the product with -G -C -V next to -G -C.  The method is clip_probe.py's.

Kernels: the configs[1] chunk (synth seed 1, 1 Mb at 30x of 100-base reads, 300 000 records without base qualities, as the
product's walkers deliver them).  Each scatter is launched --warm times, then --reps times between two HIP events with a stream
synchronise in front of each launch; the clip-tail table is cleared in front of that synchronise, so every launch inserts into an
empty table; a second series leaves the table as it stands, as the product's chunks find it, and a third runs the kernel with a
min_clip no record reaches.  The median, the smallest and the largest are printed.  --tree PATH imports indelminer_amd from another checkout
(the parent commit, built), --only clip leaves the clip-tail entries alone there.

Calls: 300 flush-shaped queries (the chunk's positions with right clips, each against the next position with left clips
behind it, cut or repeated to 300; the chunk has no large deletions, its clips stand at insertions, so the entries of either
side are compared at every shift and none verifies) through im_cliptail_verify, and the 600 arg-max queries of the same 300 records through
im_clip_query_tid; host clock around the synchronous call.  Then one pile of --pile entries on one key: what im_cliptail_add takes
for it (insertion into a pile walks the pile: quadratic in its depth) next to as many entries on keys of their own, and a verify
call of 300 queries at that pile.

Product (--wall DIR): synth_1mb_30x is written into DIR when it is not there; `--bin A -G -C -V` and `--parent-bin B -G -C` run
alternately, one warm-up each and --runs timed runs each, wall clock around the whole process; medians and spread are printed,
with the table the driver sizes for that BAM and what the data set stores in it.

    python profiles/cliptail_probe.py [--reps 20] [--tree PATH --only clip]
    python profiles/cliptail_probe.py --wall DIR --parent-bin PATH [--runs 5]
prints one JSON line.
"""
import argparse
import ctypes as C
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


def log2_slots_for(bam_bytes):
    """the host driver's rule: the smallest 2^k >= max(65 536, BAM bytes / 64), at most 2^30"""
    k = 16
    while k < 30 and (1 << k) < bam_bytes // 64:
        k += 1
    return k


def kernels(a):
    sys.path.insert(0, a.tree or ROOT)
    from indelminer_amd import capi, rawrec, synth
    L = capi.lib()
    refs, rd = synth.simulate(seed=1, ref_len=1_000_000, coverage=30, read_len=100)
    raw, off = rawrec.records(rd, qual=False)
    tails = a.only != "clip"
    ctx = capi.Context(0)
    ctx.set_reference([refs[0].tobytes()])
    ctx.clip_enable(20, 10)
    k = 19
    if tails:
        ctx.cliptail_enable(20, 10, k)
    d_raw = capi.DevBuf(ctx, len(raw) + 64).upload(raw)
    d_off = capi.DevBuf(ctx, 4 * len(off)).upload(off)
    recs = capi.DevRecords(rd.n, d_raw.ptr, d_off.ptr, 0)
    recs_ref = C.byref(recs)
    tm = capi.Timer(ctx)
    calls = {"clip_scatter_kernel": lambda: L.im_dev_clip_scatter(ctx.h, recs_ref, ctx.stream)}
    if tails:
        calls["cliptail_scatter_kernel"] = lambda: L.im_dev_cliptail_scatter(ctx.h, recs_ref, ctx.stream)
        # as the product runs it: chunk after chunk into the table as it stands (2^19 slots hold all these launches without a drop)
        calls["cliptail_scatter_kernel, table not cleared"] = calls["cliptail_scatter_kernel"]
    out = {"tree": a.tree or ROOT, "records": int(rd.n), "bytes": int(len(raw)), "warm": a.warm, "reps": a.reps,
           "clock": "HIP events around one launch, stream synchronised in front of it", "us": {}}
    for name, call in calls.items():
        ts = []
        for i in range(a.warm + a.reps):
            if name == "cliptail_scatter_kernel":
                ctx.cliptail_reset()
            ctx._check(L.im_stream_sync(ctx.h, ctx.stream))
            tm.start(ctx.stream)
            ctx._check(call())
            tm.stop(ctx.stream)
            if i >= a.warm:
                ts.append(tm.elapsed_ms() * 1e3)
        out["us"][name] = spread(ts)
    if tails:
        # the same kernel where no record clips (min_clip beyond any read): what the decision and the workgroup's hand-over cost
        # without a single insert
        none = capi.Context(0)
        none.set_reference([refs[0].tobytes()])
        none.cliptail_enable(1_000_000, 10, k)
        e_raw = capi.DevBuf(none, len(raw) + 64).upload(raw)
        e_off = capi.DevBuf(none, 4 * len(off)).upload(off)
        e_recs = capi.DevRecords(rd.n, e_raw.ptr, e_off.ptr, 0)
        tn = capi.Timer(none)
        ts = []
        for i in range(a.warm + a.reps):
            none._check(L.im_stream_sync(none.h, none.stream))
            tn.start(none.stream)
            none._check(L.im_dev_cliptail_scatter(none.h, C.byref(e_recs), none.stream))
            tn.stop(none.stream)
            if i >= a.warm:
                ts.append(tn.elapsed_ms() * 1e3)
        out["us"]["cliptail_scatter_kernel, no record clips"] = spread(ts)
        e_raw.free(); e_off.free()
        none.close()
        ctx._check(L.im_stream_sync(ctx.h, ctx.stream))
        stored, dropped = ctx.cliptail_stats()
        stored //= 1 + a.warm + a.reps                              # the last cleared launch and the launches that were not
        out["table"] = {"log2_slots": k, "stored_per_launch": stored, "dropped": dropped, "load": round(stored / (1 << k), 5),
                        "clipped_fraction_of_records": round(stored / rd.n, 5)}
        # flush-shaped queries: piles of right clips against the nearest pile of left clips behind them
        n = len(refs[0]) + 1
        p = np.arange(n, dtype=np.int32)
        runs = a.warm + a.reps                                      # the clip arrays hold that many launches
        right = ctx.clip_query_tid(0, np.zeros(n, np.uint8), p, p)[0].astype(np.int64) // runs
        left = ctx.clip_query_tid(0, np.ones(n, np.uint8), p, p)[0].astype(np.int64) // runs
        lp = np.nonzero(left >= 1)[0]
        pairs = []
        for x in np.nonzero(right >= 1)[0]:
            j = np.searchsorted(lp, x + 1)
            if j < len(lp):
                pairs.append((int(x), int(lp[j])))
        out["piles"] = len(pairs)
        if not pairs:
            pairs = [(1000, 1500)]
        pairs = (pairs * (300 // len(pairs) + 1))[:300]
        pr = np.array([x for x, _ in pairs], np.int32)
        pl = np.array([y for _, y in pairs], np.int32)
        side = np.tile(np.array([0, 1], np.uint8), 300)
        beg = np.stack([pr - 10, pl - 10], 1).reshape(-1).astype(np.int32)
        end = np.stack([pr + 10, pl + 10], 1).reshape(-1).astype(np.int32)

        def timed(fn):
            ts = []
            for i in range(a.warm + a.reps):
                t = time.perf_counter()
                r = fn()
                dt = time.perf_counter() - t
                if i >= a.warm:
                    ts.append(dt * 1e6)
            return spread(ts), r

        out["call_us"] = {"clock": "host clock around the synchronous call (copies in, one launch, copies out, one wait)"}
        out["call_us"]["clip arg-max, 600 queries"], _ = timed(lambda: ctx.clip_query_tid(0, side, beg, end))
        out["call_us"]["cliptail verify, 300 queries"], r = timed(lambda: ctx.cliptail_verify(0, pr, pl, 32))
        out["verified"] = {"right": int(r[0].sum()), "left": int(r[1].sum()), "stored_right": int(r[3].sum()), "stored_left": int(r[4].sum())}
        # one deep pile
        m = a.pile
        rng = np.random.default_rng(5)
        planes = rng.integers(0, 2**32, (m, 2), dtype=np.uint64).astype(np.uint32)
        nb = np.full(m, 32, np.uint8)
        t = time.perf_counter()
        ctx.cliptail_add(0, np.arange(m, dtype=np.int32) + 500_000, np.zeros(m, np.uint8), nb, planes)
        spread_keys_ms = (time.perf_counter() - t) * 1e3
        t = time.perf_counter()
        ctx.cliptail_add(0, np.full(m, 777_777, np.int32), np.zeros(m, np.uint8), nb, planes)
        one_key_ms = (time.perf_counter() - t) * 1e3
        out["pile"] = {"entries": m, "add_ms_keys_of_their_own": round(spread_keys_ms, 3), "add_ms_one_key": round(one_key_ms, 3)}
        q = np.full(300, 777_777, np.int32)
        out["call_us"]["cliptail verify, 300 queries at the pile of %d" % m], r = timed(lambda: ctx.cliptail_verify(0, q, q + 400, 32))
        out["pile"]["stored_right_seen"] = int(r[3][0])
        out["call_us"]["cliptail verify, 300 queries, pile present"], _ = timed(lambda: ctx.cliptail_verify(0, pr, pl, 32))
    d_raw.free(); d_off.free()
    ctx.close()
    print(json.dumps(out))


def wall(a):
    d = a.wall
    sys.path.insert(0, ROOT)
    if not os.path.exists(os.path.join(d, "aln.bam")):
        import importlib.util
        spec = importlib.util.spec_from_file_location("make_golden", os.path.join(ROOT, "tests", "golden", "make_golden.py"))
        mg = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mg)
        os.makedirs(d, exist_ok=True)
        mg.write_dataset(d, mg.SYNTH_E2E["synth_1mb_30x"])
    runs = {"-G -C -V": [a.bin, "-i", "cfg.txt", "-G", "-C", "-V"], "parent -G -C": [a.parent_bin, "-i", "cfg.txt", "-G", "-C"],
            "-G -C": [a.bin, "-i", "cfg.txt", "-G", "-C"]}
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
    # the table the driver sizes for this BAM, and what the data set stores in it
    from indelminer_amd import capi, rawrec
    bam_bytes = os.path.getsize(os.path.join(d, "aln.bam"))
    k = log2_slots_for(bam_bytes)
    raw, off, contigs = rawrec.records_from_bam(os.path.join(d, "aln.bam"))
    from tests.support import cliptails
    fasta = cliptails.read_fasta(os.path.join(d, "ref.fa"))
    ctx = capi.Context(0)
    ctx.set_reference([fasta[name] for name, _ in contigs])
    ctx.cliptail_enable(20, 10, k)
    d_raw = capi.DevBuf(ctx, len(raw) + 64).upload(raw)
    d_off = capi.DevBuf(ctx, 4 * len(off)).upload(off)
    ctx.cliptail_scatter(capi.DevRecords(len(off) - 1, d_raw.ptr, d_off.ptr, 0))
    ctx._check(capi.lib().im_stream_sync(ctx.h, ctx.stream))
    stored, dropped = ctx.cliptail_stats()
    d_raw.free(); d_off.free()
    ctx.close()
    print(json.dumps({"dataset": "synth_1mb_30x", "runs": a.runs, "clock": "wall clock around the process, ms, alternating, one warm-up each",
                      "ms": {k_: spread(v) for k_, v in ts.items()}, "stdout_bytes": sizes,
                      "table": {"bam_bytes": bam_bytes, "log2_slots": k, "records": len(off) - 1, "stored": stored, "dropped": dropped,
                                "load": round(stored / (1 << k), 5)}}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warm", type=int, default=3)
    ap.add_argument("--pile", type=int, default=4096)
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
