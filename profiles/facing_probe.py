#!/usr/bin/env python3
"""clip_facing_kernel (-I, im_span.hip) next to im_clip_reset of the same contig, cliptail_consensus_kernel next to cliptail_verify_kernel
on the same queries, and the product with -G -C -V -I next to -G -C -V.

Facing: one contig of --positions (64 M) positions.  Its two clip arrays get the clip events of the configs[1] chunk (synth seed 1, 1 Mb at
30x: right clips at refend, left clips at pos, clips of >= 20 bases), repeated every 1 Mb, through im_clip_build; im_clip_facing searches
them with m = 3, T = 30 and cap = 0, so that the call is the counter's memset, the kernel and four bytes back.  Beside it im_clip_reset of
the same contig in the genome-wide arrays: two memsets of the same (positions + 1) * 4 bytes each, the memory-speed pass over arrays of
this very shape.  Facing READS one array, the reset WRITES two.  Each is issued --warm times, then --reps times between two HIP events with
a stream synchronise in front of each; im_clip_facing waits for its counter inside the window, the reset does not wait at all, so the
facing figure carries one host wake-up the reset's does not.  Median, smallest and largest are printed, and GB/s from the median.

Consensus: the chunk's table and 300 flush-shaped queries as profiles/cliptail_probe.py makes them (300 piles of right clips, each with
the nearest pile of left clips behind it); im_cliptail_verify of the 300 pairs and im_cliptail_consensus of the same 600 piles, host clock
around the synchronous calls.

Product (--wall DIR): synth_1mb_30x is written into DIR when it is not there; `--bin A -G -C -V -I f`, `--bin A -G -C -V` and
`--parent-bin B -G -C -V` run alternately, one warm-up each and --runs timed runs each, wall clock around the whole process.

    python profiles/facing_probe.py [--reps 20] [--positions 67108864]
    python profiles/facing_probe.py --wall DIR --parent-bin PATH [--runs 5]
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


def chunk_events(rd, min_clip=20):
    """(positions of right clips, positions of left clips) of the simulator's reads under -C's record rule (every read has mapq 60)"""
    rows = np.arange(rd.n)
    last = np.maximum(rd.ncig.astype(np.int64) - 1, 0)
    ok = (rd.flag & (0x4 | 0x100 | 0x200 | 0x400)) == 0
    valid = np.arange(rd.cig_op.shape[1])[None, :] < rd.ncig[:, None]
    refend = rd.pos + (rd.cig_len * np.isin(rd.cig_op, (0, 2)) * valid).sum(1)
    right = ok & (rd.ncig > 1) & (rd.cig_op[rows, last] == 4) & (rd.cig_len[rows, last] >= min_clip)
    left = ok & (rd.ncig > 1) & (rd.cig_op[:, 0] == 4) & (rd.cig_len[:, 0] >= min_clip)
    return refend[right].astype(np.int64), rd.pos[left].astype(np.int64)


def kernels(a):
    sys.path.insert(0, ROOT)
    from indelminer_amd import capi, rawrec, synth
    L = capi.lib()
    refs, rd = synth.simulate(seed=1, ref_len=1_000_000, coverage=30, read_len=100)
    ev_r, ev_l = chunk_events(rd)
    n = a.positions
    out = {"positions": n, "warm": a.warm, "reps": a.reps, "clock": "HIP events around one call, stream synchronised in front of it", "us": {}}

    # ---- facing against the reset, one contig of n positions
    big = capi.Context(0)
    big.set_reference([b"A" * n])
    big.clip_enable(20, 10)
    reps_of_chunk = max(n // 1_000_000, 1)
    shift = (np.arange(reps_of_chunk, dtype=np.int64) * 1_000_000)[:, None]
    pos = np.concatenate([(ev_r[None, :] + shift).reshape(-1), (ev_l[None, :] + shift).reshape(-1)])
    side = np.concatenate([np.zeros(reps_of_chunk * len(ev_r), np.uint8), np.ones(reps_of_chunk * len(ev_l), np.uint8)])
    keep = pos <= n
    big.clip_build(n, pos[keep].astype(np.int32), side[keep])
    found = C.c_int32(0)
    calls = {"clip_facing_kernel (im_clip_facing, cap 0)": lambda: L.im_clip_facing(big.h, 3, 30, 0, None, None, None, None, C.byref(found)),
             "im_clip_reset (two memsets)": lambda: L.im_clip_reset(big.h, 0, big.stream)}
    tm = capi.Timer(big)
    for name, call in calls.items():
        ts = []
        for k in range(a.warm + a.reps):
            big._check(L.im_stream_sync(big.h, big.stream))
            tm.start(big.stream)
            big._check(call())
            tm.stop(big.stream)
            if k >= a.warm:
                ts.append(tm.elapsed_ms() * 1e3)
        out["us"][name] = spread(ts)
    bytes_one = 4 * (n + 1)
    out["facing"] = {"events": int(keep.sum()), "piles": int(found.value), "bytes_read": bytes_one, "bytes_reset": 2 * bytes_one,
                     "GBps_facing": round(bytes_one / out["us"]["clip_facing_kernel (im_clip_facing, cap 0)"]["median"] / 1e3, 1),
                     "GBps_reset": round(2 * bytes_one / out["us"]["im_clip_reset (two memsets)"]["median"] / 1e3, 1)}
    t = time.perf_counter()
    piles = big.clip_facing(3, 30)
    out["facing"]["whole_call_ms"] = round((time.perf_counter() - t) * 1e3, 3)
    assert len(piles[0]) == found.value
    big.close()

    # ---- consensus against verify, the chunk's own table
    raw, off = rawrec.records(rd, qual=False)
    ctx = capi.Context(0)
    ctx.set_reference([refs[0].tobytes()])
    ctx.clip_enable(20, 10)
    ctx.cliptail_enable(20, 10, 19)
    d_raw = capi.DevBuf(ctx, len(raw) + 64).upload(raw)
    d_off = capi.DevBuf(ctx, 4 * len(off)).upload(off)
    recs = capi.DevRecords(rd.n, d_raw.ptr, d_off.ptr, 0)
    ctx.clip_scatter(recs)
    ctx.cliptail_scatter(recs)
    ctx._check(L.im_stream_sync(ctx.h, ctx.stream))
    m = len(refs[0]) + 1
    p = np.arange(m, dtype=np.int32)
    right = ctx.clip_query_tid(0, np.zeros(m, np.uint8), p, p)[0]
    left = ctx.clip_query_tid(0, np.ones(m, np.uint8), p, p)[0]
    lp = np.nonzero(left >= 1)[0]
    pairs = []
    for x in np.nonzero(right >= 1)[0]:
        j = np.searchsorted(lp, x + 1)
        if j < len(lp):
            pairs.append((int(x), int(lp[j])))
    out["piles"] = len(pairs)
    pairs = ((pairs or [(1000, 1500)]) * (300 // max(len(pairs), 1) + 1))[:300]
    pr = np.array([x for x, _ in pairs], np.int32)
    pl = np.array([y for _, y in pairs], np.int32)
    qpos = np.stack([pr, pl], 1).reshape(-1)
    qside = np.tile(np.array([0, 1], np.uint8), 300)

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
    out["call_us"]["cliptail verify, 300 queries"], _ = timed(lambda: ctx.cliptail_verify(0, pr, pl, 32))
    out["call_us"]["cliptail consensus, 600 queries (both piles of the 300)"], r = timed(lambda: ctx.cliptail_consensus(0, qpos, qside, 2))
    out["call_us"]["cliptail consensus, 300 queries (the right piles)"], _ = timed(lambda: ctx.cliptail_consensus(0, pr, np.zeros(300, np.uint8), 2))
    out["consensus"] = {"entries": int(r[0].sum()), "agree": int(r[4].sum()), "bases": int(r[1].sum())}
    out["facing_of_the_chunk"] = len(ctx.clip_facing_tid(0, 3, 30)[0])
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
    f = os.path.join(d, "ins.vcf")
    runs = {"-G -C -V -I": [a.bin, "-i", "cfg.txt", "-G", "-C", "-V", "-I", f], "parent -G -C -V": [a.parent_bin, "-i", "cfg.txt", "-G", "-C", "-V"],
            "-G -C -V": [a.bin, "-i", "cfg.txt", "-G", "-C", "-V"]}
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
    records = sum(1 for ln in open(f) if ln.strip() and not ln.startswith("#"))
    print(json.dumps({"dataset": "synth_1mb_30x", "runs": a.runs, "clock": "wall clock around the process, ms, alternating, one warm-up each",
                      "ms": {k: spread(v) for k, v in ts.items()}, "stdout_bytes": sizes, "records_in_FILE": records}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warm", type=int, default=3)
    ap.add_argument("--positions", type=int, default=64 << 20)
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
