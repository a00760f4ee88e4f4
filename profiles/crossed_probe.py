#!/usr/bin/env python3
"""clip_peaks_kernel (-U, im_span.hip) over both arrays of one contig next to clip_facing_kernel on the same contig, cliptail_pairs_kernel<false>'s
time per candidate next to cliptail_verify_kernel's time per query, and the product with -G -C -V -U next to -G -C -V.

Peaks: one contig of --positions (64 M) positions whose two clip arrays get the clip events of the configs[1] chunk (synth seed 1, 1 Mb at
30x, clips of >= 20 bases), repeated every 1 Mb, through im_clip_build -- the contig of profiles/facing_probe.py.  im_clip_peaks runs on
either side with m = 3, T = 30 and cap = 0, so that a call is the counter's memset, the kernel and four bytes back; im_clip_facing with
cap = 0 beside it.  The two peaks calls READ both arrays, facing reads one and the windows of the other at its peaks.  Each is issued
--warm times, then --reps times between two HIP events with a stream synchronise in front of each.  Median, smallest and largest are
printed, and GB/s from the median.

Cross: the chunk's own arrays and table (im_dev_clip_scatter, im_dev_cliptail_scatter).  im_clip_crossed_tid with the driver's constants is
the whole call: two peaks passes over 1 M positions, two waits, the lists down, sorted and up, the cross launch, the pairs down.  To set the
cross launch apart the same call is timed with max_len = min_len = 50 (hardly a candidate: the peaks passes and the round trips alone),
and the difference is divided by the candidates, which the plain restatement of the candidate rule counts from the two peak lists.
im_cliptail_verify of 300 flush-shaped queries (profiles/cliptail_probe.py) is timed beside it.  Host clock around the synchronous calls.

Product (--wall DIR): synth_1mb_30x is written into DIR when it is not there; `--bin A -G -C -V -U f`, `--bin A -G -C -V` and
`--parent-bin B -G -C -V` run alternately, one warm-up each and --runs timed runs each, wall clock around the whole process.

    python profiles/crossed_probe.py [--reps 20] [--positions 67108864]
    python profiles/crossed_probe.py --wall DIR --parent-bin PATH [--runs 5]
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
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from facing_probe import chunk_events, spread      # noqa: E402  (the contig and the figures of the facing probe)

DRIVER = (3, 30, 50, 100_000, 32, 2)        # DUP_EV_*: min_reads, reach, min_len, max_len, shift, min_verified


def kernels(a):
    sys.path.insert(0, ROOT)
    from indelminer_amd import capi, rawrec, synth
    L = capi.lib()
    refs, rd = synth.simulate(seed=1, ref_len=1_000_000, coverage=30, read_len=100)
    ev_r, ev_l = chunk_events(rd)
    n = a.positions
    out = {"positions": n, "warm": a.warm, "reps": a.reps, "clock": "HIP events around one call, stream synchronised in front of it", "us": {}}

    # ---- the peaks passes against the facing pass, one contig of n positions
    big = capi.Context(0)
    big.set_reference([b"A" * n])
    big.clip_enable(20, 10)
    reps_of_chunk = max(n // 1_000_000, 1)
    shift = (np.arange(reps_of_chunk, dtype=np.int64) * 1_000_000)[:, None]
    pos = np.concatenate([(ev_r[None, :] + shift).reshape(-1), (ev_l[None, :] + shift).reshape(-1)])
    side = np.concatenate([np.zeros(reps_of_chunk * len(ev_r), np.uint8), np.ones(reps_of_chunk * len(ev_l), np.uint8)])
    keep = pos <= n
    big.clip_build(n, pos[keep].astype(np.int32), side[keep])
    found = [C.c_int32(0) for _ in range(3)]
    calls = {"clip_peaks_kernel, right (im_clip_peaks, cap 0)": lambda: L.im_clip_peaks(big.h, 0, 3, 30, 0, None, None, C.byref(found[0])),
             "clip_peaks_kernel, left (im_clip_peaks, cap 0)": lambda: L.im_clip_peaks(big.h, 1, 3, 30, 0, None, None, C.byref(found[1])),
             "clip_facing_kernel (im_clip_facing, cap 0)": lambda: L.im_clip_facing(big.h, 3, 30, 0, None, None, None, None, C.byref(found[2]))}
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
    med = lambda name: out["us"][name]["median"]
    both = med("clip_peaks_kernel, right (im_clip_peaks, cap 0)") + med("clip_peaks_kernel, left (im_clip_peaks, cap 0)")
    out["peaks"] = {"events": int(keep.sum()), "right_peaks": int(found[0].value), "left_peaks": int(found[1].value), "facing_piles": int(found[2].value),
                    "bytes_read_peaks": 2 * bytes_one, "bytes_read_facing": bytes_one, "us_both_sides": round(both, 2),
                    "GBps_peaks": round(2 * bytes_one / both / 1e3, 1),
                    "GBps_facing": round(bytes_one / med("clip_facing_kernel (im_clip_facing, cap 0)") / 1e3, 1),
                    "peaks_over_facing": round(both / med("clip_facing_kernel (im_clip_facing, cap 0)"), 3)}
    big.close()

    # ---- the cross launch per candidate against verify per query, the chunk's own arrays and table
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
    m, T, dmin, dmax, S, mv = DRIVER
    pr_list = ctx.clip_peaks_tid(0, 0, m, T)[0].astype(np.int64)
    pl_list = ctx.clip_peaks_tid(0, 1, m, T)[0].astype(np.int64)
    cands = lambda lo, hi: int((np.searchsorted(pl_list, pr_list - lo, "right") - np.searchsorted(pl_list, pr_list - hi, "left")).sum())
    p = np.arange(len(refs[0]) + 1, dtype=np.int32)
    right = ctx.clip_query_tid(0, np.zeros(len(p), np.uint8), p, p)[0]
    left = ctx.clip_query_tid(0, np.ones(len(p), np.uint8), p, p)[0]
    lp = np.nonzero(left >= 1)[0]
    pairs = []
    for x in np.nonzero(right >= 1)[0]:
        j = np.searchsorted(lp, x + 1)
        if j < len(lp):
            pairs.append((int(x), int(lp[j])))
    pairs = ((pairs or [(1000, 1500)]) * (300 // max(len(pairs), 1) + 1))[:300]
    qr = np.array([x for x, _ in pairs], np.int32)
    ql = np.array([y for _, y in pairs], np.int32)

    def timed(fn):
        ts = []
        for i in range(a.warm + a.reps):
            t = time.perf_counter()
            r = fn()
            dt = time.perf_counter() - t
            if i >= a.warm:
                ts.append(dt * 1e6)
        return spread(ts), r

    out["call_us"] = {"clock": "host clock around the synchronous call"}
    out["call_us"]["cliptail verify, 300 queries"], _ = timed(lambda: ctx.cliptail_verify(0, qr, ql, 32))
    out["call_us"]["im_clip_crossed_tid, the driver's constants"], res = timed(lambda: ctx.clip_crossed_tid(0, *DRIVER))
    out["call_us"]["im_clip_crossed_tid, max_len = min_len"], _ = timed(lambda: ctx.clip_crossed_tid(0, m, T, dmin, dmin, S, mv))
    n_cand, n_few = cands(dmin, dmax), cands(dmin, dmin)
    full, few = out["call_us"]["im_clip_crossed_tid, the driver's constants"]["median"], out["call_us"]["im_clip_crossed_tid, max_len = min_len"]["median"]
    out["cross"] = {"right_peaks": len(pr_list), "left_peaks": len(pl_list), "candidates": n_cand, "candidates_of_the_short_call": n_few,
                    "pairs": len(res[0]), "us_per_candidate": round((full - few) / max(n_cand - n_few, 1), 4),
                    "verify_us_per_query": round(out["call_us"]["cliptail verify, 300 queries"]["median"] / 300, 4)}
    d_raw.free(); d_off.free()
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
    f = os.path.join(d, "dup.vcf")
    runs = {"-G -C -V -U": [a.bin, "-i", "cfg.txt", "-G", "-C", "-V", "-U", f], "parent -G -C -V": [a.parent_bin, "-i", "cfg.txt", "-G", "-C", "-V"],
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
