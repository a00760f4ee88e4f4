#!/usr/bin/env python3
"""cliptail_pairs_kernel<true>'s time per candidate (-N, im_cliptail.hip) next to cliptail_pairs_kernel<false>'s in the same process, and the product
with -G -C -V -N next to -G -C -V.

Launch: the arrays and the table of the configs[1] chunk (synth seed 1, 1 Mb at 30x, clips of >= 20 bases; im_dev_clip_scatter,
im_dev_cliptail_scatter).  im_clip_inverted_tid with the driver's constants is the whole call: two peaks passes over 1 M positions, two
waits, the lists down, sorted and up, the ONE launch over both lists, the pairs down.  To set the launch apart the same call is timed with
max_len = min_len = 50 (hardly a candidate: the peaks passes and the round trips alone), and the difference is divided by the candidates,
which are counted here from the two peak lists (pairs of ONE list min_len .. max_len apart).  im_clip_crossed_tid is timed the same way
beside it, with its own constants and candidates.  How many candidates pass the kernel's first cut -- some shift at which at least
min_verified entries of the first pile match -- is counted by the plain restatement (tests/support/invertedpiles.py) from the records.
3 warm-ups, then --reps calls; median, smallest and largest; host clock around the synchronous calls.

Product (--wall DIR): synth_1mb_30x is written into DIR when it is not there; `--bin A -G -C -V -N f`, `--bin A -G -C -V` and
`--parent-bin B -G -C -V` run alternately, one warm-up each and --runs timed runs each, wall clock around the whole process.

    python profiles/inverted_probe.py [--reps 20]
    python profiles/inverted_probe.py --wall DIR --parent-bin PATH [--runs 5]
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

DRIVER = (3, 30, 50, 1_000_000, 32, 2)      # INV_EV_*: min_reads, reach, min_len, max_len, shift, min_verified
CROSSED = (3, 30, 50, 100_000, 32, 2)       # DUP_EV_*


def launch(a):
    sys.path.insert(0, ROOT)
    from indelminer_amd import capi, rawrec, synth
    L = capi.lib()
    refs, rd = synth.simulate(seed=1, ref_len=1_000_000, coverage=30, read_len=100)
    raw, off = rawrec.records(rd, qual=False)
    ctx = capi.Context(0)
    ref = refs[0].tobytes()
    ctx.set_reference([ref])
    ctx.clip_enable(20, 10)
    ctx.cliptail_enable(20, 10, 19)
    d_raw = capi.DevBuf(ctx, len(raw) + 64).upload(raw)
    d_off = capi.DevBuf(ctx, 4 * len(off)).upload(off)
    recs = capi.DevRecords(rd.n, d_raw.ptr, d_off.ptr, 0)
    ctx.clip_scatter(recs)
    ctx.cliptail_scatter(recs)
    ctx._check(L.im_stream_sync(ctx.h, ctx.stream))
    m, T, dmin, dmax, S, mv = DRIVER
    lists = [ctx.clip_peaks_tid(0, side, m, T)[0].astype(np.int64) for side in (0, 1)]
    same = lambda lo, hi: int(sum((np.searchsorted(p, p + hi, "right") - np.searchsorted(p, p + lo, "left")).sum() for p in lists))
    crossed = lambda lo, hi: int((np.searchsorted(lists[1], lists[0] - lo, "right") - np.searchsorted(lists[1], lists[0] - hi, "left")).sum())

    def timed(fn):
        ts = []
        for i in range(a.warm + a.reps):
            t = time.perf_counter()
            r = fn()
            dt = time.perf_counter() - t
            if i >= a.warm:
                ts.append(dt * 1e6)
        return spread(ts), r

    out = {"warm": a.warm, "reps": a.reps, "call_us": {"clock": "host clock around the synchronous call"}}
    c = out["call_us"]
    c["im_clip_inverted_tid, the driver's constants"], res = timed(lambda: ctx.clip_inverted_tid(0, *DRIVER))
    c["im_clip_inverted_tid, max_len = min_len"], _ = timed(lambda: ctx.clip_inverted_tid(0, m, T, dmin, dmin, S, mv))
    c["im_clip_crossed_tid, the driver's constants"], res_u = timed(lambda: ctx.clip_crossed_tid(0, *CROSSED))
    c["im_clip_crossed_tid, max_len = min_len"], _ = timed(lambda: ctx.clip_crossed_tid(0, CROSSED[0], CROSSED[1], CROSSED[2], CROSSED[2], CROSSED[4], CROSSED[5]))
    # the same launch with the distances of the crossed call, for a figure over the same kind of candidate count
    c["im_clip_inverted_tid, max_len 100 000"], _ = timed(lambda: ctx.clip_inverted_tid(0, m, T, dmin, CROSSED[3], S, mv))
    n_cand, n_few, n_mid = same(dmin, dmax), same(dmin, dmin), same(dmin, CROSSED[3])
    u_cand, u_few = crossed(CROSSED[2], CROSSED[3]), crossed(CROSSED[2], CROSSED[2])
    med = lambda k: c[k]["median"]
    out["inverted"] = {"right_peaks": len(lists[0]), "left_peaks": len(lists[1]), "candidates": n_cand, "candidates_of_the_short_call": n_few,
                       "candidates_at_max_len_100000": n_mid, "pairs": len(res[0]),
                       "us_per_candidate": round((med("im_clip_inverted_tid, the driver's constants") - med("im_clip_inverted_tid, max_len = min_len")) / max(n_cand - n_few, 1), 4),
                       "us_per_candidate_at_max_len_100000": round((med("im_clip_inverted_tid, max_len 100 000") - med("im_clip_inverted_tid, max_len = min_len")) / max(n_mid - n_few, 1), 4)}
    out["crossed"] = {"candidates": u_cand, "candidates_of_the_short_call": u_few, "pairs": len(res_u[0]),
                      "us_per_candidate": round((med("im_clip_crossed_tid, the driver's constants") - med("im_clip_crossed_tid, max_len = min_len")) / max(u_cand - u_few, 1), 4)}
    d_raw.free(); d_off.free()
    ctx.close()
    if not a.no_first_cut:
        # the first cut, from the records: the restatement's table and its match rule
        from tests.support import cliptails as ct
        from tests.support import invertedpiles as ip
        from tests.support.crossedpiles import shift_counts
        table = ct.table_of(ct.parse_raw(raw, off), [len(ref)], 20, 10)
        code = ip.comp_codes(ref)
        passed = 0
        for side, p in enumerate(lists):
            for x in p:
                for y in p[np.searchsorted(p, x + dmin):np.searchsorted(p, x + dmax, "right")]:
                    (a1, d1), _ = ip.windows(side, int(x), int(y))
                    passed += bool((shift_counts(table.get((0, side, int(x)), []), code, a1, d1, S) >= mv).any())
        out["inverted"]["candidates_that_pass_the_first_cut"] = passed
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
    f = os.path.join(d, "inv.vcf")
    runs = {"-G -C -V -N": [a.bin, "-i", "cfg.txt", "-G", "-C", "-V", "-N", f], "parent -G -C -V": [a.parent_bin, "-i", "cfg.txt", "-G", "-C", "-V"],
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
    ap.add_argument("--no-first-cut", action="store_true", help="skip the host-side count of the candidates that pass the first cut")
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
