#!/usr/bin/env python3
"""matelink_scatter_kernel's time per chunk (-T, im_links.hip) next to pairlink_scatter_kernel's in the same process, and
im_matelink_partner and im_cliptail_junction for the planted queries.

Scatter: the configs[1] chunk (synth seed 1, 1 Mb at 30x, 300 000 records as the product's walkers deliver them).  It has one contig, so
it holds NO mate link: every workgroup of the scatter ends at its early return, which is the usual chunk.  A second chunk, over a
reference of two contigs, has one in a hundred of the pairs whose mate starts inside the second contig turned inter-contig in its
cores alone (mtid; about 1 500 links: both reads of a pair store one).  The table is reset and the stream waited for in front of
every timed launch; the time is the host clock around launch + wait.  im_dev_pairlink_scatter on the plain chunk, in the same
process, is the yardstick.
Queries: the planted data set of tests/support/intercontig.py -- its links through im_matelink_add and its clip tails through
im_cliptail_add; the partner queries of its planted piles (two per pile, one call per contig and side, as the driver asks them) and the
junction queries of its twelve sites in one synchronous call.
3 warm-ups, then --reps calls; median, smallest and largest.

    python profiles/matelink_probe.py [--reps 20]
prints one JSON line.
"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from facing_probe import spread      # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warm", type=int, default=3)
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
    from indelminer_amd import capi, rawrec, synth
    from tests.support import clipcounts as cc
    from tests.support import cliptails as ct
    from tests.support import intercontig as ic
    L = capi.lib()
    refs, rd = synth.simulate(seed=1, ref_len=1_000_000, coverage=30, read_len=100)
    ctx = capi.Context(0)
    ctx.set_reference([refs[0].tobytes(), refs[0][:500_000].tobytes()])
    ctx.pairlink_enable(10, 15)
    ctx.matelink_enable(10, 15)
    sync = lambda: ctx._check(L.im_stream_sync(ctx.h, ctx.stream))

    def chunk(raw, off):
        d_raw = capi.DevBuf(ctx, len(raw) + 64).upload(raw)
        d_off = capi.DevBuf(ctx, 4 * len(off)).upload(off)
        return capi.DevRecords(len(off) - 1, d_raw.ptr, d_off.ptr, 0), (d_raw, d_off)

    def timed(reset, fn):
        ts = []
        for i in range(a.warm + a.reps):
            reset(); sync()
            t = time.perf_counter()
            fn()
            sync()
            dt = time.perf_counter() - t
            if i >= a.warm:
                ts.append(dt * 1e6)
        return spread(ts)

    out = {"warm": a.warm, "reps": a.reps, "records": int(rd.n), "scatter_us": {"clock": "host clock around launch + wait"}}
    s = out["scatter_us"]
    raw, off = rawrec.records(rd, qual=False)
    plain, keep = chunk(raw, off)
    s["im_dev_matelink_scatter, no link in the chunk"] = timed(ctx.matelink_reset, lambda: ctx.matelink_scatter(plain))
    out["links_of_the_plain_chunk"] = ctx.matelink_stats()[0]
    s["im_dev_pairlink_scatter, the same chunk"] = timed(ctx.pairlink_reset, lambda: ctx.pairlink_scatter(plain))
    # one pair in a hundred of those whose mate starts inside contig 1 inter-contig, in the cores alone: mtid 1 in both reads
    raw2 = raw.copy()
    pairs = np.nonzero(((rd.flag & (0x4 | 0x8)) == 0) & (rd.pos < rd.mpos) & (rd.mpos < 500_000))[0][::100]
    turned = set(int(x) for x in rd.pair_id[pairs])
    for i in np.nonzero(np.isin(rd.pair_id, list(turned)) & ((rd.flag & (0x4 | 0x8)) == 0))[0]:
        raw2[int(off[i]) + 20:int(off[i]) + 24] = np.frombuffer(np.int32(1).tobytes(), np.uint8)
    some, keep2 = chunk(raw2, off)
    s["im_dev_matelink_scatter, one pair in a hundred inter-contig"] = timed(ctx.matelink_reset, lambda: ctx.matelink_scatter(some))
    out["links_of_that_chunk"] = ctx.matelink_stats()[0]
    s["im_dev_matelink_scatter, no link in the chunk, again"] = timed(ctx.matelink_reset, lambda: ctx.matelink_scatter(plain))
    for b in keep + keep2:
        b.free()
    ctx.close()

    # the planted queries
    refs, rd2 = ic.planted_reads()
    d = tempfile.mkdtemp()
    ic.write_planted(d, refs, rd2)
    _, clens, links = ic.links_of_bam(d + "/aln.bam", 10)
    table = ct.table_of_bam(d + "/aln.bam", cc.MIN_CLIP, 10)[1]
    ctx = capi.Context(0)
    ctx.set_reference([np.asarray(r, np.uint8).tobytes() for r in refs])
    ctx.matelink_enable(10, 12)
    ctx.cliptail_enable(20, 10, 14)
    for tid in range(len(clens)):
        mine = [x for x in links if x[0] == tid]
        ctx.matelink_add(tid, [x[2] for x in mine], [x[3] for x in mine], [x[4] for x in mine], [x[1] for x in mine])
        rows = [(p, side, b) for (t, side, p), bs in table.items() if t == tid for b in bs]
        ctx.cliptail_add(tid, [r[0] for r in rows], [r[1] for r in rows], [len(r[2]) for r in rows], [ct.planes_of(r[2]) for r in rows])
    sites = ic.SITES + [ic.ONE_PAIR, ic.RANDOM_TAILS, ic.OUTVOTED]
    ends = sorted({e for s_ in sites for e in (s_[:3], s_[3:6])})
    calls = {}
    for tid, p, side in ends:
        calls.setdefault((tid, side), []).append(p)
    out["query_us"] = {"clock": "host clock around the synchronous calls"}
    ts, n_partner = [], []
    for i in range(a.warm + a.reps):
        t = time.perf_counter()
        n_partner = []
        for (tid, side), ps in sorted(calls.items()):
            kind = [side | m << 1 for m in (0, 1) for _ in ps]
            win = [ic.read_window(p, side) for _ in (0, 1) for p in ps]
            n_partner += [int(x) for x in ctx.matelink_partner(tid, kind, [w[0] for w in win], [w[1] for w in win])[2]]
        dt = time.perf_counter() - t
        if i >= a.warm:
            ts.append(dt * 1e6)
    out["query_us"]["im_matelink_partner, %d queries of the planted piles in %d calls" % (2 * len(ends), len(calls))] = spread(ts)
    out["n_partner"] = n_partner
    cols = [[s_[k] for s_ in sites] for k in range(6)]
    ts = []
    for i in range(a.warm + a.reps):
        t = time.perf_counter()
        got = ctx.cliptail_junction(*cols)
        dt = time.perf_counter() - t
        if i >= a.warm:
            ts.append(dt * 1e6)
    out["query_us"]["im_cliptail_junction, the %d planted sites in one call" % len(sites)] = spread(ts)
    out["junction_v1_v2_shift"] = [[int(g[i]) for g in got[:3]] for i in range(len(sites))]
    ctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
