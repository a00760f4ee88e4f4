#!/usr/bin/env python3
"""The cost of -E (im_links.hip): the pair links' scatter in the stretched form next to the plain form, and im_junction_pairs' time per
call next to one im_pairlink_count round trip on the same table in the same process.

Scatter: the configs[1] chunk (synth seed 1, 1 Mb at 30x, 300 000 records without qualities) as the other probes have it.  Two contexts
in one process, one stretched and one plain, timed alternately; the table is reset and the stream waited for in front of every timed
launch; the time is the host clock around launch + wait.

Query: the planted data sets of tests/support/junctionpairs.py (their pair and mate links added, their junctions asked in one call) and
a soak in the shape of tests/test_gpu_junction_pairs.py's (20 000 links on 300 hot ends, 2^16 slots); the yardstick is ONE
im_pairlink_count call of as many queries on the same pair-link table.  3 warm-ups, then --reps calls; median, smallest and largest.

    python profiles/junctionpairs_probe.py [--reps 20]
prints one JSON line.
"""
import argparse
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from facing_probe import spread      # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warm", type=int, default=3)
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
    import numpy as np
    from indelminer_amd import capi, rawrec, synth
    L = capi.lib()
    refs, rd = synth.simulate(seed=1, ref_len=1_000_000, coverage=30, read_len=100)
    out = {"warm": a.warm, "reps": a.reps, "records": int(rd.n),
           "scatter_us": {"clock": "host clock around launch + wait, the two contexts alternating"}, "links": {}}

    def context(stretched):
        ctx = capi.Context(0)
        ctx.set_reference([refs[0].tobytes()])
        ctx.pairlink_enable(10, 19)
        if stretched:
            ctx.pairlink_stretched_enable()
        return ctx

    forms = {"plain": context(False), "stretched": context(True)}
    raw, off = rawrec.records(rd, qual=False)
    recs, keep, ts = {}, [], {k: [] for k in forms}
    for k, ctx in forms.items():
        d_raw = capi.DevBuf(ctx, len(raw) + 64).upload(raw)
        d_off = capi.DevBuf(ctx, 4 * len(off)).upload(off)
        keep += [d_raw, d_off]
        recs[k] = capi.DevRecords(rd.n, d_raw.ptr, d_off.ptr, 0)
    for i in range(a.warm + a.reps):
        for k, ctx in forms.items():
            ctx.pairlink_reset()
            ctx._check(L.im_stream_sync(ctx.h, ctx.stream))
            t = time.perf_counter()
            ctx.pairlink_scatter(recs[k])
            ctx._check(L.im_stream_sync(ctx.h, ctx.stream))
            dt = time.perf_counter() - t
            if i >= a.warm:
                ts[k].append(dt * 1e6)
    for k, ctx in forms.items():
        out["scatter_us"][k] = spread(ts[k])
        out["links"][k] = ctx.pairlink_stats()
    for b in keep:
        b.free()
    for ctx in forms.values():
        ctx.close()

    # the query
    from tests.support import junctionpairs as jp
    from tests.support import splitjunctions as sj
    from tests.test_gpu_splitjunction import soak_links
    out["query_us"] = {"clock": "host clock around the synchronous call"}

    def timed(fn):
        ts = []
        for i in range(a.warm + a.reps):
            t = time.perf_counter()
            got = fn()
            dt = time.perf_counter() - t
            if i >= a.warm:
                ts.append(dt * 1e6)
        return spread(ts), got

    def table(name, clens, pairs, mates, junctions, log2_slots):
        ctx = capi.Context(0)
        ctx.set_reference([b"ACGT" * (n // 4 + 1) for n in clens])
        clens = [4 * (n // 4 + 1) for n in clens]
        ctx.pairlink_enable(10, log2_slots)
        ctx.pairlink_stretched_enable()
        ctx.matelink_enable(10, log2_slots)
        for tid in range(len(clens)):
            mine = [x for x in pairs if x[0] == tid]
            for k in range(0, len(mine), 7_000):
                ctx.pairlink_add(tid, [l[2] for l in mine[k:k + 7_000]], [l[3] for l in mine[k:k + 7_000]], [l[1] for l in mine[k:k + 7_000]])
            mine = [x for x in mates if x[0] == tid]
            for k in range(0, len(mine), 7_000):
                ctx.matelink_add(tid, *[[l[j] for l in mine[k:k + 7_000]] for j in (2, 3, 4, 1)])
        cols = [[j[k] for j in junctions] for k in range(6)]
        us_j, (pe1, pe2) = timed(lambda: ctx.junction_pairs(*cols, jp.REACH, jp.BACK, jp.MIN_SEP))
        want = jp.answers_fast(pairs, mates, clens, junctions)
        assert [(int(x), int(y)) for x, y in zip(pe1, pe2)] == want
        # one round trip of the count query: as many queries, all on contig 0, the windows of the junctions' first ends
        n = len(junctions)
        a0 = np.array([j[1] - jp.REACH for j in junctions], np.int32)
        us_c, _ = timed(lambda: ctx.pairlink_count(0, np.full(n, 3, np.uint8), a0, a0 + jp.REACH + jp.BACK, a0 + 300, a0 + 300 + jp.REACH + jp.BACK, jp.MIN_SEP))
        out["query_us"][name] = {"pair links": len(pairs), "mate links": len(mates), "junctions": n, "pairs counted": int(sum(w[0] + w[1] for w in want)),
                                 "im_junction_pairs": us_j, "im_pairlink_count, one call of as many queries": us_c,
                                 "ratio of the medians": round(us_j["median"] / us_c["median"], 2)}
        ctx.close()

    for kind in ("DUP", "INV", "BND", "DEL"):
        d = tempfile.mkdtemp()
        if kind == "DEL":
            jp.write_planted(d, *jp.planted_deletion())
        else:
            mod, prefs, prd = jp.planted(kind)
            mod.write_planted(d, prefs, prd)
        names, clens, pairs, mates = jp.links_of_bam(d + "/aln.bam", 10)
        kept = jp.render_of_bam(d + "/aln.bam", d + "/ref.fa")[2]
        table("planted set %s, 2^12 slots" % kind, clens, pairs, mates, [j[:6] for j in kept], 12)

    rng = np.random.default_rng(2026)
    clens = [150_000, 90_000, 40_000]
    split = soak_links(rng, clens)
    pairs, mates = [], []
    for ta, pa, sa, tb, pb, sb in split:
        x = pa + int(rng.integers(-40, 1_100)) * (1 if sa else -1)
        y = pb + int(rng.integers(-40, 1_100)) * (1 if sb else -1)
        if not (0 <= x <= clens[ta] and 0 <= y <= clens[tb]):
            continue
        if ta != tb:
            mates += [(ta, sa | sb << 1, x, tb, y), (tb, sb | sa << 1, y, ta, x)]
        else:
            pairs.append((ta, jp.KIND[(sa, sb)], x, y) if x <= y else (ta, jp.KIND[(sb, sa)], y, x))
    table("the soak, 2^16 slots", clens, pairs, mates, sorted({sj.can(l) for l in split})[::4], 16)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
