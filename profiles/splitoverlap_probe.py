#!/usr/bin/env python3
"""The cost of -H (im_links.hip): the split-link scatter with the overlap array on next to the scatter without it, and
im_splitlink_overlap's time per call next to the two count queries of every junction in the same process.

Scatter: the configs[1] chunk (synth seed 1, 1 Mb at 30x, 300 000 records without qualities) as profiles/splitlink_probe.py has it, in
two variants: 1 as it is (no SA tag: no link), 2 with one SA:Z field in front of every record's tags (the clipped reads whose clip it
fits store a link).  Two contexts in one process, one with the array and one without, timed alternately; the table is reset and the
stream waited for in front of every timed launch; the time is the host clock around launch + wait.  --scatter-only measures the
context without the array alone: run it under INDELMINER_AMD_LIB=<a build of the parent commit> for the parent's kernel on the same
chunk.

Query: the soak of tests/test_gpu_splitjunction.py (20 000 links, 2^16 slots) with a random d per link and all its junctions in one
call, and one tuple held by 64, 1 000 and 8 000 links; im_splitlink_count with the two queries of every junction is the yardstick.
3 warm-ups, then --reps calls; median, smallest and largest.

    python profiles/splitoverlap_probe.py [--reps 20] [--scatter-only]
prints one JSON line.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from facing_probe import spread      # noqa: E402
from splitlink_probe import SA       # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warm", type=int, default=3)
    ap.add_argument("--scatter-only", action="store_true")
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
    import numpy as np
    from indelminer_amd import capi, rawrec, synth
    L = capi.lib()
    refs, rd = synth.simulate(seed=1, ref_len=1_000_000, coverage=30, read_len=100)
    out = {"warm": a.warm, "reps": a.reps, "records": int(rd.n), "lib": os.environ.get("INDELMINER_AMD_LIB", "this tree's"),
           "scatter_us": {"clock": "host clock around launch + wait, the two contexts alternating"}, "links": {}}

    def context(overlap):
        ctx = capi.Context(0)
        ctx.set_reference([refs[0].tobytes()])
        ctx.splitlink_enable(20, 10, 19, ["ctg0"])
        if overlap:
            ctx.splitlink_overlap_enable()
        return ctx

    forms = {"array off": context(False)}
    if not a.scatter_only:
        forms["array on"] = context(True)
    for name, prefix in (("1: as the chunk is, no SA tag", b""), ("2: an SA tag in every record", SA)):
        raw, off = rawrec.records(rd, qual=False, aux_prefix=prefix)
        recs, keep, ts = {}, [], {k: [] for k in forms}
        for k, ctx in forms.items():
            d_raw = capi.DevBuf(ctx, len(raw) + 64).upload(raw)
            d_off = capi.DevBuf(ctx, 4 * len(off)).upload(off)
            keep += [d_raw, d_off]
            recs[k] = capi.DevRecords(rd.n, d_raw.ptr, d_off.ptr, 0)
        for i in range(a.warm + a.reps):
            for k, ctx in forms.items():
                ctx.splitlink_reset()
                ctx._check(L.im_stream_sync(ctx.h, ctx.stream))
                t = time.perf_counter()
                ctx.splitlink_scatter(recs[k])
                ctx._check(L.im_stream_sync(ctx.h, ctx.stream))
                dt = time.perf_counter() - t
                if i >= a.warm:
                    ts[k].append(dt * 1e6)
        for k, ctx in forms.items():
            out["scatter_us"]["%s, %s" % (name, k)] = spread(ts[k])
            out["links"]["%s, %s" % (name, k)] = ctx.splitlink_stats()
        for b in keep:
            b.free()
    for ctx in forms.values():
        ctx.close()
    if a.scatter_only:
        print(json.dumps(out))
        return

    # the query
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

    def table(name, clens, links, log2_slots, rng):
        ctx = capi.Context(0)
        ctx.set_reference([b"ACGT" * (n // 4) for n in clens])
        ctx.splitlink_enable(20, 10, log2_slots, ["c%d" % t for t in range(len(clens))])
        ctx.splitlink_overlap_enable()
        d = rng.integers(-60, 61, len(links)).astype(np.int16)
        for k in range(0, len(links), 7_000):
            ctx.splitlink_add_overlap(*[[x[j] for x in links[k:k + 7_000]] for j in range(6)], d[k:k + 7_000])
        found = ctx.splitlink_junctions(sj.WINDOW, 1 if len(set(links)) == 1 else sj.MIN_LINKS, sj.MIN_SPAN)
        t1, p1, s1, t2, p2, s2 = found[:6]
        w = sj.WINDOW
        two = (np.concatenate([t1, t2]), np.concatenate([s1, s2]), np.concatenate([p1 - w, p2 - w]), np.concatenate([p1 + w, p2 + w]),
               np.concatenate([t2, t1]), np.concatenate([s2, s1]), np.concatenate([p2 - w, p1 - w]), np.concatenate([p2 + w, p1 + w]))
        us_o, (known, median, agree) = timed(lambda: ctx.splitlink_overlap(t1, p1, s1, t2, p2, s2, w))
        us_c, counts = timed(lambda: ctx.splitlink_count(*two))
        n = len(t1)
        assert (known.astype(np.int64) <= counts[:n].astype(np.int64) + counts[n:]).all()        # every link has a d here; one that both queries count is taken once
        if n == 1:
            ds = np.sort(d.astype(np.int64))
            assert (int(known[0]), int(median[0]), int(agree[0])) == (len(ds), int(ds[(len(ds) - 1) // 2]), int((ds == ds[(len(ds) - 1) // 2]).sum()))
        out["query_us"][name] = {"links": len(links), "junctions": n, "im_splitlink_overlap": us_o, "im_splitlink_count, 2 queries per junction": us_c}
        ctx.close()

    rng = np.random.default_rng(2025)
    clens = [150_000, 90_000, 40_000]
    table("the soak of tests/test_gpu_splitjunction.py, 2^16 slots", clens, soak_links(rng, clens), 16, rng)
    for n in (64, 1_000, 8_000):
        table("hot site: one tuple held by %d links, 2^16 slots" % n, clens, [(0, 30_000, 0, 1, 20_000, 1)] * n, 16, rng)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
