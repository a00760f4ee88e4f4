#!/usr/bin/env python3
"""im_splitlink_junctions' time per call (-J, im_links.hip) next to im_splitlink_count's round trip in the same process, and the
product with -J next to the product without it.

Call: the links of the planted data sets (tests/support/splitlinks.py) through im_dev_splitlink_scatter into the table of 2^12 slots the
driver gives their BAM files; the soak's table (tests/test_gpu_splitjunction.py: 20 000 links on 300 hot ends, 2^16 slots); and hot
sites -- ONE tuple held by n links, n = 64, 1 000, 8 000 in a table of 2^16 slots: n walks of a run of n.  The yardstick beside every
one of them is im_splitlink_count with one query and with the two queries of every junction found, on the same table.  The time is the
host clock around the synchronous call.  3 warm-ups, then --reps calls; median, smallest and largest.

Product (--wall DIR): synth_1mb_30x is written into DIR when it is not there; `--bin A -G -J f`, `--bin A -G` and `--parent-bin B -G`
run alternately, one warm-up each and --runs timed runs each, wall clock around the process.

    python profiles/splitjunction_probe.py [--reps 20]
    python profiles/splitjunction_probe.py --wall DIR --parent-bin PATH [--runs 11]
prints one JSON line.
"""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from facing_probe import spread      # noqa: E402

W, MIN_LINKS, MIN_SPAN = 32, 3, 50


def measure(a, ctx, out, name):
    """the junction call, one count query and the two count queries of every junction, on the table ctx holds"""
    def timed(fn):
        ts = []
        for i in range(a.warm + a.reps):
            t = time.perf_counter()
            got = fn()
            dt = time.perf_counter() - t
            if i >= a.warm:
                ts.append(dt * 1e6)
        return spread(ts), got

    us, found = timed(lambda: ctx.splitlink_junctions(W, MIN_LINKS, MIN_SPAN))
    n = len(found[0])
    q = [[], [], [], [], [], [], [], []]
    for k in range(n):
        t1, p1, s1, t2, p2, s2 = (int(found[c][k]) for c in range(6))
        for x in ((t1, s1, p1 - W, p1 + W, t2, s2, p2 - W, p2 + W), (t2, s2, p2 - W, p2 + W, t1, s1, p1 - W, p1 + W)):
            for c in range(8):
                q[c].append(x[c])
    one = [c[:1] for c in q]
    us_one, _ = timed(lambda: ctx.splitlink_count(*one))
    us_all, counts = timed(lambda: ctx.splitlink_count(*q))
    assert [int(v) for v in counts] == [int(found[c][k]) for k in range(n) for c in (7, 8)]
    out[name] = {"links": ctx.splitlink_stats()[0], "junctions": n, "largest E": int(max(found[6])) if n else 0,
                 "im_splitlink_junctions": us, "im_splitlink_count, 1 query": us_one, "im_splitlink_count, %d queries" % (2 * n): us_all}


def launch(a):
    sys.path.insert(0, ROOT)
    import numpy as np
    from indelminer_amd import capi, rawrec as rr
    from tests.support import splitlinks as sl
    from tests.test_gpu_splitjunction import soak_links
    out = {"warm": a.warm, "reps": a.reps, "clock": "host clock around the synchronous call, us", "window": W, "min_links": MIN_LINKS, "min_span": MIN_SPAN}
    for kind in ("DUP", "INV", "BND"):
        mod, refs, rd, names, _ = sl.planted(kind)
        d = tempfile.mkdtemp()
        mod.write_planted(d, refs, rd)
        raw, off, _ = rr.records_from_bam(d + "/aln.bam")
        ctx = capi.Context(0)
        ctx.set_reference([r.tobytes() for r in refs])
        ctx.splitlink_enable(20, 10, 12, names)
        d_raw = capi.DevBuf(ctx, len(raw) + 64).upload(raw)
        d_off = capi.DevBuf(ctx, 4 * len(off)).upload(off)
        ctx.splitlink_scatter(capi.DevRecords(len(off) - 1, d_raw.ptr, d_off.ptr, 0))
        measure(a, ctx, out, "planted " + kind + ", 2^12 slots")
        d_raw.free(); d_off.free()
        ctx.close()
    rng = np.random.default_rng(2025)
    clens = [150_000, 90_000, 40_000]
    contigs = [bytes(rng.choice(np.frombuffer(b"ACGT", np.uint8), n)) for n in clens]

    def table(links, log2_slots):
        ctx = capi.Context(0)
        ctx.set_reference(contigs)
        ctx.splitlink_enable(20, 10, log2_slots, ["s0", "s1", "s2"])
        for k in range(0, len(links), 7_000):
            part = links[k:k + 7_000]
            ctx.splitlink_add(*[[x[c] for x in part] for c in range(6)])
        return ctx

    ctx = table(soak_links(np.random.default_rng(2025), clens), 16)
    measure(a, ctx, out, "soak: 20 000 links on 300 hot ends, 2^16 slots")
    ctx.close()
    for n in (64, 1_000, 8_000):
        ctx = table([(0, 70_000, 0, 1, 30_000, 1)] * n, 16)
        measure(a, ctx, out, "hot site: one tuple held by %d links, 2^16 slots" % n)
        ctx.close()
    ctx = table([(0, 70_000, 0, 1, 30_000, 1)] * 3, 24)
    measure(a, ctx, out, "3 links in a table of 2^24 slots (the sweep)")
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
    f = os.path.join(d, "junc.vcf")
    base = ["-i", "cfg.txt", "-G"]
    runs = {"-G -J": [a.bin] + base + ["-J", f], "parent -G": [a.parent_bin] + base, "-G": [a.bin] + base}
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
                      "ms": {k: spread(v) for k, v in ts.items()}, "stdout_bytes": sizes, "records_in_the_FILE": records}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warm", type=int, default=3)
    ap.add_argument("--wall", default=None)
    ap.add_argument("--bin", default=os.path.join(ROOT, "indelminer_amd", "indelminer"))
    ap.add_argument("--parent-bin", default=None)
    ap.add_argument("--runs", type=int, default=11)
    a = ap.parse_args()
    if a.wall:
        if not a.parent_bin:
            sys.exit("--wall needs --parent-bin")
        wall(a)
    else:
        launch(a)


if __name__ == "__main__":
    main()
