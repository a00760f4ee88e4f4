#!/usr/bin/env python3
"""splitlink_scatter_kernel's time per chunk (-S, im_links.hip) next to cliptail_scatter_kernel's and pairlink_scatter_kernel's in the
same process, im_splitlink_count for the planted queries, and the product with -S next to the product without it.

Scatter: the configs[1] chunk (synth seed 1, 1 Mb at 30x, 300 000 records as the product's walkers deliver them), in three variants:
  1  as it is: its clipped reads carry no SA tag, so the few lanes with a qualifying clip walk their aux area and find nothing;
  2  with one SA:Z field in front of every record's tags (rawrec's aux_prefix puts the same bytes into every record: only the clipped
     reads walk to it, and those whose clip it fits store a link);
  3  with the fields an aligner writes (NM MD AS XS, 50 bytes) in front of that SA:Z field, so the window has to slide.
The table is reset and the stream waited for in front of every timed launch; the time is the host clock around launch + wait.
Count: the links of the planted data sets (tests/support/splitlinks.py) through im_dev_splitlink_scatter, then the two queries of every
record of their FILEs in one synchronous call each.
3 warm-ups, then --reps calls; median, smallest and largest.

Product (--wall DIR): synth_1mb_30x is written into DIR when it is not there; `--bin A -G -C -V -U f -N g -T h -S`, the same without -S
and `--parent-bin B -G -C -V -U f -N g -T h` run alternately, one warm-up each and --runs timed runs each, wall clock around the process.

    python profiles/splitlink_probe.py [--reps 20]
    python profiles/splitlink_probe.py --wall DIR --parent-bin PATH [--runs 11]
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

SA = b"SAZctg0,500001,+,70S30M,60,0;\0"
ALIGNER = b"NMC\1" + b"MDZ" + b"7A" * 16 + b"\0" + b"ASC\x64" + b"XSC\x20"


def launch(a):
    sys.path.insert(0, ROOT)
    from indelminer_amd import capi, rawrec, synth
    from tests.support import splitlinks as sl
    L = capi.lib()
    refs, rd = synth.simulate(seed=1, ref_len=1_000_000, coverage=30, read_len=100)
    ctx = capi.Context(0)
    ctx.set_reference([refs[0].tobytes()])
    ctx.cliptail_enable(20, 10, 19)
    ctx.pairlink_enable(10, 15)
    ctx.splitlink_enable(20, 10, 19, ["ctg0"])
    sync = lambda: ctx._check(L.im_stream_sync(ctx.h, ctx.stream))

    def chunk(prefix):
        raw, off = rawrec.records(rd, qual=False, aux_prefix=prefix)
        d_raw = capi.DevBuf(ctx, len(raw) + 64).upload(raw)
        d_off = capi.DevBuf(ctx, 4 * len(off)).upload(off)
        return capi.DevRecords(rd.n, d_raw.ptr, d_off.ptr, 0), (d_raw, d_off)

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

    out = {"warm": a.warm, "reps": a.reps, "records": int(rd.n), "scatter_us": {"clock": "host clock around launch + wait"}, "links": {}}
    s = out["scatter_us"]
    keep = []
    for name, prefix in (("1: as the chunk is, no SA tag", b""), ("2: an SA tag in every record", SA), ("3: NM MD AS XS in front of it", ALIGNER + SA)):
        recs, bufs = chunk(prefix)
        keep += bufs
        s["im_dev_splitlink_scatter, " + name] = timed(ctx.splitlink_reset, lambda: ctx.splitlink_scatter(recs))
        out["links"][name] = ctx.splitlink_stats()
        if not prefix:
            s["im_dev_cliptail_scatter"] = timed(ctx.cliptail_reset, lambda: ctx.cliptail_scatter(recs))
            out["clip_tail_entries"] = ctx.cliptail_stats()[0]
            s["im_dev_pairlink_scatter"] = timed(ctx.pairlink_reset, lambda: ctx.pairlink_scatter(recs))
            plain = recs
    s["im_dev_splitlink_scatter, 1 again"] = timed(ctx.splitlink_reset, lambda: ctx.splitlink_scatter(plain))
    for b in keep:
        b.free()
    ctx.close()
    # the planted queries
    out["count_us"] = {"clock": "host clock around the synchronous call"}
    for kind in ("DUP", "INV", "BND"):
        from indelminer_amd import rawrec as rr
        from tests.support import intercontig as ic, pairlinks as pk
        mod, refs, rd2, names, _ = sl.planted(kind)
        d = tempfile.mkdtemp()
        mod.write_planted(d, refs, rd2)
        bam, fa = d + "/aln.bam", d + "/ref.fa"
        raw, off, contigs = rr.records_from_bam(bam)
        clens = [n for _, n in contigs]
        plain_file = pk.render_of_bam(kind, bam, fa, 10)[0] if kind != "BND" else ic.render_of_bam(bam, fa, 10)[0]
        found = sl.with_sr(plain_file, kind, names, clens, sl.links_of(sl.split_raw(raw, off), names, clens, 20, 10))[1]
        q = []
        for first, second, _, _ in found:
            for x, y in ((first, second), (second, first)):
                q.append((x[0], x[2], x[1] - sl.WINDOW, x[1] + sl.WINDOW, y[0], y[2], y[1] - sl.WINDOW, y[1] + sl.WINDOW))
        ctx = capi.Context(0)
        ctx.set_reference([r.tobytes() for r in refs])
        ctx.splitlink_enable(20, 10, 12, names)
        d_raw = capi.DevBuf(ctx, len(raw) + 64).upload(raw)
        d_off = capi.DevBuf(ctx, 4 * len(off)).upload(off)
        ctx.splitlink_scatter(capi.DevRecords(len(off) - 1, d_raw.ptr, d_off.ptr, 0))
        cols = [[w[k] for w in q] for k in range(8)]
        ts = []
        for i in range(a.warm + a.reps):
            t = time.perf_counter()
            got = ctx.splitlink_count(*cols)
            dt = time.perf_counter() - t
            if i >= a.warm:
                ts.append(dt * 1e6)
        out["count_us"]["im_splitlink_count, the %d planted queries of %s" % (len(q), kind)] = spread(ts)
        out["sr_" + kind] = [int(x) for x in got]
        assert out["sr_" + kind] == [n for _, _, n1, n2 in found for n in (n1, n2)]
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
    f, g, h = (os.path.join(d, x) for x in ("dup.vcf", "inv.vcf", "bnd.vcf"))
    base = ["-i", "cfg.txt", "-G", "-C", "-V", "-U", f, "-N", g, "-T", h]
    runs = {"-G -C -V -U -N -T -S": [a.bin] + base + ["-S"], "parent -G -C -V -U -N -T": [a.parent_bin] + base, "-G -C -V -U -N -T": [a.bin] + base}
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
    records = [sum(1 for ln in open(p) if ln.strip() and not ln.startswith("#")) for p in (f, g, h)]
    print(json.dumps({"dataset": "synth_1mb_30x", "runs": a.runs, "clock": "wall clock around the process, ms, alternating, one warm-up each",
                      "ms": {k: spread(v) for k, v in ts.items()}, "stdout_bytes": sizes, "records_in_the_FILEs": records}))


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
