#!/usr/bin/env python3
"""-A's counting entry (im_support_count) against the entry it is derived from (im_support_batch + the host's verdict loop) on
the 40 000-task shape of support_probe.py, and annotate mode as a whole program with and without -A.

Kernel level: the same tasks both ways.  The probe lays every target of support_probe.py into one contig as left half + d filler
bases + right half and names the deletion of the filler as the task's known variant, so the window the count kernel reads through
the splice is byte for byte the target the batch entry is handed.  Repeated, interleaved runs; the baseline's own spread is the
margin.

Whole program (--program): a tumour / normal pair from the simulator (BASELINE configs[4] in small); discovery on the tumour, then
annotate mode on the normal without and with -A, INDELMINER_TIMING's lines with them.

    python profiles/known_counts_probe.py [n_tasks] [--program]
"""
import os
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
from indelminer_amd import capi  # noqa: E402

REPEATS = 9


def kernel_level(n):
    rng = np.random.default_rng(9)
    targets, queries, pieces = [], [], []
    variants, tasks = [], []
    off = 64
    qoff = 0
    for it in range(n):
        d = int(rng.integers(1, 50))
        len1 = 100 + 2 * d
        t = rng.choice(list(b"ACGT"), size=len1).astype(np.uint8)
        p = int(rng.integers(0, 2 * d + 1))
        q = t[p:p + 100].copy()
        if rng.random() < 0.5:
            cut = int(rng.integers(20, 80))
            q = np.concatenate([q[:cut], q[cut + min(d, 15):], rng.choice(list(b"ACGT"), size=min(d, 15)).astype(np.uint8)])
        sub = rng.random(len(q)) < 0.01
        q[sub] = rng.choice(list(b"ACGT"), size=int(sub.sum())).astype(np.uint8)
        targets.append(t.tobytes()); queries.append(q.tobytes())
        h = len1 // 2
        filler = rng.choice(list(b"ACGT"), size=d).astype(np.uint8)
        pieces += [t[:h], filler, t[h:], np.full(16, ord("N"), np.uint8)]
        variants.append((0, off + h, off + h + d + 1, capi.CLS_DELETION, 0, 1))
        own = (int(rng.integers(0, 4)), int(rng.integers(0, 20)), len(q) - int(rng.integers(0, 8)))
        tasks.append((it, off, off + len1 + d, qoff, len(q)) + own + (int(rng.integers(0, 4)) << 1,))
        off += len1 + d + 16
        qoff += len(q)
    contig = np.concatenate([np.full(64, ord("N"), np.uint8)] + pieces).tobytes()
    variants = np.array(variants, dtype=capi.KNOWN_VARIANT_DTYPE)
    tasks = np.array(tasks, dtype=capi.COUNT_TASK_DTYPE)
    qbytes = b"".join(queries)
    ctx = capi.Context(0)
    ctx.set_reference([contig])

    def baseline():
        out = ctx.support_batch(targets, queries)
        ok = (out[:, 0] <= tasks["own_subs"]) & (out[:, 1] <= tasks["own_indels"]) & (out[:, 2] >= tasks["own_aligned"])
        c = np.zeros((n, 3), np.int32)
        c[:, 0] = ok
        c[:, 1] = ok & ((tasks["flags"] & capi.SC_MAPQ_OK) != 0)
        c[:, 2] = ok & ((tasks["flags"] & (capi.SC_MAPQ_OK | capi.SC_SPANS)) == (capi.SC_MAPQ_OK | capi.SC_SPANS))
        return c

    def counting():
        return ctx.support_count(variants, b"N", tasks, qbytes)

    assert np.array_equal(baseline(), counting()), "the two entries disagree"
    tb, tc = [], []
    for _ in range(REPEATS):
        t0 = time.perf_counter(); baseline(); tb.append(time.perf_counter() - t0)
        t0 = time.perf_counter(); counting(); tc.append(time.perf_counter() - t0)
    for name, ts in (("im_support_batch + host verdict", tb), ("im_support_count", tc)):
        print("%-34s %d tasks  median %.2f ms  min %.2f  max %.2f  (%d runs, host buffers, incl. copies and the Python wrapper)"
              % (name, n, statistics.median(ts) * 1e3, min(ts) * 1e3, max(ts) * 1e3, len(ts)))
    print("baseline spread (max - min) / median: %.1f %%;  count / baseline at the medians: %.2f"
          % (100 * (max(tb) - min(tb)) / statistics.median(tb), statistics.median(tc) / statistics.median(tb)))
    ctx.close()


def whole_program():
    from indelminer_amd import bamwrite, build, synth
    prod = build.build_host()
    kw = dict(seed=4, ref_len=300_000, coverage=30, n_contigs=2)
    with tempfile.TemporaryDirectory() as d:
        for name, extra in (("normal", {}), ("tumor", dict(read_seed=55, somatic_spacing=15_000))):
            refs, rd = synth.simulate(**kw, **extra)
            contigs = [("ctg%d" % i, len(r)) for i, r in enumerate(refs)]
            bamwrite.write_fasta(d + "/ref.fa", contigs, refs)
            bamwrite.write_bam(d + "/%s.bam" % name, contigs, rd)
        open(d + "/cfg.txt", "w").write("IL generic 300 700\n")
        t = subprocess.run([prod, "-i", "cfg.txt", "ref.fa", "t=tumor.bam"], cwd=d, stdout=subprocess.PIPE, stderr=subprocess.DEVNULL, check=True)
        open(d + "/tumor.vcf", "wb").write(t.stdout)
        env = dict(os.environ, INDELMINER_TIMING="1")
        for flags in ([], ["-A"]):
            ts, lines = [], []
            for _ in range(5):
                t0 = time.perf_counter()
                r = subprocess.run([prod, "-i", "cfg.txt", "-q", "0", "-a", "-e", "1"] + flags + ["ref.fa", "tumor.vcf", "normal=normal.bam"], cwd=d,
                                   stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env, check=True)
                ts.append(time.perf_counter() - t0)
                lines = [ln for ln in r.stderr.decode().split("\n") if "annotate mode" in ln]
            print("annotate mode %-3s median %.3f s  min %.3f  max %.3f  (5 runs)" % (" ".join(flags), statistics.median(ts), min(ts), max(ts)))
            for ln in lines:
                print("    " + ln)


if __name__ == "__main__":
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    kernel_level(int(args[0]) if args else 40000)
    if "--program" in sys.argv:
        whole_program()
