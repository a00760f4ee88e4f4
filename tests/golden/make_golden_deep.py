#!/usr/bin/env python3
"""Goldens of the deep-locus inputs (tests/support/deeplocus.py, INPUTS), made by the REFERENCE compiled in place
(oracle/_ref/indelminer): per input the VCF whose DP= beside the stacked records shows samtools' pileup cap at work, or not.
Beside every DP= near the stack this prints the PLAIN count -- the M/=/X depth of every record the pileup does not skip, summed
over the record's window [POS - 1, BP_END) and divided like src/shared.c:205 -- so that a reader sees where the cap bound.
python tests/golden/make_golden_deep.py [name ...]"""
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from tests.support import deeplocus  # noqa: E402

REF_BIN = os.path.join(ROOT, "oracle", "_ref", "indelminer")


def plain_count(rd, tid, beg, end):
    """floor(mean M/=/X depth over [beg, end)) of the records with none of 0x4 | 0x100 | 0x200 | 0x400"""
    ok = (rd.tid == tid) & ((rd.flag & (0x4 | 0x100 | 0x200 | 0x400)) == 0)
    total = 0
    x = rd.pos[ok].astype(np.int64)
    for k in range(rd.cig_op.shape[1]):
        has = rd.ncig[ok] > k
        op = rd.cig_op[ok][:, k]; ln = np.where(has, rd.cig_len[ok][:, k], 0).astype(np.int64)
        m = has & (op == 0)
        total += int(np.clip(np.minimum(x + ln, end) - np.maximum(x, beg), 0, None)[m].sum())
        x = x + np.where(has & ((op == 0) | (op == 2) | (op == 3)), ln, 0)
    return total // (end - beg)


def main(names):
    todo = []
    for name in names:
        todo.append((name, deeplocus.INPUTS[name], None))
        if name in deeplocus.ROUTE_INPUTS:
            todo.append((name + "_five_indels", dict(deeplocus.INPUTS[name], five_indels=True), None))
            todo.append((name + "_region", deeplocus.INPUTS[name], deeplocus.region_flags))
    for name, kw, flags in todo:
        with tempfile.TemporaryDirectory() as td:
            refs, rd, where = deeplocus.make(**kw)
            n, where2 = deeplocus.write(td, **kw)
            assert where2 == where
            t0 = time.time()
            q = subprocess.run([REF_BIN, "-i", "cfg.txt"] + (flags(where) if flags else []) + ["ref.fa", "s=aln.bam"], cwd=td, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
            took = time.time() - t0
            assert q.returncode == 0, q.stderr.decode()[-2000:]
            open(os.path.join(ROOT, "tests", "golden", "vcf", name + ".vcf"), "wb").write(q.stdout)
            body = [l.split(b"\t") for l in q.stdout.splitlines() if not l.startswith(b"#")]
            near = [f for f in body if f[0] == b"ctg%d" % where["contig"] and abs(int(f[1]) - where["deletion_start"]) < 60]
            shown = []
            for f in near:
                info = dict(kv.split(b"=") for kv in f[7].split(b";") if b"=" in kv)
                shown.append("POS %d DP=%d plain %d" % (int(f[1]), int(info[b"DP"]), plain_count(rd, where["contig"], int(f[1]) - 1, int(info[b"BP_END"]))))
            print("%-27s %6d reads, %s, %d records, the reference took %.1f s; at the stack: %s" % (name, n, where, len(body), took, "; ".join(shown)), flush=True)


if __name__ == "__main__":
    main(sys.argv[1:] or list(deeplocus.INPUTS))
