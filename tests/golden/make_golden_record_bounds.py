#!/usr/bin/env python3
"""Writes tests/golden/vcf/record_bounds_65_segments.vcf: what the COMPILED REFERENCE (oracle/_ref/indelminer, oracle/Makefile)
prints for the input of tests/support/recordbounds.py product_dataset -- a 2 x 1020 library in which three realign candidates support one deletion,
one of them with a segment list of 65 words.  Neither the product nor the CPU shim can print these bytes themselves: both hold the result
record's bound of 64 words (the shim in its im_realign_batch, tests/shim/im_shim.c).
    python tests/golden/make_golden_record_bounds.py"""
import os, subprocess, sys, tempfile
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from tests.support import recordbounds

REF = os.path.join(ROOT, "oracle", "_ref", "indelminer")
with tempfile.TemporaryDirectory() as d:
    infos, b1 = recordbounds.product_dataset(d)
    r = subprocess.run([REF] + recordbounds.PRODUCT_FLAGS + ["ref.fa", "sample=aln.bam"], cwd=d, stdout=subprocess.PIPE, stderr=subprocess.PIPE, check=True)
open(os.path.join(ROOT, "tests", "golden", "vcf", "record_bounds_65_segments.vcf"), "wb").write(r.stdout)
print("%d bytes, %d SPLIT_READ lines; the three reads: %r segments, one deletion at %d" % (
    len(r.stdout), r.stdout.count(b"SPLIT_READ"), [i.n_ops for i in infos], b1))
print([l for l in r.stdout.decode().splitlines() if "\t%d\t" % b1 in l or "\t%d\t" % (b1 + 1) in l])
