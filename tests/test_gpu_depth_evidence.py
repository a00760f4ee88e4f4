"""-D: depth evidence for the deletions of 50 bases and more (FORMAT DM:DFC), through the product's command line.

The yardstick is the plain restatement in this file and in tests/support/depthmedian.py, from the definition in the VCF header and
DESIGN.md section 4.5d: depth[p] = the records samtools' pileup would count (flag & (0x4 | 0x100 | 0x200 | 0x400) == 0) whose M / = / X covers p, capped at 4095;
DM = the lower medians (element (n - 1) // 2 of the sorted depths) over the deleted bases [POS, END), the 1000 bases in front and the
1000 bases behind, each clipped to the contig; DFC = (2000 inside + (l + r) // 2) // (l + r), with one flank f
(1000 inside + f // 2) // f, "." where the flanks present sum to zero.
"""
import functools
import os
import struct
import subprocess

import numpy as np
import pytest

from tests.support import spanarrays
from tests.support.depthmedian import CAP, FLANK, MIN_LEN, evidence_of
from tests.support.spanarrays import _product

pytestmark = pytest.mark.gpu


# (position, bases, insertion, on the reads of both halves of the sample): a deletion within 1000 bases of the contig's start, a
# split-read deletion under 50 bases, an insertion, a split-read deletion over 50, and deletions of some kb on every read
# (homozygous) or on half of them (heterozygous), which only discordant pairs can show
EVENTS = [(700, 80, False, True), (6000, 30, False, True), (9000, 20, True, True), (12000, 80, False, True),
          (20000, 3000, False, True), (30000, 2500, False, False), (40000, 2000, False, True), (50000, 1500, False, False)]
HOM_AT, HET_AT = 20000, 30000


def _half(which, **kw):
    """one half of the sample from the project's generator, with the events above in place of its random ones"""
    from indelminer_amd import synth
    ev = [e for e in EVENTS if e[3] or which == "a"]
    return synth.simulate(events=([e[0] for e in ev], [e[1] for e in ev], [e[2] for e in ev]), **kw)


def parse_record(b, o, _end):
    tid, pos, l_qname, mapq, _bin, n_cig, flag = struct.unpack_from("<iiBBHHH", b, o)
    cw = struct.unpack_from("<%dI" % n_cig, b, o + 32 + l_qname)
    return tid, pos, flag, [(c & 15, c >> 4) for c in cw]


read_bam_records = functools.partial(spanarrays.read_bam_records, parse_record=parse_record)


def depth_of_bam(bam):
    refs, recs = read_bam_records(bam)
    diff = [np.zeros(l + 1, np.int64) for _, l in refs]
    for tid, pos, flag, cigar in recs:
        if tid < 0 or flag & (0x4 | 0x100 | 0x200 | 0x400):
            continue
        x = pos
        for op, ln in cigar:
            if op in (0, 7, 8):
                a, b = max(x, 0), min(x + ln, refs[tid][1])
                if a < b:
                    diff[tid][a] += 1; diff[tid][b] -= 1
            if op in (0, 2, 3, 7, 8):
                x += ln
    return [n for n, _ in refs], [np.minimum(np.cumsum(d)[:l], CAP) for d, (_, l) in zip(diff, refs)]


@pytest.fixture(scope="module")
def sample(tmp_path_factory):
    from indelminer_amd import bamwrite, synth
    tmp = tmp_path_factory.mktemp("depth_evidence")
    kw = dict(seed=6, ref_len=60_000, coverage=15, n_contigs=1)
    refs, a = _half("a", **kw)
    refs_b, b = _half("b", read_seed=77, **kw)
    assert all(np.array_equal(x, y) for x, y in zip(refs, refs_b))
    rd = synth.Reads()
    order = np.lexsort((np.concatenate([a.pos, b.pos]), np.concatenate([a.tid, b.tid])))
    for k in ("tid", "pos", "flag", "mpos", "isize", "seq", "cig_op", "cig_len", "ncig", "mate_first"):
        setattr(rd, k, np.concatenate([getattr(a, k), getattr(b, k)])[order])
    rd.pair_id = np.concatenate([a.pair_id, b.pair_id + int(a.pair_id.max()) + 1])[order]
    rd.n, rd.read_len, rd.range_max, rd.mapq = a.n + b.n, a.read_len, a.range_max, a.mapq
    contigs = [("ctg%d" % i, len(r)) for i, r in enumerate(refs)]
    bamwrite.write_fasta(str(tmp / "ref.fa"), contigs, refs)
    bamwrite.write_bam(str(tmp / "aln.bam"), contigs, rd)
    (tmp / "cfg.txt").write_text("IL generic 300 700\n")
    names, depth = depth_of_bam(str(tmp / "aln.bam"))
    assert 25 <= np.median(depth[0]) <= 35
    return str(tmp), names, depth


def _run(binary, flags, cwd, env=None):
    e = dict(os.environ)
    e.update(env or {})
    return subprocess.run([binary] + flags + ["ref.fa", "sample=aln.bam"], cwd=cwd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=e)


def _ok(r):
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    return r.stdout


def records_of(out):
    return [ln.split("\t") for ln in out.decode().split("\n") if ln and not ln.startswith("#")]


ADDED_HEADER = ("##FORMAT=<ID=DM,", "##FORMAT=<ID=DFC,", "##depthEvidence=")


def strip_evidence(out):
    """a -D VCF without what -D adds: its three header lines, the two keys and the two values of the records that carry them"""
    lines = []
    for ln in out.decode().split("\n"):
        if ln.startswith(ADDED_HEADER):
            continue
        if ln and not ln.startswith("#"):
            cols = ln.split("\t")
            if cols[8].endswith(":DM:DFC"):
                cols[8] = cols[8][:-len(":DM:DFC")]
                cols[9] = ":".join(cols[9].split(":")[:-2])
            ln = "\t".join(cols)
        lines.append(ln)
    return "\n".join(lines).encode()


def check_header(out, pairs):
    text = out.decode().split("\n")
    at = [i for i, ln in enumerate(text) if ln.startswith("##FORMAT=")]
    assert [text[i].split(",")[0] for i in at] == ["##FORMAT=<ID=" + k for k in ("GT", "AD", "GQ", "DM", "DFC")] and at == list(range(at[0], at[0] + 5))
    assert "Number=3" in text[at[3]] and "Number=1" in text[at[4]]
    rest = text[at[4] + 1:]
    if pairs:
        assert rest[0].startswith("##pairedReadAD=")
        rest = rest[1:]
    assert rest[0].startswith("##depthEvidence=") and rest[1].startswith("#CHROM")
    for word in ("median", "1000", "50", "4095", "8000"):
        assert word in rest[0], word


def check_records(out, names, depth):
    """every record against the restatement; returns {POS: (cols, DFC)} of the records that carry the fields"""
    seen = {}
    kinds = set()
    for cols in records_of(out):
        info = dict(kv.split("=") for kv in cols[7].split(";") if "=" in kv)
        tags = cols[7].split(";")
        pos, end = int(cols[1]), int(info["END"])
        if tags[0] == "DELETION" and end - pos >= MIN_LEN:
            assert cols[8] == "GT:AD:GQ:DM:DFC", cols
            dm, dfc = evidence_of(depth[names.index(cols[0])], pos, end)
            assert cols[9].split(":")[3:] == [dm, dfc], (cols, dm, dfc)
            seen[pos] = (cols, dfc)
            kinds.add(tags[1])
        else:
            assert cols[8] == "GT:AD:GQ" and len(cols[9].split(":")) == 3, cols
            kinds.add("short" if tags[0] == "DELETION" else "insertion")
    return seen, kinds


@pytest.mark.parametrize("pairs", [False, True])
def test_product_depth_evidence(sample, pairs):
    d, names, depth = sample
    prod = _product()
    base = ["-i", "cfg.txt", "-G"] + (["-P"] if pairs else [])
    without = _ok(_run(prod, base, d))
    out = _ok(_run(prod, base + ["-D"], d))
    check_header(out, pairs)
    assert strip_evidence(out) == without                           # byte for byte what it printed without -D
    assert not any(ln.startswith(ADDED_HEADER) for ln in without.decode().split("\n")) and b":DM" not in without
    seen, kinds = check_records(out, names, depth)
    assert {"SPLIT_READ", "PAIRED_READ", "short", "insertion"} <= kinds, kinds
    near = lambda p: [v for k, v in seen.items() if abs(k - p) <= 20]
    (edge_cols, _), = near(700)
    dm = edge_cols[9].split(":")[3].split(",")
    assert "." not in dm and int(edge_cols[1]) < FLANK              # a flank that the contig's start cuts short is still a flank
    (hom_cols, hom), = near(HOM_AT)
    (het_cols, het), = near(HET_AT)
    assert "PAIRED_READ" in het_cols[7] and int(hom) < int(het) < 1000, (hom, het)      # of the data, not of the arithmetic
    # the record-at-a-time path prints the same bytes (im_depth_median over im_depth_build's array)
    assert _ok(_run(prod, base + ["-D"], d, env={"INDELMINER_PIPELINE": "host"})) == out
    if not pairs:
        r = _run(prod, base + ["-D", "-c", "ctg0:1-30000"], d)
        assert r.returncode != 0 and r.stdout == b"" and b"indelminer: -D is not available with -c" in r.stderr
        d0 = _ok(_run(prod, ["-i", "cfg.txt", "-o", "detailed"], d))
        assert _ok(_run(prod, ["-i", "cfg.txt", "-o", "detailed", "-G", "-D"], d)) == d0 and len(d0) > 0
