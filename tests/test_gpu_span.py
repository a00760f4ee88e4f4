"""Genotype columns (-G): the reference-spanning read counts of im_span.hip and what the host driver makes of them.

The yardstick is the plain restatement in this file (span_of / genotype_of), written from the definition in
include/indelminer_amd.h and DESIGN.md, not the code under test:

  * a record is eligible iff flag & (0x4 | 0x100 | 0x200 | 0x400) == 0, 0 <= tid < contigs, mapq >= min_mapq;
  * a run is a maximal sequence of consecutive M / = / X operations, covering [s, e) clipped to [0, clen); D and N advance and
    end a run, every other operation ends a run without advancing;
  * span[p], 0 <= p <= clen, counts the runs with s <= p - m and p + m <= e;
  * RS of a printed variant = min(span[p] for p in POS .. POS + (BP_END - END)); GT / GQ from (RS, NS) in integers.
"""
import functools
import importlib.util
import os
import struct
import subprocess

import numpy as np
import pytest

from tests.support import spanarrays
from tests.support.spanarrays import GOLD, ROOT, _golden, _product, check_device, genotype_of, interval_minima, interval_queries

pytestmark = pytest.mark.gpu

TD = os.path.join(GOLD, "test_data")

OPS = "MIDNSHP=X"


# ------------------------------------------------------------------------------------------ the restatement

def runs_of(pos, cigar):
    """cigar: [(op, len)] -> the maximal M/=/X runs [(s, e)], unclipped"""
    out, x, s = [], pos, None
    for op, ln in cigar:
        if op in (0, 7, 8):
            if s is None:
                s = x
            x += ln
            continue
        if s is not None:
            out.append((s, x))
            s = None
        if op in (2, 3):
            x += ln
    if s is not None:
        out.append((s, x))
    return out


def eligible(tid, flag, mapq, n_contigs, min_mapq):
    return (flag & (0x4 | 0x100 | 0x200 | 0x400)) == 0 and 0 <= tid < n_contigs and mapq >= min_mapq


def span_of_runs(runs, clen, m):
    """runs: [(s, e)] of one contig -> span[0 .. clen] by counting, position by position, through a difference array"""
    d = np.zeros(clen + 2, np.int64)
    for s, e in runs:
        s, e = max(s, 0), min(e, clen)
        if e - s >= 2 * m:
            d[s + m] += 1          # first p with s <= p - m
            d[e - m + 1] -= 1      # one past the last p with p + m <= e
    return np.cumsum(d)[:clen + 1]


def span_of(records, clens, m, min_mapq):
    """records: [(tid, pos, mapq, flag, [(op, len)])] -> one span array per contig"""
    per = [[] for _ in clens]
    for tid, pos, mapq, flag, cigar in records:
        if eligible(tid, flag, mapq, len(clens), min_mapq):
            per[tid] += runs_of(pos, cigar)
    return [span_of_runs(per[t], clens[t], m) for t in range(len(clens))]


def span_brute(records, clen, tid_want, m, min_mapq, n_contigs):
    """the definition itself, no difference array (small inputs): checks the restatement above"""
    out = np.zeros(clen + 1, np.int64)
    for tid, pos, mapq, flag, cigar in records:
        if tid != tid_want or not eligible(tid, flag, mapq, n_contigs, min_mapq):
            continue
        for s, e in runs_of(pos, cigar):
            s, e = max(s, 0), min(e, clen)
            for p in range(clen + 1):
                if s <= p - m and p + m <= e:
                    out[p] += 1
    return out


# ------------------------------------------------------------------------------------------ records

def cig(text):
    """'50M2D50M' -> [(op, len)]"""
    out, num = [], ""
    for ch in text:
        if ch.isdigit():
            num += ch
        else:
            out.append((OPS.index(ch), int(num)))
            num = ""
    return out


def raw_records(records):
    """[(tid, pos, mapq, flag, cigar)] -> the device layout (raw uint8, rec_off uint32[n + 1]): core, qname, CIGAR, packed bases,
    qualities, no aux; every record at a 4-byte aligned offset"""
    blob, off = bytearray(), [0]
    for i, (tid, pos, mapq, flag, cigar) in enumerate(records):
        qname = b"h%d\0" % i
        l_seq = sum(ln for op, ln in cigar if op in (0, 1, 4, 7, 8))
        core = struct.pack("<iiBBHHHiiii", tid, pos, len(qname), mapq, 4680, len(cigar), flag, l_seq, tid, pos, 0)
        body = core + qname + b"".join(struct.pack("<I", (ln << 4) | op) for op, ln in cigar) + b"\x11" * ((l_seq + 1) // 2) + b"\x28" * l_seq
        blob += body + b"\0" * (-len(body) % 4)
        off.append(len(blob))
    return np.frombuffer(bytes(blob), np.uint8).copy(), np.array(off, np.uint32)


def parse_record(b, o, _end=None):
    """one record at b[o:] -> (tid, pos, mapq, flag, cigar), bases left alone"""
    tid, pos, l_qname, mapq, _bin, n_cig, flag = struct.unpack_from("<iiBBHHH", b, o)
    cw = struct.unpack_from("<%dI" % n_cig, b, o + 32 + l_qname)
    return tid, pos, mapq, flag, [(c & 15, c >> 4) for c in cw]


def parse_raw(raw, off):
    """the device layout back into [(tid, pos, mapq, flag, cigar)]"""
    b = raw.tobytes()
    return [parse_record(b, int(off[i])) for i in range(len(off) - 1)]


read_bam_records = functools.partial(spanarrays.read_bam_records, parse_record=parse_record)


# ------------------------------------------------------------------------------------------ device level


Device = functools.partial(spanarrays.Device, "span")

CLENS = [150_000, 5_000]


def hand_made(m, min_mapq=10):
    c0, c1 = CLENS
    F = 0x63                                   # a proper pair, first in pair, mate reverse
    R = [
        (0, 1000, 60, F, cig("10=1X10=2X20=1X56=")),              # = / X alternating: one run of 100
        (0, 1010, 60, F, cig("50M2D50M")),                        # two runs of 50: both count at m = 10 and 25, neither at 26
        (0, 1020, 60, F, cig("30S70M")),
        (0, 1030, 60, F, cig("%dM" % (2 * m))),                   # a run of exactly 2 m: one position
        (0, 1040, 60, F, cig("%dM" % (2 * m - 1))),               # one base short: none
        (0, 0, 60, F, cig("100M")),                               # starts at position 0
        (0, c0 - 100, 60, F, cig("100M")),                        # ends on clen
        (0, c0 - 40, 60, F, cig("100M")),                         # reaches beyond clen: clipped
        (0, 1050, 60, F, cig("12M1I11M2D9M1I13M3D10M1I12M2N30M5S")),   # more CIGAR operations than the kernel keeps in registers
        (0, 1055, 60, F, cig("5H20M3P20M1I30M4H")),               # H and P end a run without advancing
        (0, 1060, 60, F | 0x4, cig("100M")),                      # unmapped
        (0, 1061, 60, F | 0x100, cig("100M")),                    # secondary
        (0, 1062, 60, F | 0x400, cig("100M")),                    # duplicate
        (0, 1063, 60, F | 0x200, cig("100M")),                    # QC fail
        (0, 1064, 60, F | 0x800, cig("100M")),                    # supplementary: not in the mask, counts
        (0, 1070, min_mapq - 1, F, cig("100M")),
        (0, 1071, min_mapq, F, cig("100M")),
        (-1, 1072, 60, F, cig("100M")),                           # no contig
        (7, 1073, 60, F, cig("100M")),                            # a contig that does not exist
        (1, 200, 60, F, cig("100M")),                             # a second contig in the same workgroup
        (1, 260, 60, F, cig("40M1D60M")),
        (1, c1 - 30, 60, F, cig("30M")),
        (0, 120_000, 60, F, cig("100M")),                         # far outside the LDS window
        (0, 120_030, 60, F, cig("60M10D40M")),
        (0, 1080, 60, F, cig("100M")),                            # and back again (unsorted input is legal for the scatter)
    ]
    return R


@pytest.mark.parametrize("m", [10, 25, 26])
def test_span_hand_made_records_every_position(m):
    recs = hand_made(m)
    want = span_of(recs, CLENS, m, 10)
    # the restatement against the definition, where that is affordable
    assert np.array_equal(want[1], span_brute(recs, CLENS[1], 1, m, 10, len(CLENS)))
    a = want[0]
    if m == 26:
        assert a[1010 + 26] == a[1010 + 25] and span_of([recs[1]], CLENS, m, 10)[0].max() == 0       # 50M2D50M: neither run
    else:
        assert span_of([recs[1]], CLENS, m, 10)[0].max() == 1
    assert span_of([recs[3]], CLENS, m, 10)[0].sum() == 1 and span_of([recs[4]], CLENS, m, 10)[0].sum() == 0
    dev = Device(CLENS, m, 10)
    try:
        raw, off = raw_records(recs)
        dev.scatter(raw, off)
        dev.scan()
        check_device(dev, want, np.random.default_rng(m))
    finally:
        dev.close()


def test_span_synthetic_chunk_every_position():
    """a chunk at the density of the 30x benchmark input (two contigs, so that workgroups straddle the contig boundary), scattered
    in two calls, with the hand-made records on top"""
    from indelminer_amd import rawrec, synth
    refs, rd = synth.simulate(seed=11, ref_len=150_000, coverage=30, n_contigs=2, big_every=9)
    clens = [len(r) for r in refs]
    raw, off = rawrec.records(rd)
    half = rd.n // 2
    m, q = 10, 10
    dev = Device(clens, m, q)
    try:
        for lo, hi in ((0, half), (half, rd.n)):
            r, o = rawrec.records(rd, lo, hi)
            dev.scatter(r, o)
        extra = [x for x in hand_made(m) if x[0] != 1 or x[1] < 1000]
        hr, ho = raw_records(extra)
        dev.scatter(hr, ho)
        dev.scan()
        recs = parse_raw(raw, off) + extra
        assert len(recs) == rd.n + len(extra)
        want = span_of(recs, clens, m, q)
        assert want[0].max() >= 15 and want[1].max() >= 15          # 30x of 100-base reads: about 24 span a boundary with 10 on each side
        check_device(dev, want, np.random.default_rng(5))
    finally:
        dev.close()


def test_span_records_without_qualities_and_reset():
    """the layout the product's walkers deliver (no base qualities); im_span_reset + a second pass gives the same array"""
    from indelminer_amd import rawrec, synth
    refs, rd = synth.simulate(seed=12, ref_len=60_000, coverage=20)
    clens = [len(r) for r in refs]
    raw, off = rawrec.records(rd, qual=False)
    full_raw, full_off = rawrec.records(rd)
    want = span_of(parse_raw(full_raw, full_off), clens, 12, 10)
    dev = Device(clens, 12, 10)
    try:
        dev.scatter(raw, off)
        dev.scan()
        assert np.array_equal(dev.every_position(0), want[0])
        dev.ctx.span_reset(0)
        dev.scatter(raw, off)
        dev.scan()
        assert np.array_equal(dev.every_position(0), want[0])
    finally:
        dev.close()


def test_span_host_segments_form():
    """im_span_build / im_span_query on host-given runs, against the same restatement on the same runs"""
    from indelminer_amd import capi
    rng = np.random.default_rng(21)
    clen = 90_000
    recs = [(0, int(p), 60, 0x63, cig(c)) for p, c in zip(rng.integers(-30, clen - 20, 30_000),
                                                         rng.choice(["100M", "50M2D50M", "30S70M", "20M", "19M", "21M", "40M1I59M", "250M"], 30_000))]
    runs = [r for rec in recs for r in runs_of(rec[1], rec[4])]
    start = np.array([s for s, e in runs], np.int32); length = np.array([e - s for s, e in runs], np.int32)
    ctx = capi.Context(0)
    try:
        for m in (1, 10, 25):
            want = span_of_runs(runs, clen, m)
            ctx.span_build(clen, start, length, m)
            p = np.arange(clen + 1, dtype=np.int32)
            assert np.array_equal(ctx.span_query(p, p).astype(np.int64), want), m
            beg, end = interval_queries(rng, clen)
            assert np.array_equal(ctx.span_query(beg, end).astype(np.int64), interval_minima(want, beg, end, clen)), m
        # a shorter contig in the same context, no runs at all
        ctx.span_build(100, np.zeros(0, np.int32), np.zeros(0, np.int32), 3)
        assert not ctx.span_query(np.arange(101, dtype=np.int32), np.arange(101, dtype=np.int32)).any()
    finally:
        ctx.close()


def span_of_run_arrays(start, length, clen, m):
    """span_of_runs on arrays (the large contigs below); the test checks it against span_of_runs itself first"""
    a = np.clip(start.astype(np.int64), 0, clen); b = np.clip(start.astype(np.int64) + length, 0, clen)
    ok = b - a >= 2 * m
    d = np.zeros(clen + 2, np.int64)
    np.add.at(d, a[ok] + m, 1); np.add.at(d, b[ok] - m + 1, -1)
    return np.cumsum(d)[:clen + 1]


def _span_case(ctx, rng, clen, nrun, m):
    """one im_span_build on ctx: every position, intervals clipped at both ends, intervals that are empty after the clip"""
    start = rng.integers(-50, clen + 20, nrun).astype(np.int32)
    length = rng.choice([19, 20, 21, 50, 70, 100, 250], nrun).astype(np.int32)
    want = span_of_run_arrays(start, length, clen, m)
    ctx.span_build(clen, start, length, m)
    p = np.arange(clen + 1, dtype=np.int32)
    assert np.array_equal(ctx.span_query(p, p).astype(np.int64), want), (clen, m)
    beg, end = interval_queries(rng, clen)
    beg = np.concatenate([beg, [-1, -70, -3, -100]]).astype(np.int32); end = np.concatenate([end, [5, 90, clen + 4, clen + 100]]).astype(np.int32)
    assert np.array_equal(ctx.span_query(beg, end).astype(np.int64), interval_minima(want, beg, end, clen)), (clen, m)
    beg = np.array([clen + 1, clen + 5, -9, 40, -3], np.int32); end = np.array([clen + 9, clen + 5, -2, 39, -3], np.int32)
    assert not ctx.span_query(beg, end).any(), (clen, m)
    return start, length, want


def test_span_build_contigs_in_sequence_and_tile_edges():
    """im_span_build call after call on ONE context, as test_depth_build_contigs_in_sequence_and_tile_edges does for the depth
    array: contigs that grow, shrink and grow again, clen + 1 a multiple of the scan's 8192-position tile, 32 / 33 / 1025 tiles,
    an empty build, the same build three times over"""
    from indelminer_amd import capi
    rng = np.random.default_rng(22)
    runs = [(int(s), int(s) + int(l)) for s, l in zip(rng.integers(-30, 5000, 900), rng.choice([19, 20, 21, 100], 900))]
    st = np.array([s for s, e in runs], np.int32); ln = np.array([e - s for s, e in runs], np.int32)
    for m in (1, 10):
        assert np.array_equal(span_of_run_arrays(st, ln, 5000, m), span_of_runs(runs, 5000, m))
    ctx = capi.Context(0)
    try:
        for clen, nrun, m in ((5000, 800, 10), (3_000_000, 900_000, 10), (100, 40, 1), (3_000_001, 900_000, 25),
                              (8191, 3000, 10), (32 * 8192 - 1, 80_000, 10), (32 * 8192, 80_000, 1), (1024 * 8192, 1_200_000, 10),
                              (70_000, 0, 3)):
            _span_case(ctx, rng, clen, nrun, m)
        clen = 33 * 8192 - 1
        start, length, want = _span_case(ctx, rng, clen, 90_000, 10)
        p = np.arange(clen + 1, dtype=np.int32)
        for _again in range(3):
            ctx.span_build(clen, start, length, 10)
            assert np.array_equal(ctx.span_query(p, p).astype(np.int64), want)
    finally:
        ctx.close()


def _depth_of(ctx, capi, clens, raw, off):
    """the pileup depth of every position from the same chunk: the triage's depth scatter, scanned and read back"""
    ctx.set_insert_ranges(["generic"], [700])
    ctx.depth_enable()
    n = len(off) - 1
    pipe = capi.Pipeline(ctx, n, len(raw), cap_cand=max(n, 16), want_depth=True)
    pipe.upload(raw, off)
    pipe.triage()
    pipe.sync()
    out = []
    for t, clen in enumerate(clens):
        ctx.depth_scan(t)
        p = np.arange(clen, dtype=np.int32)
        out.append(ctx.depth_query_tid(t, p, p + 1).astype(np.int64))
    return out


def test_span_never_exceeds_depth():
    """needs no restatement: a run that holds m bases on each side of the boundary in front of p covers p, so span[p] <= depth[p]
    (depth[] counts every pileup-eligible record, span[] those of them with mapq >= min_mapq)"""
    from indelminer_amd import rawrec, synth
    refs, rd = synth.simulate(seed=13, ref_len=80_000, coverage=30, n_contigs=2, big_every=7)
    clens = [len(r) for r in refs]
    raw, off = rawrec.records(rd)
    dev = Device(clens, 10, 10)
    try:
        dev.ctx.set_reference([r.tobytes() for r in refs])      # the triage decodes candidates against the real contigs
        dev.ctx.span_enable(10, 10)
        dev.scatter(raw, off)
        dev.scan()
        depth = _depth_of(dev.ctx, dev.capi, clens, raw, off)
        for t, clen in enumerate(clens):
            span = dev.every_position(t)
            assert span[clen] == 0
            assert (span[:clen] <= depth[t]).all() and span.max() > 0
    finally:
        dev.close()


def test_span_flank_one_is_the_smaller_neighbour_depth():
    """m = 1 on records whose CIGAR is one M: span[p] counts the reads that cover p - 1 and p.  depth[p - 1] = both + (reads that
    end in front of p), depth[p] = both + (reads that start at p), so span[p] == min(depth[p - 1], depth[p]) wherever not both
    of the other two kinds occur -- the records here start at multiples of 7 and end at 7 k + 3, so nowhere do they."""
    rng = np.random.default_rng(31)
    clen = 40_000
    starts = np.sort(rng.integers(0, (clen - 200) // 7, 6000)) * 7
    recs = [(0, int(s), 60, 0x63, [(0, int(7 * k + 3))]) for s, k in zip(starts, rng.integers(2, 20, len(starts)))]
    raw, off = raw_records(recs)
    dev = Device([clen], 1, 0)
    try:
        dev.scatter(raw, off)
        dev.scan()
        depth = _depth_of(dev.ctx, dev.capi, [clen], raw, off)[0]
        span = dev.every_position(0)
        assert depth.max() > 5
        assert span[0] == 0 and span[clen] == 0
        assert np.array_equal(span[1:clen], np.minimum(depth[:-1], depth[1:]))
    finally:
        dev.close()


# ------------------------------------------------------------------------------------------ the product

def _thd():
    spec = importlib.util.spec_from_file_location("thd_for_span", os.path.join(ROOT, "tests", "test_host_driver.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _run(binary, flags, cwd, ref, bam, env=None, vcf=None, sample="sample"):
    e = dict(os.environ)
    e.update(env or {})
    return subprocess.run([binary] + flags + [ref] + ([vcf] if vcf else []) + [sample + "=" + bam], cwd=cwd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=e)


def strip_columns(out):
    """a -G VCF without what -G adds: the ##FORMAT lines, the last two columns of the header line and of every record"""
    lines = []
    for ln in out.decode().split("\n"):
        if ln.startswith("##FORMAT="):
            continue
        if ln and not ln.startswith("##"):
            cols = ln.split("\t")
            assert len(cols) == 10, ln
            ln = "\t".join(cols[:8])
        lines.append(ln)
    return "\n".join(lines).encode()


def check_columns(out, bam, m, min_mapq, region=None, sample="sample"):
    """every GT:AD:GQ against the restatement computed from the BAM and the line's own POS, END, BP_END, NS.  region = (tid, beg,
    end): a -c run sees the records bam_fetch delivers for the stretch (those that overlap it), and counts those -- as its NS does."""
    refs, recs = read_bam_records(bam)
    if region is not None:
        rt, rb, re_ = region
        def overlaps(r):
            reflen = sum(ln for op, ln in r[4] if op in (0, 2, 3, 7, 8))
            return r[0] == rt and r[1] < re_ and r[1] + max(reflen, 1) > rb
        recs = [r for r in recs if overlaps(r)]
    span = span_of(recs, [l for _, l in refs], m, min_mapq)
    names = [n for n, _ in refs]
    text = out.decode().split("\n")
    fmt = [ln for ln in text if ln.startswith("##FORMAT=")]
    assert [ln.split(",")[0] for ln in fmt] == ["##FORMAT=<ID=GT", "##FORMAT=<ID=AD", "##FORMAT=<ID=GQ"]
    assert "Number=2" in fmt[1] and "upper bound" in fmt[1]
    assert text.index(fmt[0]) > max(i for i, ln in enumerate(text) if ln.startswith("##INFO="))
    head = [ln for ln in text if ln.startswith("#CHROM")]
    assert head == ["#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\t" + sample]
    n = 0
    kinds = set()
    for ln in text:
        if not ln or ln.startswith("#"):
            continue
        cols = ln.split("\t")
        assert cols[8] == "GT:AD:GQ", ln
        info = dict(kv.split("=") for kv in cols[7].split(";") if "=" in kv)
        pos, end, bp_end, ns = int(cols[1]), int(info["END"]), int(info["BP_END"]), int(info["NS"])
        if "PAIRED_READ" in cols[7].split(";"):
            assert cols[9] == "./.:.,%d:." % ns, ln
        else:
            sp = span[names.index(cols[0])]
            rs = int(sp[pos:pos + (bp_end - end) + 1].min())
            gt, gq = genotype_of(rs, ns)
            assert cols[9] == "%s:%d,%d:%d" % (gt, rs, ns, gq), (ln, rs)
            kinds.add(gt)
        n += 1
    return n, kinds


def test_genotype_rule_restated():
    """the integer rule on cases worked by hand (thousandths of a phred: E = 20000, C = 44, H = 3010)"""
    assert genotype_of(0, 2) == ("1/1", 6)                 # L = 40000, 6020, 88 -> second is 5932
    assert genotype_of(24, 0) == ("0/0", 71)               # L = 1056, 72240, 480000 -> 71184
    assert genotype_of(10, 10) == ("0/1", 99)              # L = 200440, 60200, 200440
    assert genotype_of(1, 1) == ("0/1", 14)                # L = 20044, 6020, 20044 -> 14024
    assert genotype_of(3, 0) == ("0/0", 9)                 # L = 132, 9030, 60000 -> 8898
    assert genotype_of(0, 1)[0] == "1/1" and genotype_of(1, 0)[0] == "0/0"


@pytest.mark.parametrize("name,flags", [("default_config", ["-i", "indelminer.config"]), ("default_noconfig", [])])
def test_product_genotype_columns_test_data(name, flags):
    prod = _product()
    bam = os.path.join(TD, "alignments.bam")
    r = _run(prod, flags + ["-G"], TD, "reference.fa", "alignments.bam")
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    assert strip_columns(r.stdout) == _golden(name)                                     # (a)
    n, _ = check_columns(r.stdout, bam, 10, 10)                                         # (b)
    assert n == sum(1 for ln in _golden(name).split(b"\n") if ln and not ln.startswith(b"#")) > 0
    h = _run(prod, flags + ["-G"], TD, "reference.fa", "alignments.bam", env={"INDELMINER_PIPELINE": "host"})
    assert h.returncode == 0 and h.stdout == r.stdout                                   # (c)
    # -n and -q move the flank and the mapping-quality gate of the reference side with them
    r2 = _run(prod, ["-i", "indelminer.config", "-b", "40", "-n", "15", "-q", "30", "-G"], TD, "reference.fa", "alignments.bam")
    assert r2.returncode == 0, r2.stderr.decode()[-2000:]
    check_columns(r2.stdout, bam, 15, 30)
    # without -G: the parent's bytes
    assert _run(prod, flags, TD, "reference.fa", "alignments.bam").stdout == _golden(name)


def test_product_genotype_columns_region():
    """(d) -c: the span array is built in region runs too (the depth array is not)"""
    prod = _product()
    flags = ["-i", "indelminer.config", "-c", "reference:1-5000", "-G"]
    r = _run(prod, flags, TD, "reference.fa", "alignments.bam")
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    assert strip_columns(r.stdout) == _golden("region")
    n, _ = check_columns(r.stdout, os.path.join(TD, "alignments.bam"), 10, 10, region=(0, 0, 5000))
    assert n > 0
    h = _run(prod, flags, TD, "reference.fa", "alignments.bam", env={"INDELMINER_PIPELINE": "host"})
    assert h.returncode == 0 and h.stdout == r.stdout


@pytest.fixture(scope="module")
def synth_1mb(tmp_path_factory):
    return _thd()._synth_dir(tmp_path_factory, "synth_1mb_30x")


def test_product_genotype_columns_synthetic_1mb(synth_1mb):
    prod = _product()
    flags = ["-i", "cfg.txt", "-G"]
    r = _run(prod, flags, synth_1mb, "ref.fa", "aln.bam")
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    assert strip_columns(r.stdout) == _golden("synth_1mb_30x")
    n, kinds = check_columns(r.stdout, os.path.join(synth_1mb, "aln.bam"), 10, 10)
    assert n > 100 and "1/1" in kinds                       # the simulator's sample carries every indel on all its reads
    for env in ({"INDELMINER_PIPELINE": "host"}, {"INDELMINER_PIECE_BYTES": "120000", "INDELMINER_WALKERS": "3"}):
        h = _run(prod, flags, synth_1mb, "ref.fa", "aln.bam", env=env)
        assert h.returncode == 0 and h.stdout == r.stdout, env
    # a stretch of it
    rg = _run(prod, ["-i", "cfg.txt", "-c", "ctg0:200,001-640,000", "-G"], synth_1mb, "ref.fa", "aln.bam")
    assert rg.returncode == 0, rg.stderr.decode()[-2000:]
    plain = _run(prod, ["-i", "cfg.txt", "-c", "ctg0:200,001-640,000"], synth_1mb, "ref.fa", "aln.bam")
    assert strip_columns(rg.stdout) == plain.stdout
    check_columns(rg.stdout, os.path.join(synth_1mb, "aln.bam"), 10, 10, region=(0, 200_000, 640_000))
    # -o detailed ignores -G
    d0 = _run(prod, ["-i", "cfg.txt", "-o", "detailed"], synth_1mb, "ref.fa", "aln.bam")
    d1 = _run(prod, ["-i", "cfg.txt", "-o", "detailed", "-G"], synth_1mb, "ref.fa", "aln.bam")
    assert d1.returncode == 0 and d1.stdout == d0.stdout and len(d0.stdout) > 0


def _mixed_sample(tmp_path):
    """reads of two simulated samples with the same genome and germline indels, one of them with further (somatic) indels, in one
    BAM: the germline indels are on every read, the somatic ones on about half -- a sample with 1/1 and 0/1 sites"""
    from indelminer_amd import bamwrite, synth
    kw = dict(seed=6, ref_len=120_000, coverage=15, n_contigs=2)
    refs, a = synth.simulate(**kw)
    refs_b, b = synth.simulate(read_seed=77, somatic_spacing=6_000, **kw)
    assert all(np.array_equal(x, y) for x, y in zip(refs, refs_b))
    rd = synth.Reads()
    order = np.lexsort((np.concatenate([a.pos, b.pos]), np.concatenate([a.tid, b.tid])))
    for k in ("tid", "pos", "flag", "mpos", "isize", "seq", "cig_op", "cig_len", "ncig", "mate_first"):
        setattr(rd, k, np.concatenate([getattr(a, k), getattr(b, k)])[order])
    rd.pair_id = np.concatenate([a.pair_id, b.pair_id + int(a.pair_id.max()) + 1])[order]
    rd.n, rd.read_len, rd.range_max, rd.mapq = a.n + b.n, a.read_len, a.range_max, a.mapq
    contigs = [("ctg%d" % i, len(r)) for i, r in enumerate(refs)]
    bamwrite.write_fasta(str(tmp_path / "ref.fa"), contigs, refs)
    bamwrite.write_bam(str(tmp_path / "aln.bam"), contigs, rd)
    (tmp_path / "cfg.txt").write_text("IL generic 300 700\n")
    return str(tmp_path)


def test_product_genotype_columns_mixed_sample(tmp_path):
    """sites where reference-spanning reads exist: AD's first number is not zero, GT takes more than one value"""
    prod = _product()
    d = _mixed_sample(tmp_path)
    plain = _run(prod, ["-i", "cfg.txt"], d, "ref.fa", "aln.bam")
    assert plain.returncode == 0, plain.stderr.decode()[-2000:]
    r = _run(prod, ["-i", "cfg.txt", "-G"], d, "ref.fa", "aln.bam")
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    assert strip_columns(r.stdout) == plain.stdout
    n, kinds = check_columns(r.stdout, os.path.join(d, "aln.bam"), 10, 10)
    assert n > 50 and {"0/1", "1/1"} <= kinds, (n, kinds)
    ad_ref = [int(ln.split("\t")[9].split(":")[1].split(",")[0]) for ln in r.stdout.decode().split("\n") if ln and ln[0] != "#" and "./." not in ln.split("\t")[9]]
    assert sum(1 for x in ad_ref if x >= 5) >= 10
    for env in ({"INDELMINER_PIPELINE": "host"}, {"INDELMINER_PIECE_BYTES": "60000", "INDELMINER_WALKERS": "3"}):
        h = _run(prod, ["-i", "cfg.txt", "-G"], d, "ref.fa", "aln.bam", env=env)
        assert h.returncode == 0 and h.stdout == r.stdout, env
    # other -n / -q: the reference side follows
    r2 = _run(prod, ["-i", "cfg.txt", "-n", "20", "-q", "60", "-G"], d, "ref.fa", "aln.bam")
    assert r2.returncode == 0, r2.stderr.decode()[-2000:]
    n2, _ = check_columns(r2.stdout, os.path.join(d, "aln.bam"), 20, 60)
    assert n2 > 50


def test_product_genotype_columns_survive_the_hand_over(tmp_path):
    """(e) a read with more indels than the kernels hold: the pipelined run hands over to the record-at-a-time child, -G with it"""
    thd = _thd()
    prod = _product()
    thd._many_indels_in_one_read(prod, tmp_path, ())        # writes the input, checks the shim's output against the reference's
    d = str(tmp_path)
    want = thd._run(thd._build_shim(), ["-i", "cfg.txt"], d, ref="ref.fa", bam="aln.bam", env={"INDELMINER_PIPELINE": "host"})
    r = _run(prod, ["-i", "cfg.txt", "-G"], d, "ref.fa", "aln.bam", env={"INDELMINER_DEBUG_HANDOFF": "1"})
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    assert b"[handoff]" in r.stderr
    assert strip_columns(r.stdout) == want
    n, _ = check_columns(r.stdout, os.path.join(d, "aln.bam"), 10, 10)
    assert n > 10


def test_product_annotate_reads_a_genotyped_vcf(tmp_path):
    """(f) annotate mode fed a VCF that -G wrote prints what it prints for the plain one; (g) -G itself is refused there"""
    thd = _thd()
    prod = _product()
    spec = importlib.util.spec_from_file_location("make_golden", os.path.join(GOLD, "make_golden.py"))
    mg = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mg)
    d = str(tmp_path)
    mg.write_dataset(d, mg.SYNTH_TN["tumor"], "tumor_")
    mg.write_dataset(d, mg.SYNTH_TN["normal"], "normal_")
    t = _run(prod, ["-i", "cfg.txt", "-G"], d, "ref.fa", "tumor_aln.bam", sample="t")
    assert t.returncode == 0, t.stderr.decode()[-2000:]
    assert strip_columns(t.stdout) == _golden("synth_tn_tumor")
    check_columns(t.stdout, os.path.join(d, "tumor_aln.bam"), 10, 10, sample="t")
    open(os.path.join(d, "tumor_g.vcf"), "wb").write(t.stdout)
    a = _run(prod, ["-i", "cfg.txt", "-q", "0", "-a", "-e", "1"], d, "ref.fa", "normal_aln.bam", vcf="tumor_g.vcf", sample="normal")
    assert a.returncode == 0, a.stderr.decode()[-2000:]
    assert a.stdout == _golden("synth_tn_annotate")
    g = _run(prod, ["-i", "cfg.txt", "-q", "0", "-a", "-e", "1", "-G"], d, "ref.fa", "normal_aln.bam", vcf="tumor_g.vcf", sample="normal")
    assert g.returncode != 0 and g.stdout == b""
    assert b"-G is not available with a VCF argument" in g.stderr
    w = _run(prod, ["-i", "cfg.txt", "-G"], d, "ref.fa", "tumor_aln.bam", sample="t", env={"WORLD_SIZE": "2", "RANK": "0"})
    assert w.returncode != 0 and w.stdout == b"" and b"-G is not available with more than one rank" in w.stderr
