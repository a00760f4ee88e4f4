"""What tests/test_gpu_junction_gt.py and tests/test_junction_gt_host.py share: the plain restatement of the junction genotypes (-K),
written from the rule in include/indelminer_amd.h (seam 5, "Junction genotypes"), not from the code under test; the restatement of -J's
FILE with -K, built on tests/support/splitjunctions.py's; and a data set with planted truth.

A JUNCTION is (t1, p1, s1, t2, p2, s2, E, n1, n2), as in tests/support/splitjunctions.py.  SPANS is one array per contig, span[0 .. clen]
of seam 5.  A CALL is (GT, RS, ALT, GQ, RS1, RS2).  Everything is an integer and every comparison is exact.
"""
import struct

import numpy as np

from tests.support import splitjunctions as sj
from tests.support import splitlinks as sl
from tests.support.spanarrays import genotype_of

FLANK, MIN_MAPQ = 10, 10                        # the driver's -n and -q as the tests run it


# ---------------------------------------------------------------------- the rule

def call(junction, spans, dup_correction=True):
    """the call of one junction; dup_correction=False: the rule without its exception, which the tests show to be wrong"""
    t1, p1, s1, t2, p2, s2, _e, n1, n2 = junction
    rs1, rs2 = int(spans[t1][p1]), int(spans[t2][p2])
    alt = n1 + n2
    rs = min(rs1, rs2)
    if dup_correction and sj.jt_of(t1, s1, t2, s2) == "DUP":
        rs = max(0, rs - alt)
    gt, gq = genotype_of(rs, alt)
    return gt, rs, alt, gq, rs1, rs2


def calls(found, spans, dup_correction=True):
    return [call(j, spans, dup_correction) for j in found]


def ends_minima(spans, tid, pos, slack):
    """what im_span_query_ends answers: per end the minimum of span[p] of its contig over [pos - slack, pos + slack] clipped to it"""
    out = []
    for t, p in zip(tid, pos):
        a = spans[int(t)]
        out.append(int(a[max(int(p) - slack, 0):min(int(p) + slack, len(a) - 1) + 1].min()))
    return np.array(out, np.int64)


# ---------------------------------------------------------------------- span[] from a BAM file, restated once more

def _runs(pos, cigar):
    """the maximal M / = / X runs [(s, e)] of one record, unclipped"""
    out, x, s = [], pos, None
    for op, ln in cigar + [(4, 0)]:
        if op in (0, 7, 8):
            s = x if s is None else s
            x += ln
            continue
        if s is not None:
            out.append((s, x))
            s = None
        if op in (2, 3):
            x += ln
    return out


def spans_of_bam(bam, m=FLANK, q=MIN_MAPQ):
    """(names, clens, spans): span[p] counts the runs [s, e) of the eligible records with s <= p - m and p + m <= e"""
    from indelminer_amd import rawrec
    raw, off, contigs = rawrec.records_from_bam(bam)
    names, clens = [n for n, _ in contigs], [n for _, n in contigs]
    diff = [np.zeros(n + 2, np.int64) for n in clens]
    for b in sl.split_raw(raw, off):
        tid, pos, l_qname, mapq, _bin, n_cig, flag = struct.unpack_from("<iiBBHHH", b, 0)
        if flag & (0x4 | 0x100 | 0x200 | 0x400) or not 0 <= tid < len(clens) or mapq < q:
            continue
        cigar = [(w & 15, w >> 4) for w in struct.unpack_from("<%dI" % n_cig, b, 32 + l_qname)]
        for s, e in _runs(pos, cigar):
            s, e = max(s, 0), min(e, clens[tid])
            if e - s >= 2 * m:
                diff[tid][s + m] += 1
                diff[tid][e - m + 1] -= 1
    return names, clens, [np.cumsum(d)[:n + 1] for d, n in zip(diff, clens)]


# ---------------------------------------------------------------------- FILE with -K

FORMATS = (
    "##FORMAT=<ID=GT,Number=1,Type=String,Description=\"Genotype of the junction, the most likely of 0/0, 0/1, 1/1 given AD\">\n"
    "##FORMAT=<ID=AD,Number=2,Type=Integer,Description=\"Read support of the reference and the junction allele: RS, the smaller number of RB (for JT=DUP "
    "less the second number here, not below 0), and the sum of the two numbers of SR\">\n"
    "##FORMAT=<ID=GQ,Number=1,Type=Integer,Description=\"Genotype quality: phred-scaled distance to the second most likely genotype, at most 99\">\n"
    "##FORMAT=<ID=RB,Number=2,Type=Integer,Description=\"Alignments that match the reference for the -n distance on both sides of the boundary behind "
    "base POS, and of the one behind base POS2\">\n")
JUNCTION_GENOTYPE = (
    "##junctionGenotype=\"every junction against the reads that run through its two ends on the reference allele: ALT is the sum of the two numbers of SR "
    "(a split read stores one link, at its primary record, so the two are disjoint sets of reads); RB=RS1,RS2 are -G's count of alignments at or above -q "
    "that match the reference for the -n distance on both sides, the smallest within 0 bases of the boundary behind base POS and of the one behind "
    "base POS2, which is where a clip on either side puts the junction (a split read's own alignment ends there and is in neither); RS is the "
    "smaller of RS1 and RS2, except for JT=DUP, where RS is that less ALT and not below 0: a tandem duplication keeps both outer boundaries of the "
    "duplicated segment intact on the duplicated allele, so every copy of that allele adds reference-looking reads at POS and at POS2 at the rate at which "
    "it adds split reads, and a homozygous duplication would show RS about ALT and never be called 1/1; GT and GQ are -G's, the same integers from AD=RS,ALT; "
    "a reference read must hold -n bases on either side while a split read needs a clip of 20 bases and a placed remainder, so the two alleles are not "
    "equally detectable and nothing corrects for it; RS is exact for one position while micro-homology lets an aligner place the split anywhere inside it; "
    "a read with an indel near an end may count on neither side; the two junctions of an inversion or of a reciprocal translocation are genotyped "
    "independently; the records of -U, -N and -T have no genotype\"\n")
CHROM = "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\n"


def header(sample="sample"):
    """-J's header with what -K adds: four ##FORMAT lines behind the ##INFO lines, other words in ##splitJunctions where it said "no
    genotype", the ##junctionGenotype line behind it, FORMAT and the sample's name in the column line"""
    h = sj.HEADER
    assert h.endswith(CHROM) and h.count("; no genotype; ") == 1 and h.count("##splitJunctions=") == 1
    at = h.index("##splitJunctions=")
    h = h[:at] + FORMATS + h[at:-len(CHROM)].replace("; no genotype; ", "; the genotype is that of ##junctionGenotype; ")
    return h + JUNCTION_GENOTYPE + CHROM[:-1] + "\tFORMAT\t" + sample + "\n"


def render(names, refs, found, spans, sample="sample", dup_correction=True):
    """FILE as the driver writes it with -K (found None: after an overflow, this header alone)"""
    plain = sj.render(names, refs, found).decode()
    assert plain.startswith(sj.HEADER)
    body = plain[len(sj.HEADER):].split("\n")[:-1]
    kept = [j for j in found or [] if j[1] != 0 and j[4] != 0]
    assert len(body) == len(kept)
    lines = [header(sample)]
    for ln, j in zip(body, kept):
        lines.append("%s\tGT:AD:GQ:RB\t%s:%d,%d:%d:%d,%d\n" % ((ln,) + call(j, spans, dup_correction)))
    return "".join(lines).encode()


def render_of_bam(bam, fasta_path, q=MIN_MAPQ, m=FLANK, overflowed=False, sample="sample"):
    """(FILE with -K, junctions, calls) from BAM + FASTA with the driver's constants"""
    from tests.support import cliptails as ct
    names, clens, links = sl.links_of_bam(bam, sl.MIN_CLIP, q)
    fasta = ct.read_fasta(fasta_path)
    refs = [fasta[n] for n in names]
    found = sj.junctions(links, clens)
    spans = spans_of_bam(bam, m, q)[2]
    return render(names, refs, None if overflowed else found, spans, sample), found, calls(found, spans)


# ---------------------------------------------------------------------- the cases worked by hand

# (name, junction, (span at p1, span at p2), the call worked by hand): contig 0 has 1 000 positions, contig 1 has 500
HAND_CLENS = [1_000, 500]
HAND = [
    # L = (ALT * 20000 + RS * 44, (ALT + RS) * 3010, ALT * 44 + RS * 20000) in thousandths of a phred
    ("DEL, RS1 < RS2", (0, 100, 0, 0, 400, 1, 6, 4, 2), (7, 9), ("0/1", 7, 6, 81, 7, 9)),           # 120308, 39130, 140264: 81178
    ("DEL, RS1 > RS2", (0, 100, 0, 0, 400, 1, 6, 4, 2), (9, 7), ("0/1", 7, 6, 81, 9, 7)),
    ("INV 3to3", (0, 100, 0, 0, 400, 0, 3, 3, 0), (0, 5), ("1/1", 0, 3, 9, 0, 5)),                   # 60000, 9030, 132: 8898
    ("INV 5to5", (0, 100, 1, 0, 400, 1, 3, 0, 3), (3, 3), ("0/1", 3, 3, 42, 3, 3)),                  # 60132, 18060, 60132: 42072
    ("TRA, the sides of a DUP on two contigs: no correction", (0, 100, 1, 1, 400, 0, 3, 1, 2), (3, 4), ("0/1", 3, 3, 42, 3, 4)),
    ("DUP, min(RS1, RS2) below ALT", (0, 100, 1, 0, 400, 0, 5, 3, 2), (4, 6), ("1/1", 0, 5, 15, 4, 6)),      # 100000, 15050, 220: 14830
    ("DUP, equal to ALT", (0, 100, 1, 0, 400, 0, 5, 3, 2), (6, 5), ("1/1", 0, 5, 15, 6, 5)),
    ("DUP, above ALT", (0, 100, 1, 0, 400, 0, 5, 3, 2), (9, 12), ("0/1", 4, 5, 53, 9, 12)),                  # 100176, 27090, 80220: 53130
    ("ALT 3 against RS 0", (0, 100, 0, 1, 400, 1, 3, 3, 0), (0, 0), ("1/1", 0, 3, 9, 0, 0)),
    ("ALT 3 against RS 3", (0, 100, 0, 1, 400, 1, 3, 3, 0), (3, 3), ("0/1", 3, 3, 42, 3, 3)),
    ("ALT 3 against RS 300", (0, 100, 0, 1, 400, 1, 3, 3, 0), (300, 300), ("0/0", 300, 3, 99, 300, 300)),    # 73200, 912030, 6000132
    ("GQ of 99", (0, 100, 0, 0, 400, 1, 20, 10, 10), (20, 21), ("0/1", 20, 20, 99, 20, 21)),                 # 400880, 120400, 400880
    # 0 : 0 makes every genotype cost nothing: the lower index wins.  The driver's threshold of 3 links keeps such a record out of FILE
    ("a tie, which the lower index wins", (0, 100, 0, 0, 400, 1, 0, 0, 0), (0, 0), ("0/0", 0, 0, 0, 0, 0)),
    ("an end at position 0 of the array and one at the contig's length", (0, 0, 1, 1, 500, 0, 3, 3, 0), (2, 1), ("0/1", 1, 3, 8, 2, 1)),      # 60044, 12040, 20132: 8092
]


def hand_spans(junction, at):
    spans = [np.zeros(n + 1, np.int64) for n in HAND_CLENS]
    spans[junction[0]][junction[1]] = at[0]
    spans[junction[3]][junction[4]] = at[1]
    return spans


# ---------------------------------------------------------------------- the data set with planted truth

CONTIG = 20_000
PER_COPY = 10                                   # reads per allele copy
# (what, a = the end the reads are clipped on their right at, b = the end they are clipped on their left at, reference reads through each
# end, split reads): a split read runs up to base a - 1 and goes on at base b -- forwards for a deletion, a < b; back to the start of the
# duplicated segment for a tandem duplication, a > b
PLANTED = [
    ("heterozygous DEL", 3_000, 4_000, PER_COPY, PER_COPY),
    ("homozygous DEL", 7_000, 8_000, 0, 2 * PER_COPY),
    ("heterozygous DUP", 12_000, 11_000, 2 * PER_COPY, PER_COPY),
    ("homozygous DUP", 16_000, 15_000, 2 * PER_COPY, 2 * PER_COPY),
]
PLANTED_GT = ["0/1", "1/1", "0/1", "1/1"]                                           # in FILE's order, which is the order above
PLANTED_COLUMN = ["0/1:10,10:99:10,10", "1/1:0,20:59:0,0", "0/1:10,10:99:20,20", "1/1:0,20:59:20,20"]
PLANTED_WITHOUT_THE_CORRECTION = ["0/1", "1/1", "0/1", "0/1"]


def planted_truth():
    """(refs, rd): one contig of 20 000 random bases and, per site of PLANTED, reads of 100 bases in proper pairs whose mates lie 400 to
    500 bases away from every end: plain reads through either end (5 bases apart, 25 bases or more on either side), and split reads across
    the junction that carry the bases of both ends and the SA tag a split aligner would have written, alternately with the part in front
    of the junction and the part behind it as the primary record.  A few hundred records, no differences from the reference."""
    from indelminer_amd import synth
    rng = np.random.default_rng(77)
    ref = rng.choice(np.frombuffer(b"ACGT", np.uint8), CONTIG)
    L = 100
    rows = []                                   # (pos, flag, cigar [(len, op)], seq, mate pos, isize, pair id, tags or None)

    def pair(pos, cigar, seq, mate_behind, reverse_tag_of=None):
        """one site read and its plain mate, 400 bases behind it or in front of it; the site read is the forward one of a pair whose
        mate lies behind, the reverse one otherwise"""
        pid = len(rows) // 2
        mpos = pos + 400 if mate_behind else pos - 400
        lo, hi = min(pos, mpos), max(pos, mpos)
        isize = hi + L - lo
        fwd, rev = 0x1 | 0x2 | 0x20 | 0x40, 0x1 | 0x2 | 0x10 | 0x80
        flag = fwd if mate_behind else rev
        tags = reverse_tag_of(bool(flag & 0x10)) if reverse_tag_of else None
        rows.append((pos, flag, cigar, seq, mpos, isize if mate_behind else -isize, pid, tags))
        rows.append((mpos, rev if mate_behind else fwd, [(L, synth.OP_M)], ref[mpos:mpos + L].copy(), pos, -isize if mate_behind else isize, pid, None))

    for _what, a, b, n_ref, n_split in PLANTED:
        for end in (a, b):
            for i in range(n_ref):
                pos = end - 75 + 5 * (i % 10) + (i // 10)
                pair(pos, [(L, synth.OP_M)], ref[pos:pos + L].copy(), mate_behind=end == max(a, b))
        for i in range(n_split):
            x = 40 + 4 * (i // 2 % 10)          # bases in front of the junction: 40 .. 76, so either part has 24 bases or more
            seq = np.concatenate([ref[a - x:a], ref[b:b + L - x]])
            if i % 2 == 0:                      # the part in front is the primary: xM(L - x)S, clipped on its right at a
                tag = lambda reverse, x=x, b=b: sl.sa(sl.sa_value(L, 0, x, reverse, "ctg0", b, 1, 0)[0])
                pair(a - x, [(x, synth.OP_M), (L - x, synth.OP_S)], seq, mate_behind=a == max(a, b), reverse_tag_of=tag)
            else:                               # the part behind is: xS(L - x)M, clipped on its left at b
                tag = lambda reverse, x=x, a=a: sl.sa(sl.sa_value(L, 1, x, reverse, "ctg0", a, 0, 0)[0])
                pair(b, [(x, synth.OP_S), (L - x, synth.OP_M)], seq, mate_behind=b == max(a, b), reverse_tag_of=tag)

    order = sorted(range(len(rows)), key=lambda k: rows[k][0])          # stable
    rd = synth.Reads()
    rd.n, rd.read_len, rd.mapq, rd.range_max = len(rows), L, 60, 700
    rd.tid = np.zeros(rd.n, np.int64)
    rd.pos = np.array([rows[k][0] for k in order]); rd.flag = np.array([rows[k][1] for k in order])
    rd.mpos = np.array([rows[k][4] for k in order]); rd.isize = np.array([rows[k][5] for k in order]); rd.pair_id = np.array([rows[k][6] for k in order])
    rd.mate_first = (rd.flag & 0x40) != 0
    rd.ncig = np.array([len(rows[k][2]) for k in order])
    rd.cig_len = np.zeros((rd.n, 2), np.int64); rd.cig_op = np.zeros((rd.n, 2), np.int64)
    rd.seq = np.zeros((rd.n, L), np.uint8)
    rd.overrides = {}
    for i, k in enumerate(order):
        for j, (ln, op) in enumerate(rows[k][2]):
            rd.cig_len[i, j], rd.cig_op[i, j] = ln, op
        rd.seq[i] = rows[k][3]
        if rows[k][7] is not None:
            rd.overrides[i] = {"tags": b"MQC" + bytes([60]) + rows[k][7]}
    return [ref], rd


def write_planted(d, refs, rd):
    """ref.fa, aln.bam (+ .bai) and cfg.txt in directory d"""
    from tests.support import intercontig
    return intercontig.write_planted(d, refs, rd)
