"""What tests/test_gpu_splitoverlap.py and tests/test_splitoverlap_host.py share: the plain restatement of the junction overlap (-H),
written from the rule in include/indelminer_amd.h (seam 5, "Junction overlap"), not from the code under test; the restatement of -J's
FILE with -H, built on tests/support/splitjunctions.py's (and, with -K, on tests/support/junctiongt.py's); cases worked by hand; and a
data set with planted truth.

A LINK is (tA, pA, sA, tB, pB, sB) and a JUNCTION (t1, p1, s1, t2, p2, s2, E, n1, n2), as in tests/support/splitjunctions.py.  A PAIR
is (link, d), d an integer or None for unknown.  A SUMMARY is (known, median, agree).  Everything is an integer and every comparison is
exact.
"""
import struct

import numpy as np

from tests.support import splitjunctions as sj
from tests.support import splitlinks as sl

WINDOW = sj.WINDOW
D_MAX = 32767
UNKNOWN = -32768                                # what im_splitlink_add_overlap takes for "unknown"
READ_OPS = (0, 1, 7, 8)                         # M I = X
CLIPS = (4, 5)                                  # S H


# ---------------------------------------------------------------------- the rule

def overlap_of(rec, names, clens, c, q):
    """(link, d) of one delivered record, d None for unknown; None when the record stores no link (sl.link_of has that rule)"""
    link = sl.link_of(rec, names, clens, c, q)
    if link is None:
        return None
    b = bytes(rec)
    _tid, _pos, l_qname, _mapq, bin_, n_cigar, flag, l_seq = struct.unpack_from("<iiBBHHHi", b, 0)
    o_cigar = 32 + l_qname
    ops = [(w >> 4, w & 15) for w in struct.unpack_from("<%dI" % n_cigar, b, o_cigar)]
    lead = 0
    while ops[lead][1] in CLIPS:
        lead += 1
    trail = len(ops)
    while ops[trail - 1][1] in CLIPS:
        trail -= 1
    L1, T1 = sum(n for n, _ in ops[:lead]), sum(n for n, _ in ops[trail:])
    Q1 = L1 + T1 + sum(n for n, op in ops if op in READ_OPS)
    o_aux = o_cigar + 4 * n_cigar + (l_seq + 1) // 2 + (0 if bin_ == 0xFFFF else l_seq)
    o = sl.find_tag(b, o_aux, b"SA")
    m = sl.ENTRY.fullmatch(b[o + 1:b.find(b"\0", o + 1)])
    sa_ops = [(int(n), sl.OPS.index(chr(op[0]))) for n, op in sl.CIGAR_OP.findall(m.group(4))]
    Q2 = sum(n for n, op in sa_ops if op in READ_OPS + CLIPS)
    L2 = sa_ops[0][0] if sa_ops[0][1] in CLIPS else 0
    T2 = sa_ops[-1][0] if sa_ops[-1][1] in CLIPS else 0
    if (m.group(3) == b"-") != bool(flag & 0x10):
        L2, T2 = T2, L2
    if Q1 != Q2:
        return link, None
    d = (Q1 - T1) - L2 if link[2] == 0 else (Q1 - T2) - L1          # end A on side 0 is BEHIND, on side 1 FRONT
    return link, (d if -D_MAX <= d <= D_MAX else None)


def overlaps_of(records, names, clens, c, q):
    return [x for x in (overlap_of(r, names, clens, c, q) for r in records) if x is not None]


def overlaps_of_bam(bam, c=sl.MIN_CLIP, q=sl.MIN_MAPQ):
    """(contig names, contig lengths, pairs) of a BAM file"""
    from indelminer_amd import rawrec
    raw, off, contigs = rawrec.records_from_bam(bam)
    names, clens = [n for n, _ in contigs], [n for _, n in contigs]
    return names, clens, overlaps_of(sl.split_raw(raw, off), names, clens, c, q)


def summary(ds):
    """(known, median, agree) of a multiset of d: its known elements, their lower median (0 of none) and how many equal it"""
    ds = sorted(d for d in ds if d is not None)
    if not ds:
        return 0, 0, 0
    med = ds[(len(ds) - 1) // 2]
    return len(ds), med, ds.count(med)


def junction_ds(pairs, clens, junction, window=WINDOW):
    """the d, known or not, of every stored link that one of rule 5's two count queries counts, each link once"""
    t1, p1, s1, t2, p2, s2 = junction[:6]
    q1 = (t1, s1, p1 - window, p1 + window, t2, s2, p2 - window, p2 + window)
    q2 = (t2, s2, p2 - window, p2 + window, t1, s1, p1 - window, p1 + window)
    return [d for l, d in pairs if sl.count([l], clens, q1) or sl.count([l], clens, q2)]


def junction_summary(pairs, clens, junction, window=WINDOW):
    return summary(junction_ds(pairs, clens, junction, window))


def summaries_fast(pairs, clens, junctions, window=WINDOW):
    """the same answers for the soak: the pairs in a dictionary by (contigs, sides), nothing else changed"""
    by_kind = {}
    for k, (l, d) in enumerate(pairs):
        by_kind.setdefault((l[0], l[2], l[3], l[5]), []).append((k, l, d))
    out = []
    for j in junctions:
        t1, p1, s1, t2, p2, s2 = j[:6]
        seen = {}
        for ta, pa, sa, tb, pb, sb in ((t1, p1, s1, t2, p2, s2), (t2, p2, s2, t1, p1, s1)):
            a0, a1, b0, b1 = max(pa - window, 0), min(pa + window, clens[ta]), max(pb - window, 0), min(pb + window, clens[tb])
            for k, l, d in by_kind.get((ta, sa, tb, sb), []):
                if a0 <= l[1] <= a1 and b0 <= l[4] <= b1:
                    seen[k] = d
        out.append(summary(seen.values()))
    return out


# ---------------------------------------------------------------------- FILE with -H

INFOS = (
    "##INFO=<ID=HOMLEN,Number=1,Type=Integer,Description=\"Micro-homology at the junction: the read bases that both parts of a split read align, "
    "the lower median over the reads of SR that state it; 0 when that median is an insertion\">\n"
    "##INFO=<ID=INSLEN,Number=1,Type=Integer,Description=\"Inserted bases at the junction: the read bases between the two parts of a split read that "
    "neither aligns, from the same median; 0 when it is a homology\">\n"
    "##INFO=<ID=OA,Number=2,Type=Integer,Description=\"Overlap agreement: the reads of SR whose own overlap equals that median, and the reads of SR "
    "that state one\">\n")
JUNCTION_OVERLAP = (
    "##junctionOverlap=\"every split read states its own overlap d in its two CIGARs: with L1, T1 the clipped bases (S and H) in front of and behind "
    "the primary alignment, L2, T2 those of the SA entry (exchanged when the entry is on the other strand), Q1 = L1 + T1 + the primary's M, I, = and X "
    "bases and Q2 the entry's M, I, S, H, = and X bases, d = Q1 - T1 - L2 when the entry aligns the bases behind the primary's and d = Q1 - T2 - L1 "
    "when it aligns those in front; d above 0 is that many read bases aligned by both parts (micro-homology), d below 0 that many aligned by "
    "neither (inserted bases), 0 a clean junction; a read with Q1 other than Q2 or with d outside -32767 .. 32767 states none; over the reads of "
    "SR, from either end, within 32 bases at both ends, that state one, OA=agree,known gives their number and how many equal their lower "
    "median (the element of index (known - 1) / 2 in ascending order), HOMLEN is that median when above 0 and INSLEN its negative when below, "
    "each 0 otherwise; HOMLEN=.;INSLEN=.;OA=0,0 when no read states one; no inserted sequence is printed (that needs read bases), there is "
    "no CIPOS, d is what the aligner says and is not compared with the reference, so a junction above 32 bases of homology is described as well; "
    "the records of -U, -N and -T are not touched\"\n")


def info_of(s):
    """what -H appends to a record's INFO"""
    known, med, agree = s
    if known == 0:
        return ";HOMLEN=.;INSLEN=.;OA=0,0"
    return ";HOMLEN=%d;INSLEN=%d;OA=%d,%d" % (max(0, med), max(0, -med), agree, known)


def with_overlap(text, summaries):
    """a FILE of -J (with or without -K) as it is written with -H: the three ##INFO lines behind the present ones, the ##junctionOverlap
    line as the last description line, and the keys of info_of at the very end of INFO of every record, in order"""
    lines = text.decode().split("\n")
    assert lines[-1] == ""
    last_info = max(i for i, ln in enumerate(lines) if ln.startswith("##INFO"))
    chrom = next(i for i, ln in enumerate(lines) if ln.startswith("#CHROM"))
    assert len(lines) - 1 - (chrom + 1) == len(summaries)
    out = []
    for i, ln in enumerate(lines[:-1]):
        if i == chrom:
            out.append(JUNCTION_OVERLAP)
        if i > chrom:
            f = ln.split("\t")
            f[7] += info_of(summaries[i - chrom - 1])
            ln = "\t".join(f)
        out.append(ln + "\n")
        if i == last_info:
            out.append(INFOS)
    return "".join(out).encode()


def render(names, refs, clens, pairs, genotype_spans=None, overflowed=False):
    """(FILE with -H, junctions, summaries of the printed ones) from the pairs; genotype_spans: span[] per contig, for FILE with -H -K"""
    found = sj.junctions([l for l, _ in pairs], clens)
    shown = None if overflowed else found
    if genotype_spans is None:
        plain = sj.render(names, refs, shown)
    else:
        from tests.support import junctiongt as jg
        plain = jg.render(names, refs, shown, genotype_spans)
    kept = [j for j in shown or [] if j[1] != 0 and j[4] != 0]
    sums = [junction_summary(pairs, clens, j) for j in kept]
    return with_overlap(plain, sums), found, sums


def render_of_bam(bam, fasta_path, q=sl.MIN_MAPQ, genotype=False, overflowed=False):
    """(FILE with -H, or with -H -K; junctions; summaries) from BAM + FASTA with the driver's constants"""
    from tests.support import cliptails as ct
    names, clens, pairs = overlaps_of_bam(bam, sl.MIN_CLIP, q)
    fasta = ct.read_fasta(fasta_path)
    refs = [fasta[n] for n in names]
    spans = None
    if genotype:
        from tests.support import junctiongt as jg
        spans = jg.spans_of_bam(bam, jg.FLANK, q)[2]
    return render(names, refs, clens, pairs, spans, overflowed)


# ---------------------------------------------------------------------- the cases worked by hand

NAMES, CLENS = sl.NAMES, sl.CLENS


def _cases():
    """[(name, keyword arguments of sl.make_record, d worked by hand or None for unknown)]: every one stores a link.  The primary record
    is on ctg1 at 1 000, a read of 100 bases unless the case says otherwise; p stands at 501 on ctg10"""
    out = []

    def add(name, d, cigar, entry, flag=0):
        out.append((name, dict(cigar=cigar, flag=flag, aux=sl.sa("ctg10,501,%s,60,0;" % entry)), d))

    # BEHIND: d = (Q1 - T1) - L2; the primary aligns read bases [0, Q1 - T1), the entry [L2, Q2)
    add("behind, same strand, clean", 0, "60M40S", "+,60S40M")
    add("behind, same strand, 5 shared", 5, "65M35S", "+,60S40M")
    add("behind, same strand, 10 between", -10, "55M45S", "+,65S35M")
    add("behind, other strand, clean", 0, "60M40S", "-,40M60S")
    add("behind, other strand, 7 shared", 7, "67M33S", "-,40M60S")
    add("behind, other strand, 3 between", -3, "57M43S", "-,40M60S")
    # FRONT: d = (Q1 - T2) - L1; the entry aligns [0, Q2 - T2), the primary [L1, Q1)
    add("front, same strand, clean", 0, "40S60M", "+,40M60S")
    add("front, same strand, 6 shared", 6, "40S60M", "+,46M54S")
    add("front, same strand, 12 between", -12, "40S60M", "+,28M72S")
    add("front, other strand, clean", 0, "40S60M", "-,60S40M")
    add("front, other strand, 4 shared", 4, "40S60M", "-,56S44M")
    add("front, other strand, 9 between", -9, "49S51M", "-,60S40M")
    add("a reverse primary: '-' is the same strand", 5, "65M35S", "-,60S40M", flag=0x10)
    add("a reverse primary: '+' is the other strand", 7, "67M33S", "+,40M60S", flag=0x10)
    # I is read bases, D is not: were D counted the first would be 10 and the third unknown, were I not they would be -5 and unknown
    add("I and D in the primary", 0, "30M5I25M10D40S", "+,60S40M")
    add("I and D in the primary, 3 shared", 3, "30M5I28M10D37S", "+,60S40M")
    add("I and D in the entry", 0, "60M40S", "+,60S20M4I16M9D")
    add("I and D in the entry, in front", 2, "40S60M", "+,20M4I18M9D58S")
    add("N and P and = and X", 1, "20=10X7N31M2P39S", "+,60S10=2P5N30X")
    # H and S: a run on the primary, the one outer operation on the entry
    add("H outside S behind the primary", 0, "60M35S5H", "+,60H40M")
    add("H outside S in front of the primary", 0, "5H35S60M", "+,40M60H")
    add("H in front of the primary's S, the entry clipped hard at both ends", 2, "5H35S60M", "+,3H39M58H")
    add("only the entry's first operation is L2", 5, "60M40S", "+,55H5S40M")
    # the swap: unequal clips on the other strand; unswapped, L2 = 10 and T2 = 60 would be neither behind nor in front
    add("clipped at both ends on the other strand", 0, "60M40S", "-,10S30M60S")
    add("clipped at both ends on the other strand, 8 between", -8, "5S47M48S", "-,10S30M60S")
    # unknown
    add("Q2 one short", None, "60M40S", "+,60S39M")
    add("Q2 one long", None, "60M40S", "+,60S40M1S")
    add("Q1 one short", None, "59M40S", "+,60S40M")
    # the ends of the 16-bit code, on I operations, which take no reference
    add("d = 32767", D_MAX, "10M32797I10M40S", "+,50S32767I40M")
    add("d = 32768", None, "10M32798I10M40S", "+,50S32768I40M")
    add("d = -32767", -D_MAX, "60M32807S", "+,32827S40M")
    add("d = -32768", None, "60M32808S", "+,32828S40M")
    return out


HAND = _cases()


# ---------------------------------------------------------------------- the data set with planted truth

CONTIG = 20_000
N_SPLIT = 10                                    # split reads per site, alternately from either end
# (what, a, b, d): a split read runs up to base a - 1 and goes on behind -- a deletion, a < b.  d > 0: the d bases in front of a are also
# the bases from b on, and the part behind the junction starts at b, on them; d < 0: -d random bases lie between the parts
PLANTED = [
    ("clean", 3_000, 4_000, 0),
    ("7 bases of homology", 7_000, 8_000, 7),
    ("40 bases of homology", 11_000, 12_000, 40),
    ("12 inserted bases", 15_000, 16_000, -12),
]
# beside the ten: at the clean site one read whose SA entry is a base short (Q1 != Q2: a link, no d); at the site of 7 one read from
# either end that its aligner split 5 bases into the homology, not 7
PLANTED_SUMMARY = [(10, 0, 10), (12, 7, 10), (10, 40, 10), (10, -12, 10)]
PLANTED_INFO = ["SE=11;SR=6,5;HOMLEN=0;INSLEN=0;OA=10,10", "SE=10;SR=6,6;HOMLEN=7;INSLEN=0;OA=10,12", "SE=10;SR=5,5;HOMLEN=40;INSLEN=0;OA=10,10",
                "SE=10;SR=5,5;HOMLEN=0;INSLEN=12;OA=10,10"]


def planted_truth():
    """(refs, rd): one contig of 20 000 random bases and, per site of PLANTED, reads of 100 bases in proper pairs whose mates lie 400
    bases away: five plain reads through either end, and split reads across the junction with the SA tag a split aligner would have
    written, alternately with the part in front of the junction and the part behind it as the primary record.  Both parts align the
    shared bases of a homology; neither aligns inserted ones.  Fewer than 200 records, no differences from the reference."""
    from indelminer_amd import synth
    rng = np.random.default_rng(78)
    acgt = np.frombuffer(b"ACGT", np.uint8)
    ref = rng.choice(acgt, CONTIG)
    for _what, a, b, d in PLANTED:
        if d > 0:
            ref[b:b + d] = ref[a - d:a]
    L = 100
    rows = []                                   # (pos, flag, cigar [(len, op)], seq, mate pos, isize, pair id, tags or None)

    def pair(pos, cigar, seq, mate_behind, tag_of=None):
        pid = len(rows) // 2
        mpos = pos + 400 if mate_behind else pos - 400
        isize = max(pos, mpos) + L - min(pos, mpos)
        fwd, rev = 0x1 | 0x2 | 0x20 | 0x40, 0x1 | 0x2 | 0x10 | 0x80
        flag = fwd if mate_behind else rev
        tags = tag_of("-" if flag & 0x10 else "+") if tag_of else None
        rows.append((pos, flag, cigar, seq, mpos, isize if mate_behind else -isize, pid, tags))
        rows.append((mpos, rev if mate_behind else fwd, [(L, synth.OP_M)], ref[mpos:mpos + L].copy(), pos, -isize if mate_behind else isize, pid, None))

    def split(a, b, d, x, i, short=0):
        """read i of a site: x bases up to a, then -d inserted ones, then the bases from b + max(d, 0) on; the front part's record
        is xM(L - x)S, the back part's (x - d)S(L - x + d)M at b; short: the entry states so many bases fewer"""
        h, k = max(d, 0), max(-d, 0)
        seq = np.concatenate([ref[a - x:a], rng.choice(acgt, k), ref[b + h:b + h + L - x - k]])
        assert len(seq) == L and x - d >= 24 and L - x >= 24
        if i % 2 == 0:
            tag = lambda strand: sl.sa("ctg0,%d,%s,%dS%dM,60,0;" % (b + 1, strand, x - d, L - x + d - short))
            pair(a - x, [(x, synth.OP_M), (L - x, synth.OP_S)], seq, mate_behind=False, tag_of=tag)
        else:
            tag = lambda strand: sl.sa("ctg0,%d,%s,%dM%dS,60,0;" % (a - x + 1, strand, x, L - x - short))
            pair(b, [(x - d, synth.OP_S), (L - x + d, synth.OP_M)], seq, mate_behind=True, tag_of=tag)

    for what, a, b, d in PLANTED:
        for end in (a, b):
            for i in range(5):
                pos = end - 70 + 9 * i
                pair(pos, [(L, synth.OP_M)], ref[pos:pos + L].copy(), mate_behind=end == b)
        for i in range(N_SPLIT):
            split(a, b, d, max(d, 0) + 24 + 3 * (i // 2), i)
        if what == "clean":
            split(a, b, d, 45, 0, short=1)
        if d == 7:
            split(a, b + 2, 5, 50, 0)
            split(a, b + 2, 5, 53, 1)

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
