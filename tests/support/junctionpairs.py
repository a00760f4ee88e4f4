"""What tests/test_gpu_junction_pairs.py and tests/test_junction_pairs_host.py share: the plain restatement of the junction pairs (-E),
written from the rule in include/indelminer_amd.h (seam 5, "Junction pairs"), not from the code under test; the restatement of -J's FILE
with -E, layered on tests/support/splitjunctions.py's (with -K on junctiongt.py's, with -H on splitoverlap.py's); cases worked by hand;
and the planted data sets.

A record is anything with tid, pos, mapq, flag, mtid, mpos (tests/support/pairlinks.py's Rec).  A PAIR LINK is (tid, kind, pos, mpos),
kind 0 .. 2 as in tests/support/pairlinks.py and 3 STRETCHED; a MATE LINK is (tid, kind, pos, mtid, mpos) as in
tests/support/intercontig.py.  A JUNCTION is (t1, p1, s1, t2, p2, s2, ...).  Everything is an integer and every comparison is exact.
"""
import numpy as np

from tests.support import intercontig as ic
from tests.support import pairlinks as pk
from tests.support import splitjunctions as sj
from tests.support import splitlinks as sl
from tests.support.pairlinks import Rec

STRETCHED = 3
REACH, BACK, MIN_SEP = 1_000, 32, 50            # what the host driver uses: LINK_EV_WINDOW, CLIPTAIL_MAX_SHIFT, LINK_EV_MIN_SEP
NONE = 0xFFFFFFFF
KIND = {(1, 0): 0, (0, 0): 1, (1, 1): 2, (0, 1): 3}     # K(s_lo, s_hi)


# ---------------------------------------------------------------------- the two rules

def pair_link_of(rec, clens, q, stretched=True):
    """(tid, kind, pos, mpos) of one record, or None: the pair links' rule, and with the switch on its fourth kind"""
    f = rec.flag
    if not f & 0x1 or f & pk.EXCLUDED:
        return None
    if not 0 <= rec.tid < len(clens) or rec.mtid != rec.tid:
        return None
    if not (rec.pos < rec.mpos or (rec.pos == rec.mpos and f & 0x40)):
        return None
    if rec.mapq < q:
        return None
    if not (0 <= rec.pos <= clens[rec.tid] and 0 <= rec.mpos <= clens[rec.tid]):
        return None
    kind = {(1, 0): 0, (0, 0): 1, (1, 1): 2, (0, 1): STRETCHED}[((f >> 4) & 1, (f >> 5) & 1)]
    if kind == STRETCHED and (not stretched or f & 0x2):
        return None
    return rec.tid, kind, rec.pos, rec.mpos


def pair_links_of(records, clens, q, stretched=True):
    return [x for x in (pair_link_of(r, clens, q, stretched) for r in records) if x is not None]


def window(p, s, clen, reach=REACH, back=BACK):
    """W(p, s) clipped to [0, clen], or None when nothing is left of it"""
    w0, w1 = (p - back, p + reach) if s else (p - reach, p + back)
    w0, w1 = max(w0, 0), min(w1, clen)
    return None if w0 > w1 else (w0, w1)


def junction_pairs(pair_links, mate_links, clens, junction, reach=REACH, back=BACK, min_sep=MIN_SEP):
    """(pe1, pe2) of one junction"""
    t1, p1, s1, t2, p2, s2 = junction[:6]
    if t1 == t2:
        (plo, slo), (phi, shi) = ((p1, s1), (p2, s2)) if p1 <= p2 else ((p2, s2), (p1, s1))
        a, b = window(plo, slo, clens[t1], reach, back), window(phi, shi, clens[t1], reach, back)
        if a is None or b is None:
            return 0, 0
        kind = KIND[(slo, shi)]
        return sum(1 for t, k, p, m in pair_links if t == t1 and k == kind and a[0] <= p <= a[1] and b[0] <= m <= b[1] and m - p >= min_sep), 0
    a, b = window(p1, s1, clens[t1], reach, back), window(p2, s2, clens[t2], reach, back)
    if a is None or b is None:
        return 0, 0
    pe1 = sum(1 for t, k, p, mt, m in mate_links if t == t1 and k == (s1 | s2 << 1) and a[0] <= p <= a[1] and mt == t2 and b[0] <= m <= b[1])
    pe2 = sum(1 for t, k, p, mt, m in mate_links if t == t2 and k == (s2 | s1 << 1) and b[0] <= p <= b[1] and mt == t1 and a[0] <= m <= a[1])
    return pe1, pe2


def answers(pair_links, mate_links, clens, junctions, reach=REACH, back=BACK, min_sep=MIN_SEP, pair_over=False, mate_over=False):
    """what im_junction_pairs answers: a junction whose table has overflowed is NONE twice"""
    out = []
    for j in junctions:
        over = pair_over if j[0] == j[3] else mate_over
        out.append((NONE, NONE) if over else junction_pairs(pair_links, mate_links, clens, j, reach, back, min_sep))
    return out


def answers_fast(pair_links, mate_links, clens, junctions, reach=REACH, back=BACK, min_sep=MIN_SEP):
    """the same answers for the soak: the links in dictionaries by (contig, kind), nothing else changed"""
    pairs, mates = {}, {}
    for l in pair_links:
        pairs.setdefault(l[:2], []).append(l)
    for l in mate_links:
        mates.setdefault(l[:2], []).append(l)
    out = []
    for j in junctions:
        t1, p1, s1, t2, p2, s2 = j[:6]
        if t1 == t2:
            (plo, slo), (phi, shi) = ((p1, s1), (p2, s2)) if p1 <= p2 else ((p2, s2), (p1, s1))
            out.append(junction_pairs(pairs.get((t1, KIND[(slo, shi)]), []), [], clens, j, reach, back, min_sep))
        else:
            out.append(junction_pairs([], mates.get((t1, s1 | s2 << 1), []) + mates.get((t2, s2 | s1 << 1), []), clens, j, reach, back, min_sep))
    return out


def links_of_bam(bam, q, stretched=True):
    """(contig names, contig lengths, pair links, mate links) of a BAM file"""
    from tests.support import bamlite
    _, refs, recs = bamlite.read_bam(bam)
    clens = [n for _, n in refs]
    return [n for n, _ in refs], clens, pair_links_of(recs, clens, q, stretched), ic.links_of(recs, clens, q)


# ---------------------------------------------------------------------- FILE with -E

PE_INFO = ("##INFO=<ID=PE,Number=.,Type=Integer,Description=\"Read pairs across the junction: on one contig the pairs of the junction's orientation with "
           "one read at either end; on two contigs the pairs counted from the first end and from the second\">\n")
JUNCTION_PAIRS = (
    "##junctionPairs=\"every junction against the read pairs on either side of it, which come from other molecules than the split reads of SE and SR: "
    "a record counts when it is paired, mapped with a mapped mate, primary, no duplicate and no failure, at or above -q (its mate's quality is not "
    "known); an end with CT 3 is supported by forward reads that start from 1000 bases in front of it to 32 behind, an end with CT 5 by reverse reads "
    "that start from 32 in front of it to 1000 behind; on one contig PE=n counts the pairs whose leftmost read supports the end with the smaller position "
    "(POS on a tie) and whose mate supports the other, their starts at least 50 bases apart: JT=DUP reverse then forward, JT=INV both forward (3to3) "
    "or both reverse (5to5), and JT=DEL forward then reverse, the normal orientation, only when the aligner has NOT flagged the pair a proper pair "
    "(flag 0x2 clear) -- its verdict stands in for an insert-size test, so a deletion shorter than the spread of the library's insert size leaves "
    "proper pairs and PE=0 is expected there; on two contigs PE=n1,n2 counts the pairs with a read that supports the first end and its mate "
    "supporting the second, at the record of the first end's read and at that of the second end's; PE=. or PE=.,. once that table has "
    "overflowed (stderr says so); a duplication or an inversion shorter than a read leaves no such pair; nothing is filtered by PE, and the "
    "ALT of ##junctionGenotype stays the split reads alone; the records of -U, -N and -T are not touched\"\n")


def info_of(junction, pe):
    """what -E appends to a record's INFO"""
    if junction[0] == junction[3]:
        return ";PE=." if pe[0] == NONE else ";PE=%d" % pe[0]
    return ";PE=.,." if pe[0] == NONE else ";PE=%d,%d" % pe


def with_pairs(text, kept, pes):
    """a FILE of -J (with or without -K and -H) as it is written with -E: the ##INFO line behind the present ones, the ##junctionPairs line
    as the last description line, and PE at the very end of INFO of every record, in order"""
    lines = text.decode().split("\n")
    assert lines[-1] == ""
    last_info = max(i for i, ln in enumerate(lines) if ln.startswith("##INFO"))
    chrom = next(i for i, ln in enumerate(lines) if ln.startswith("#CHROM"))
    assert len(lines) - 1 - (chrom + 1) == len(kept) == len(pes)
    out = []
    for i, ln in enumerate(lines[:-1]):
        if i == chrom:
            out.append(JUNCTION_PAIRS)
        if i > chrom:
            f = ln.split("\t")
            f[7] += info_of(kept[i - chrom - 1], pes[i - chrom - 1])
            ln = "\t".join(f)
        out.append(ln + "\n")
        if i == last_info:
            out.append(PE_INFO)
    return "".join(out).encode()


def render_of_bam(bam, fasta_path, q=sl.MIN_MAPQ, genotype=False, overlap=False, pair_over=False, mate_over=False):
    """(FILE with -E -- and -K, -H --, FILE without -E, junctions printed, their (pe1, pe2)) from BAM + FASTA with the driver's constants"""
    if overlap:
        from tests.support import splitoverlap as so
        plain, found = so.render_of_bam(bam, fasta_path, q, genotype=genotype)[:2]
    elif genotype:
        from tests.support import junctiongt as jg
        plain, found = jg.render_of_bam(bam, fasta_path, q)[:2]
    else:
        plain, found = sj.render_of_bam(bam, fasta_path, q)
    names, clens, pairs, mates = links_of_bam(bam, q)
    kept = [j for j in found if j[1] != 0 and j[4] != 0]
    pes = answers(pairs, mates, clens, kept, pair_over=pair_over, mate_over=mate_over)
    return with_pairs(plain, kept, pes), plain, kept, pes


# ---------------------------------------------------------------------- the cases worked by hand

HAND_CLENS = [100_000, 50_000, 3_000]
PAIRED, PROPER, REV, MREV, FIRST, SECOND = 0x1, 0x2, 0x10, 0x20, 0x40, 0x80
FLAGS = {0: PAIRED | REV | FIRST, 1: PAIRED | FIRST, 2: PAIRED | REV | MREV | FIRST, 3: PAIRED | MREV | FIRST}     # a leftmost record of each kind


def _pair(kind, pos, mpos, tid=0, mapq=60, extra=0):
    return Rec(tid, pos, mapq, FLAGS[kind] | extra, tid, mpos)


def _mates(t1, a, r1, t2, b, r2):
    """the two records of a pair on two contigs: one read at a on t1 (reverse iff r1), its mate at b on t2 (reverse iff r2)"""
    return [Rec(t1, a, 60, PAIRED | FIRST | (REV if r1 else 0) | (MREV if r2 else 0), t2, b),
            Rec(t2, b, 60, PAIRED | SECOND | (REV if r2 else 0) | (MREV if r1 else 0), t1, a)]


def _hand():
    """[(name, records, junction, (pe1, pe2) worked by hand)] at reach 1 000, back 32, min_sep 50, -q 10"""
    out = []
    add = lambda name, recs, j, want: out.append((name, recs, j, want))
    # the header's worked examples: one pair in the middle of both windows
    add("DEL: forward then reverse, not proper", [_pair(3, 4_500, 5_900)], (0, 5_000, 0, 0, 5_400, 1), (1, 0))
    add("DEL: the same pair flagged proper", [_pair(3, 4_500, 5_900, extra=PROPER)], (0, 5_000, 0, 0, 5_400, 1), (0, 0))
    add("DUP: reverse then forward", [_pair(0, 5_100, 5_300)], (0, 5_000, 1, 0, 5_400, 0), (1, 0))
    add("INV 3to3: both forward", [_pair(1, 4_500, 8_500)], (0, 5_000, 0, 0, 9_000, 0), (1, 0))
    add("INV 5to5: both reverse", [_pair(2, 5_500, 9_500)], (0, 5_000, 1, 0, 9_000, 1), (1, 0))
    every = [_pair(k, 4_990, 5_410) for k in range(4)]                  # inside all four classes' windows at once
    for k, (s1, s2) in enumerate(((1, 0), (0, 0), (1, 1), (0, 1))):
        add("one pair of every kind: sides %d, %d count kind %d alone" % (s1, s2, k), every + [every[k]], (0, 5_000, s1, 0, 5_400, s2), (2, 0))
    # two contigs: the four side classes; a pair is counted from either end by the record that lies there
    for s1 in (0, 1):
        for s2 in (0, 1):
            p1, p2 = 5_000 + (500 if s1 else -500), 7_000 + (500 if s2 else -500)
            recs = _mates(0, p1, s1, 1, p2, s2) + _mates(0, p1, s1, 1, p2, s2)[:1] + _mates(0, p1, 1 - s1, 1, p2, s2) + _mates(0, p1, s1, 2, 2_000, s2)
            add("TRA: sides %d, %d" % (s1, s2), recs, (0, 5_000, s1, 1, 7_000, s2), (2, 1))
    add("TRA from the other end: the columns change places", _mates(0, 4_500, 0, 1, 7_500, 1) + _mates(0, 4_600, 0, 1, 7_500, 1)[:1], (1, 7_000, 1, 0, 5_000, 0), (1, 2))
    # pos1 > pos2, and the tie
    add("pos1 > pos2: lo is end 2", [_pair(3, 4_500, 5_900)], (0, 5_400, 1, 0, 5_000, 0), (1, 0))
    add("pos1 > pos2 with the sides of a duplication", [_pair(0, 5_100, 5_300), _pair(3, 4_500, 5_900)], (0, 5_400, 0, 0, 5_000, 1), (1, 0))
    add("a tie: end 1 is lo, kind K(0, 1)", [_pair(3, 4_500, 5_500), _pair(0, 5_500, 4_500 + 1_100)], (0, 5_000, 0, 0, 5_000, 1), (1, 0))
    add("a tie the other way round: kind K(1, 0)", [_pair(0, 5_500, 5_600), _pair(3, 4_500, 5_500)], (0, 5_000, 1, 0, 5_000, 0), (0, 0))
    add("a tie the other way round, a pair that fits", [_pair(0, 4_970, 5_030)], (0, 5_000, 1, 0, 5_000, 0), (1, 0))
    # the windows' edges
    J = (0, 20_000, 0, 0, 30_000, 1)                                     # W(lo) = [19 000, 20 032], W(hi) = [29 968, 31 000]
    add("lo: reach and reach + 1 in front", [_pair(3, 19_000, 30_500), _pair(3, 18_999, 30_500)], J, (1, 0))
    add("lo: back and back + 1 behind", [_pair(3, 20_032, 30_500), _pair(3, 20_033, 30_500)], J, (1, 0))
    add("hi: back and back + 1 in front", [_pair(3, 19_500, 29_968), _pair(3, 19_500, 29_967)], J, (1, 0))
    add("hi: reach and reach + 1 behind", [_pair(3, 19_500, 31_000), _pair(3, 19_500, 31_001)], J, (1, 0))
    T = (0, 20_000, 1, 1, 30_000, 0)                                     # W(1) = [19 968, 21 000], W(2) = [29 000, 30 032]
    edges = [(19_968, 29_000), (21_000, 30_032), (19_967, 29_500), (21_001, 29_500), (20_500, 28_999), (20_500, 30_033)]
    add("TRA: every edge of both windows and one base outside each", sum((_mates(0, a, 1, 1, b, 0) for a, b in edges), []), T, (2, 2))
    # min_sep on a 50-base deletion whose windows overlap
    add("mpos - pos of 49 and of 50", [_pair(3, 7_000, 7_049), _pair(3, 7_000, 7_050), _pair(3, 7_001, 7_050)], (0, 7_000, 0, 0, 7_050, 1), (1, 0))
    # ends at 0 and at the contig's length: the clip
    add("an end at 0", [_pair(3, 0, 600), _pair(3, 32, 600)], (0, 0, 0, 0, 500, 1), (2, 0))
    add("an end at the contig's length", [_pair(3, 2_400, 3_000, tid=2), _pair(3, 2_400, 2_968, tid=2)], (2, 2_400, 0, 2, 3_000, 1), (2, 0))
    add("TRA: ends at 0 and at the contig's length", _mates(0, 0, 1, 2, 3_000, 0) + _mates(0, 1_000, 1, 2, 2_000, 0), (0, 0, 1, 2, 3_000, 0), (2, 2))
    add("a window that is empty after the clip", [_pair(3, 2_900, 3_000, tid=2)], (2, 2_000, 0, 2, 3_033, 1), (0, 0))
    add("TRA: a window that is empty after the clip", _mates(0, 100, 0, 2, 3_000, 1), (0, -33, 0, 2, 3_000, 1), (0, 0))
    # bucket edges
    add("pos 255 and 256, mpos 511 and 512", [_pair(3, 255, 511), _pair(3, 256, 512), _pair(3, 255, 512)], (0, 256, 0, 0, 512, 1), (3, 0))
    add("TRA: pos 255 and 256 at either end", _mates(0, 255, 0, 1, 256, 1) + _mates(0, 256, 0, 1, 255, 1), (0, 260, 0, 1, 250, 1), (2, 2))
    # pos == mpos
    same = (0, 9_000, 0, 0, 9_000, 1)
    add("pos == mpos with 0x40: a link, min_sep 50 drops it", [Rec(0, 9_000, 60, PAIRED | MREV | FIRST, 0, 9_000)], same, (0, 0))
    add("pos == mpos without 0x40: no link", [Rec(0, 9_000, 60, PAIRED | MREV | SECOND, 0, 9_000)], same, (0, 0))
    # the front of the rule
    D = (0, 40_000, 0, 0, 40_400, 1)
    front = [_pair(3, 39_500, 40_900, mapq=9), _pair(3, 39_500, 40_900, mapq=10)] + [_pair(3, 39_500, 40_900, extra=b) for b in (0x4, 0x8, 0x100, 0x200, 0x400, 0x800)]
    front += [Rec(0, 39_500, 60, MREV | FIRST, 0, 40_900), Rec(0, 40_900, 60, PAIRED | REV | SECOND, 0, 39_500), Rec(0, 39_500, 60, PAIRED | MREV | FIRST, 1, 40_900)]
    add("mapq q - 1 and q, the six excluded bits, not paired, the rightmost record, a mate elsewhere", front, D, (1, 0))
    return out


HAND = _hand()
# the same records and junctions with min_sep 0, for the two pos == mpos cases: what the link alone answers
HAND_NO_SEP = {"pos == mpos with 0x40: a link, min_sep 50 drops it": (1, 0), "pos == mpos without 0x40: no link": (0, 0)}


# ---------------------------------------------------------------------- the planted data sets

def planted(kind, overflow=False):
    """(module, refs, rd) of the planted data set of -U ("DUP"), -N ("INV") or -T ("BND") with the pairs that -M's and -T's tests plant at
    its junctions and the SA tags that -J's tests plant (tests/support/splitlinks.py's planted(), on the reads with the pairs);
    overflow ("DUP", "BND"): the set of -M's or -T's overflow test instead, whose 2 100 more links its table of a small BAM cannot keep"""
    from tests.support import crossedpiles, invertedpiles
    if kind == "DUP":
        mod, (refs, rd) = crossedpiles, pk.planted_overflow_reads() if overflow else pk.planted_dup_reads()[:2]
    elif kind == "INV":
        mod, (refs, rd) = invertedpiles, pk.planted_inv_reads()[:2]
    else:
        mod, (refs, rd) = ic, ic.planted_overflow_reads() if overflow else ic.planted_reads()
    names = ["ctg%d" % t for t in range(len(refs))]
    ends = []
    if kind == "DUP":
        for pl, n in mod.SITES:
            ends += [((0, pl, 1), (0, pl + n, 0), 0), ((0, pl + n, 0), (0, pl, 1), 0)]
        decoys = ends[12:14]
    elif kind == "INV":
        for a, n in mod.SITES:
            for x, y in ((a, a + n), (a + n, a)):
                ends += [((0, x, 0), (0, y, 0), 0), ((0, x, 1), (0, y, 1), 0)]
        decoys = ends[24:28]
    else:
        for ta, pa, sa_, tb, pb, sb, h in mod.SITES:
            ends += [((ta, pa, sa_), (tb, pb, sb), h), ((tb, pb, sb), (ta, pa, sa_), h)]
        decoys = ends[2:4] + ends[10:12]
    keep = dict(getattr(rd, "overrides", None) or {})
    sl.plant_tags(rd, names, ends, decoys)
    for i, o in keep.items():                                           # mtid and mapq of -T's pairs stay beside the tags
        rd.overrides[i] = dict(o, **{k: v for k, v in rd.overrides.get(i, {}).items() if k not in o})
    return mod, refs, rd


DEL_CLENS = [20_000, 5_000]
DEL_A, DEL_B = 8_000, 8_400                     # a 400-base deletion: W(lo) = [7 000, 8 032], W(hi) = [8 368, 9 400]
DEL_JUNCTION = (0, DEL_A, 0, 0, DEL_B, 1)
DEL_N_SPLIT = 10
DEL_COUNTED = [(7_000, 8_368), (8_032, 9_400), (7_500, 8_900), (7_900, 8_368), (7_000, 9_400), (7_700, 8_600)]     # on all four edges, and inside
DEL_PE = 6
DEL_DECOYS = [                                  # (what, pos, mpos)
    ("proper", 7_600, 8_700), ("one base in front of lo", 6_999, 8_500), ("one base behind lo", 8_033, 8_500), ("one base in front of hi", 7_500, 8_367),
    ("one base behind hi", 7_500, 9_401), ("mapq q - 1", 7_550, 8_750), ("duplicate", 7_650, 8_650), ("mate on another contig", 7_450, 1_000)]


def planted_deletion():
    """(refs, rd): two contigs of random bases; on the first a 400-base deletion with ten split reads across it that carry the SA tag a
    split aligner would have written, alternately from either end, in proper pairs of their own; the six pairs of DEL_COUNTED in the
    normal orientation without the proper-pair flag, their starts on the four window edges and inside; and the decoys of DEL_DECOYS,
    none of which counts.  Reads of 100 bases, no differences from the reference."""
    from indelminer_amd import synth
    rng = np.random.default_rng(404)
    acgt = np.frombuffer(b"ACGT", np.uint8)
    refs = [rng.choice(acgt, n) for n in DEL_CLENS]
    ref, L, q = refs[0], 100, sl.MIN_MAPQ
    rows = []                                   # (tid, pos, flag, cigar, seq, mpos, isize, pair id, overrides or None)
    fwd, rev = PAIRED | MREV | FIRST, PAIRED | REV | SECOND

    def pair(pos, mpos, extra=0, ov_first=None, ov_second=None, mtid=0):
        pid = len(rows) // 2
        isize = mpos + L - pos if mtid == 0 else 0
        rows.append((0, pos, fwd | extra, [(L, synth.OP_M)], ref[pos:pos + L].copy(), mpos, isize, pid, ov_first))
        rows.append((mtid, mpos, rev | extra, [(L, synth.OP_M)], refs[mtid][mpos:mpos + L].copy(), pos, -isize, pid, ov_second))

    def split(x, i):
        """read i: x bases up to DEL_A, then the bases from DEL_B on; in a proper pair whose mate lies 400 bases away"""
        seq = np.concatenate([ref[DEL_A - x:DEL_A], ref[DEL_B:DEL_B + L - x]])
        pid = len(rows) // 2
        if i % 2 == 0:
            pos, mpos, flag, mflag = DEL_A - x, DEL_A - x - 400, PAIRED | PROPER | REV | SECOND, PAIRED | PROPER | MREV | FIRST
            cigar, tag = [(x, synth.OP_M), (L - x, synth.OP_S)], sl.sa("ctg0,%d,-,%dS%dM,60,0;" % (DEL_B + 1, x, L - x))
        else:
            pos, mpos, flag, mflag = DEL_B, DEL_B + 400, PAIRED | PROPER | MREV | FIRST, PAIRED | PROPER | REV | SECOND
            cigar, tag = [(x, synth.OP_S), (L - x, synth.OP_M)], sl.sa("ctg0,%d,+,%dM%dS,60,0;" % (DEL_A - x + 1, x, L - x))
        isize = abs(mpos - pos) + L
        rows.append((0, pos, flag, cigar, seq, mpos, isize if pos < mpos else -isize, pid, {"tags": b"MQC" + bytes([60]) + tag}))
        rows.append((0, mpos, mflag, [(L, synth.OP_M)], ref[mpos:mpos + L].copy(), pos, -isize if pos < mpos else isize, pid, None))

    for i in range(DEL_N_SPLIT):
        split(30 + 4 * (i // 2), i)
    for pos, mpos in DEL_COUNTED:
        pair(pos, mpos)
    for what, pos, mpos in DEL_DECOYS:
        if what == "proper":
            pair(pos, mpos, extra=PROPER)
        elif what == "mapq q - 1":
            pair(pos, mpos, ov_first={"mapq": q - 1})
        elif what == "duplicate":
            pair(pos, mpos, extra=0x400)
        elif what == "mate on another contig":
            pair(pos, mpos, ov_first={"mtid": 1}, ov_second={"mtid": 0}, mtid=1)
        else:
            pair(pos, mpos)
    order = sorted(range(len(rows)), key=lambda k: (rows[k][0], rows[k][1]))        # stable
    rd = synth.Reads()
    rd.n, rd.read_len, rd.mapq, rd.range_max = len(rows), L, 60, 700
    rd.tid = np.array([rows[k][0] for k in order], np.int64)
    rd.pos = np.array([rows[k][1] for k in order]); rd.flag = np.array([rows[k][2] for k in order])
    rd.mpos = np.array([rows[k][5] for k in order]); rd.isize = np.array([rows[k][6] for k in order]); rd.pair_id = np.array([rows[k][7] for k in order])
    rd.mate_first = (rd.flag & 0x40) != 0
    rd.ncig = np.array([len(rows[k][3]) for k in order])
    rd.cig_len = np.zeros((rd.n, 2), np.int64); rd.cig_op = np.zeros((rd.n, 2), np.int64)
    rd.seq = np.zeros((rd.n, L), np.uint8)
    rd.overrides = {}
    for i, k in enumerate(order):
        for j, (ln, op) in enumerate(rows[k][3]):
            rd.cig_len[i, j], rd.cig_op[i, j] = ln, op
        rd.seq[i] = rows[k][4]
        if rows[k][8] is not None:
            rd.overrides[i] = rows[k][8]
    return refs, rd


def write_planted(d, refs, rd):
    """ref.fa, aln.bam (+ .bai) and cfg.txt in directory d"""
    return ic.write_planted(d, refs, rd)


# ---------------------------------------------------------------------- records through a BAM file

def write_recs_bam(path, recs, clens):
    """[Rec] (contigs of the reference, positions from 0 on) as a BAM file written by bamwrite.write_bam: 100M each, the mate's contig
    and the mapping quality through its per-record overrides"""
    from indelminer_amd import bamwrite, synth
    rd = synth.Reads()
    n = len(recs)
    rd.n, rd.read_len, rd.mapq = n, 100, 60
    rd.tid = np.array([r.tid for r in recs]); rd.pos = np.array([r.pos for r in recs]); rd.flag = np.array([r.flag for r in recs])
    rd.mpos = np.array([r.mpos for r in recs]); rd.isize = np.zeros(n, np.int64); rd.pair_id = np.arange(n)
    rd.ncig = np.ones(n, np.int64); rd.cig_len = np.full((n, 1), 100); rd.cig_op = np.zeros((n, 1), np.int64)
    rd.seq = np.full((n, 100), ord("A"), np.uint8)
    rd.overrides = {i: {"mtid": r.mtid, "mapq": r.mapq} for i, r in enumerate(recs)}
    bamwrite.write_bam(path, [("c%d" % t, n) for t, n in enumerate(clens)], rd)


def hand_records():
    """every record of HAND once, and which of them a BAM file can hold"""
    recs = [r for _, rs, _, _ in HAND for r in rs]
    return recs, [r for r in recs if 0 <= r.tid < len(HAND_CLENS) and r.pos >= 0 and -1 <= r.mtid < len(HAND_CLENS)]
