"""What tests/test_gpu_splitjunction.py and tests/test_splitjunction_host.py share: the plain restatement of the split junctions (-J),
written from the rule in include/indelminer_amd.h (seam 5, "Split junctions"), not from the kernels, and the restatement of -J's FILE.
tests/test_splitjunction_host.py pins both to cases worked by hand (no GPU needed).

A LINK is (tA, pA, sA, tB, pB, sB), as in tests/support/splitlinks.py, whose count() is the window count the rule names.  A JUNCTION is
(t1, p1, s1, t2, p2, s2, E, n1, n2).  Everything is quadratic in the distinct end pairs of one (t1, s1, t2, s2): plain, not fast.
"""
from collections import Counter

from tests.support import splitlinks as sl

WINDOW, MIN_SPAN, MIN_LINKS = 32, 50, 3         # the driver's: SPLIT_EV_WINDOW, JUNC_EV_MIN_SPAN, JUNC_EV_MIN_LINKS
CT = {(0, 0): "3to3", (0, 1): "3to5", (1, 0): "5to3", (1, 1): "5to5"}


def rev(l):
    return l[3:6] + l[0:3]


def can(l):
    return l if l[0:3] <= l[3:6] else rev(l)


def is_candidate(l, min_span):
    return l[0] != l[3] or abs(l[1] - l[4]) >= min_span


def junctions(links, clens, window=WINDOW, min_links=MIN_LINKS, min_span=MIN_SPAN):
    """the answer of the rule, in its order"""
    links = [tuple(int(v) for v in l) for l in links]
    stored = Counter(links)
    cands = sorted({can(l) for l in links if is_candidate(l, min_span)})
    E = {c: stored[c] + (stored[rev(c)] if rev(c) != c else 0) for c in cands}

    def near(c, d):
        return (c[0], c[2], c[3], c[5]) == (d[0], d[2], d[3], d[5]) and abs(c[1] - d[1]) <= window and abs(c[4] - d[4]) <= window

    def beats(d, c):
        return (-E[d], d[1], d[4]) < (-E[c], c[1], c[4])

    out = []
    for c in cands:
        if any(near(c, d) and beats(d, c) for d in cands):
            continue
        t1, p1, s1, t2, p2, s2 = c
        n1 = sl.count(links, clens, (t1, s1, p1 - window, p1 + window, t2, s2, p2 - window, p2 + window))
        n2 = sl.count(links, clens, (t2, s2, p2 - window, p2 + window, t1, s1, p1 - window, p1 + window))
        if n1 + n2 >= min_links:
            out.append(c + (E[c], n1, n2))
    return sorted(out, key=lambda j: (j[0], j[1], j[3], j[4], j[2], j[5]))


def junctions_fast(links, clens, window=WINDOW, min_links=MIN_LINKS, min_span=MIN_SPAN):
    """the same answer for the soak: the candidates and the links in a dictionary by (contigs, sides), nothing else changed"""
    links = [tuple(int(v) for v in l) for l in links]
    stored = Counter(links)
    groups, by_kind = {}, {}
    for c in {can(l) for l in links if is_candidate(l, min_span)}:
        groups.setdefault((c[0], c[2], c[3], c[5]), []).append(c)
    for l, n in stored.items():
        by_kind.setdefault((l[0], l[2], l[3], l[5]), []).append((l, n))
    E = {c: stored[c] + (stored[rev(c)] if rev(c) != c else 0) for g in groups.values() for c in g}

    def window_count(t1, s1, p1, t2, s2, p2):
        a0, a1, b0, b1 = max(p1 - window, 0), min(p1 + window, clens[t1]), max(p2 - window, 0), min(p2 + window, clens[t2])
        return sum(n for l, n in by_kind.get((t1, s1, t2, s2), []) if a0 <= l[1] <= a1 and b0 <= l[4] <= b1)

    out = []
    for g in groups.values():
        for c in g:
            if any(abs(c[1] - d[1]) <= window and abs(c[4] - d[4]) <= window and (-E[d], d[1], d[4]) < (-E[c], c[1], c[4]) for d in g):
                continue
            t1, p1, s1, t2, p2, s2 = c
            n1, n2 = window_count(t1, s1, p1, t2, s2, p2), window_count(t2, s2, p2, t1, s1, p1)
            if n1 + n2 >= min_links:
                out.append(c + (E[c], n1, n2))
    return sorted(out, key=lambda j: (j[0], j[1], j[3], j[4], j[2], j[5]))


# ---------------------------------------------------------------------- FILE

HEADER = (
    "##fileformat=VCFv4.1\n"
    "##INFO=<ID=SVTYPE,Number=1,Type=String,Description=\"Type of structural variant: BND, one junction between two ends\">\n"
    "##INFO=<ID=CHR2,Number=1,Type=String,Description=\"Contig of the second end\">\n"
    "##INFO=<ID=POS2,Number=1,Type=Integer,Description=\"Position of the second end\">\n"
    "##INFO=<ID=CT,Number=1,Type=String,Description=\"Which side of either end the junction joins: 3 = the reads there are clipped on their right, 5 = on their left\">\n"
    "##INFO=<ID=JT,Number=1,Type=String,Description=\"What a junction of this CT on these contigs is read as: TRA on two contigs; on one, DEL for 3to5, DUP for 5to3, "
    "INV for 3to3 and 5to5\">\n"
    "##INFO=<ID=SVLEN,Number=1,Type=Integer,Description=\"POS2 - POS, on one contig only\">\n"
    "##INFO=<ID=SE,Number=1,Type=Integer,Description=\"Split reads that name exactly these two ends, from either\">\n"
    "##INFO=<ID=SR,Number=2,Type=Integer,Description=\"Split reads whose primary part ends within 32 bases of the first end and whose SA tag "
    "places the clipped part within 32 bases of the second, and the same from the second to the first\">\n"
    "##splitJunctions=\"junctions from split reads alone: a split read is a primary record at or above -q whose soft clip at either end has 20 bases "
    "or more and whose SA tag holds exactly one entry, itself at or above -q, that continues the read; it names two ends (contig, position, side); "
    "an end pair on two contigs, or on one contig 50 bases or more apart, is a candidate, its read count SE the reads that name exactly its two ends from "
    "either; a candidate is kept when no candidate of the same contigs and sides within 32 bases at both ends has a larger SE, or the same SE and a "
    "smaller POS, then a smaller POS2 (a candidate that loses stays lost when its winner loses to a third); SR counts every split read between the "
    "windows of 32 bases around the two ends, from the first and from the second; a kept candidate needs SR of 3 in sum; no clip pile and no "
    "comparison with the reference is needed, so a junction with inserted bases, with micro-homology above 32 bases or with reads clipped at "
    "scattered positions is reported; nothing is merged with or filtered against the records of -U, -N and -T; no genotype; a tag with several "
    "entries stores nothing; the file has no records once the split-link table has overflowed (stderr says so); POS 0 and POS2 0 are skipped\"\n"
    "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\n")


def jt_of(t1, s1, t2, s2):
    if t1 != t2:
        return "TRA"
    return {(0, 1): "DEL", (1, 0): "DUP"}.get((s1, s2), "INV")


def render(names, refs, found):
    """FILE as the driver writes it from the junctions of the rule (none: after an overflow)"""
    lines = [HEADER]
    for t1, p1, s1, t2, p2, s2, e, n1, n2 in found or []:
        if p1 == 0 or p2 == 0:
            continue
        ref, there = chr(refs[t1][p1 - 1]).upper(), "%s:%d" % (names[t2], p2)
        alt = {(0, 1): "%s[%s[", (1, 0): "]%s]%s", (0, 0): "%s]%s]", (1, 1): "[%s[%s"}[(s1, s2)] % ((ref, there) if s1 == 0 else (there, ref))
        info = "SVTYPE=BND;CHR2=%s;POS2=%d;CT=%s;JT=%s" % (names[t2], p2, CT[(s1, s2)], jt_of(t1, s1, t2, s2))
        if t1 == t2:
            info += ";SVLEN=%d" % (p2 - p1)
        lines.append("%s\t%d\t.\t%s\t%s\t.\t.\t%s;SE=%d;SR=%d,%d\n" % (names[t1], p1, ref, alt, info, e, n1, n2))
    return "".join(lines).encode()


def render_of_bam(bam, fasta_path, q, overflowed=False):
    """(FILE, junctions) from BAM + FASTA at -q q with the driver's constants"""
    from tests.support import cliptails as ct
    names, clens, links = sl.links_of_bam(bam, sl.MIN_CLIP, q)
    fasta = ct.read_fasta(fasta_path)
    refs = [fasta[n] for n in names]
    found = junctions(links, clens)
    return render(names, refs, None if overflowed else found), found


# ---------------------------------------------------------------------- the data set no pile search reports

def planted_insertion():
    """(module, refs, rd, names, site): the planted data set of -T, and at the one site of it whose clipped reads carry RANDOM bases
    (intercontig.RANDOM_TAILS: an insertion at the junction, which -T's comparison with the reference refuses by construction) the SA
    tags a split aligner would have written, from either end"""
    from tests.support import intercontig as ic
    refs, rd = ic.planted_reads()
    names = ["ctg%d" % t for t in range(len(refs))]
    ta, pa, sa, tb, pb, sb, h = ic.RANDOM_TAILS
    import numpy as np
    from indelminer_amd import synth
    rd.overrides = dict(rd.overrides)
    for (t, p, s), (to, po, so) in (((ta, pa, sa), (tb, pb, sb)), ((tb, pb, sb), (ta, pa, sa))):
        two = rd.ncig == 2
        if s == 0:
            hit = two & (rd.cig_op[:, 0] == synth.OP_M) & (rd.cig_op[:, 1] == synth.OP_S) & (rd.pos + rd.cig_len[:, 0] == p)
        else:
            hit = two & (rd.cig_op[:, 0] == synth.OP_S) & (rd.cig_op[:, 1] == synth.OP_M) & (rd.pos == p)
        reads = [int(i) for i in np.nonzero(hit & (rd.tid == t) & ((rd.flag & 0x4) == 0))[0]]
        assert len(reads) >= 3
        for i in reads:
            value, pb_named = sl.sa_value(rd.read_len, s, int(rd.cig_len[i, 0]), bool(int(rd.flag[i]) & 0x10), names[to], po, so, h)
            assert pb_named == po
            mq = 0 if int(rd.flag[i]) & 0x8 else int(rd.mapq)
            rd.overrides[i] = dict(rd.overrides.get(i, {}), tags=b"MQC" + bytes([mq]) + sl.sa(value))
    return ic, refs, rd, names, (ta, pa, sa, tb, pb, sb)


# ---------------------------------------------------------------------- the cases worked by hand

HAND_CLENS = [10_000, 5_000]
A, C_, D = (0, 1_000, 0, 1, 500, 1), (0, 1_033, 0, 1, 500, 1), (0, 1_000, 0, 1, 533, 1)
# (name, links, parameters other than the driver's, the junctions worked by hand)
HAND = [
    ("three equal links", [A] * 3, {}, [A + (3, 3, 0)]),
    ("two one way and one the other", [A] * 2 + [rev(A)], {}, [A + (3, 2, 1)]),
    ("from the higher contig to the lower: the canonical flip", [rev(A)] * 3, {}, [A + (3, 0, 3)]),
    ("ends exactly W apart at both ends: near, the smaller E loses and counts in n1", [A] * 3 + [(0, 1_032, 0, 1, 532, 1)] * 2, {}, [A + (3, 5, 0)]),
    ("W + 1 apart at either end: three peaks", [A] * 3 + [C_] * 3 + [D] * 3, {}, [A + (3, 3, 0), D + (3, 3, 0), C_ + (3, 3, 0)]),
    ("a tie in E: the smaller p1, then the smaller p2", [(0, 1_010, 0, 1, 500, 1)] * 2 + [(0, 1_000, 0, 1, 520, 1)] * 2 + [(0, 1_000, 0, 1, 510, 1)] * 2, {},
     [(0, 1_000, 0, 1, 510, 1, 2, 6, 0)]),
    # 2 040 would have n1 = 3 were it a peak: it stays suppressed by 2 020, which 2 000 suppresses
    ("a chain 20 bases apart with E = 3, 2, 1: suppression is not transitive", [(0, 2_000, 0, 1, 900, 1)] * 3 + [(0, 2_020, 0, 1, 900, 1)] * 2 + [(0, 2_040, 0, 1, 900, 1)], {},
     [(0, 2_000, 0, 1, 900, 1, 3, 5, 0)]),
    ("spans of 49 and 50 on one contig", [(0, 3_000, 0, 0, 3_049, 1)] * 3 + [(0, 4_000, 0, 0, 4_050, 1)] * 3, {}, [(0, 4_000, 0, 0, 4_050, 1, 3, 3, 0)]),
    ("a link of span 40 is no candidate and still counts in n1", [(0, 5_000, 0, 0, 5_060, 1)] * 3 + [(0, 5_010, 0, 0, 5_050, 1)], {}, [(0, 5_000, 0, 0, 5_060, 1, 3, 4, 0)]),
    ("n1 + n2 of 2 and of 3", [(0, 6_000, 0, 1, 100, 1)] * 2 + [(0, 7_000, 0, 1, 200, 1), (1, 200, 1, 0, 7_000, 0), (0, 7_005, 0, 1, 203, 1)], {},
     [(0, 7_000, 0, 1, 200, 1, 2, 2, 1)]),
    # X (E 2) suppresses Y, Y suppresses Z; X has 3 links in its windows and is dropped at min_links 4; Y would have 4 and stays suppressed
    ("the threshold comes after the suppression", [(0, 1_000, 0, 1, 500, 1)] * 2 + [(0, 1_030, 0, 1, 500, 1), (0, 1_060, 0, 1, 500, 1)], {"min_links": 4}, []),
    ("ends at position 0 and at the contig's length, windows clipped at both", [(0, 0, 1, 1, 5_000, 0)] * 3 + [(0, 10, 1, 1, 4_990, 0)] + [(0, 10_000, 0, 1, 0, 1)] * 3, {},
     [(0, 0, 1, 1, 5_000, 0, 3, 4, 0), (0, 10_000, 0, 1, 0, 1, 3, 3, 0)]),
    ("windows across a bucket edge at 255 / 256", [(0, 255, 0, 1, 256, 1)] * 3 + [(0, 256, 0, 1, 255, 1)] * 2, {}, [(0, 255, 0, 1, 256, 1, 3, 5, 0)]),
    # 224 and 288 are inside the window of 256 and lose to it; 223 is a peak of two links and is dropped; 289 loses to 288
    ("a window of [224, 288]: 223 and 289 are outside", [(0, 256, 0, 1, 1_000, 1)] * 3 + [(0, p, 0, 1, 1_000, 1) for p in (223, 224, 288, 289)], {},
     [(0, 256, 0, 1, 1_000, 1, 3, 5, 0)]),
    ("the same at the far end of links stored the other way round", [(1, 2_000, 1, 0, 256, 0)] * 3 + [(1, 2_000, 1, 0, 224, 0), (1, 2_000, 1, 0, 289, 0)], {},
     [(0, 256, 0, 1, 2_000, 1, 3, 0, 4)]),
    ("min_span 0: a link whose two ends are one end is its own reverse and counts once", [(0, 800, 0, 0, 800, 0)] * 3, {"min_span": 0}, [(0, 800, 0, 0, 800, 0, 3, 3, 3)]),
    ("window 0: only equal tuples are near", [A] * 2 + [(0, 1_001, 0, 1, 500, 1)], {"window": 0, "min_links": 1}, [A + (2, 2, 0), (0, 1_001, 0, 1, 500, 1, 1, 1, 0)]),
]
