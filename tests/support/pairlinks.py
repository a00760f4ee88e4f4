"""What tests/test_gpu_pairlink.py and tests/test_pairlink_host.py share: the plain restatement of the pair links (-M), written from the
definition in include/indelminer_amd.h (seam 5, "Pair links"), not from the code under test.  tests/test_pairlink_host.py pins it to
cases worked by hand (no GPU needed).  The records of the two FILEs come from tests/support/crossedpiles.py and invertedpiles.py.

A record is anything with tid, pos, mapq, flag, mtid, mpos (tests/support/bamlite.py's Record, or Rec below).  It is a LINK
(tid, kind, pos, mpos) iff it is paired, none of 0x4 0x8 0x100 0x200 0x400 0x800 is set, 0 <= tid < contigs, mtid == tid, it is the
leftmost of its pair (pos < mpos, or pos == mpos and first in pair), mapq >= q, both positions lie in [0, length], and the pair is not
in the normal orientation: (reverse, mate reverse) = (1, 0) kind 0 EVERTED, (0, 0) kind 1 FORWARD, (1, 1) kind 2 REVERSE, (0, 1) none.
A QUERY (tid, kind, a0, a1, b0, b1) with min_sep counts the links of that kind with a0 <= pos <= a1, b0 <= mpos <= b1 (both clipped to
[0, length]) and mpos - pos >= min_sep.
"""
import struct
from collections import namedtuple

import numpy as np

EVERTED, FORWARD, REVERSE = 0, 1, 2
WINDOW, REACH, MIN_SEP = 1_000, 32, 50          # what the host driver uses: LINK_EV_WINDOW, CLIPTAIL_MAX_SHIFT, LINK_EV_MIN_SEP
NONE = 0xFFFFFFFF
EXCLUDED = 0x4 | 0x8 | 0x100 | 0x200 | 0x400 | 0x800

Rec = namedtuple("Rec", "tid pos mapq flag mtid mpos")


def link_of(rec, clens, q):
    """(tid, kind, pos, mpos) of one record, or None"""
    f = rec.flag
    if not f & 0x1 or f & EXCLUDED:
        return None
    if not 0 <= rec.tid < len(clens) or rec.mtid != rec.tid:
        return None
    if not (rec.pos < rec.mpos or (rec.pos == rec.mpos and f & 0x40)):
        return None
    if rec.mapq < q:
        return None
    if not (0 <= rec.pos <= clens[rec.tid] and 0 <= rec.mpos <= clens[rec.tid]):
        return None
    kind = {(1, 0): EVERTED, (0, 0): FORWARD, (1, 1): REVERSE}.get(((f >> 4) & 1, (f >> 5) & 1))
    return None if kind is None else (rec.tid, kind, rec.pos, rec.mpos)


def links_of(records, clens, q):
    return [x for x in (link_of(r, clens, q) for r in records) if x is not None]


def count(links, clens, tid, kind, a0, a1, b0, b1, min_sep):
    """the answer to one query"""
    a0, b0, a1, b1 = max(a0, 0), max(b0, 0), min(a1, clens[tid]), min(b1, clens[tid])
    if a0 > a1 or b0 > b1:
        return 0
    return sum(1 for t, k, p, m in links if t == tid and k == kind and a0 <= p <= a1 and b0 <= m <= b1 and m - p >= min_sep)


def window_of(svtype, ct, first, second):
    """(kind, a0, a1, b0, b1) of a printed record: <DUP:TANDEM> POS = pl, END = pr; <INV> POS = x, END = y with its CT"""
    if svtype == "DUP":
        return EVERTED, first - REACH, first + WINDOW, second - WINDOW, second + REACH
    if ct == "3to3":
        return FORWARD, first - WINDOW, first + REACH, second - WINDOW, second + REACH
    return REVERSE, first - REACH, first + WINDOW, second - REACH, second + WINDOW


def links_of_bam(bam, q):
    """(contig names, contig lengths, links) of a BAM file"""
    from tests.support import bamlite
    _, refs, recs = bamlite.read_bam(bam)
    clens = [n for _, n in refs]
    return [n for n, _ in refs], clens, links_of(recs, clens, q)


PE_INFO = {
    "DUP": "##INFO=<ID=PE,Number=1,Type=Integer,Description=\"everted read pairs (the leftmost read reverse, its mate forward) that start within POS - 32 .. "
           "POS + 1000 and whose mate starts within END - 1000 .. END + 32, at least 50 bases apart\">\n",
    "INV": "##INFO=<ID=PE,Number=1,Type=Integer,Description=\"read pairs with both reads forward (CT=3to3: both start within 1000 bases in front of and 32 "
           "behind POS and END) or both reverse (CT=5to5: within 32 in front of and 1000 behind), at least 50 bases apart\">\n",
}
PAIR_LINKS = (
    "##pairLinks=\"PE counts read pairs on one contig, each once at its leftmost read: paired, both reads mapped, neither secondary, supplementary, duplicate "
    "nor failing quality control, the leftmost read of mapping quality >= -q, both starts inside the contig, in the orientation of the record's junction "
    "(the normal one, forward in front of reverse, never counts, whatever its insert size); start of the leftmost read and start of its mate each within a "
    "window that reaches 1000 bases from the record's breakpoint towards where the junction's pairs lie and 32 bases the other way, the two starts at "
    "least 50 bases apart; PE is . once the pair-link table has overflowed (stderr says so); a duplication shorter than a read leaves no everted pair: "
    "PE=0 is expected there; pairs whose mate lies on another contig are not counted\"\n")


def with_pe(text, svtype, names, clens, links, overflowed=False):
    """(a FILE of -U (svtype "DUP") or -N ("INV") as it is written with -M, [(contig, POS, END, CT or None, PE)]): the PE line behind the
    other ##INFO lines, the ##pairLinks line behind the file's own description line, ;PE=n at the end of every record"""
    lines = text.decode().split("\n")
    assert lines[-1] == ""
    last_info = max(i for i, ln in enumerate(lines) if ln.startswith("##INFO"))
    chrom = next(i for i, ln in enumerate(lines) if ln.startswith("#CHROM"))
    assert chrom == last_info + 2 and lines[chrom - 1].startswith("##")
    out, found = [], []
    for i, ln in enumerate(lines[:-1]):
        if i > chrom:
            f = ln.split("\t")
            info = dict(kv.split("=") for kv in f[7].split(";"))
            pos, end, ct = int(f[1]), int(info["END"]), info.get("CT")
            n = count(links, clens, names.index(f[0]), *window_of(svtype, ct, pos, end), MIN_SEP)
            found.append((f[0], pos, end, ct, n))
            ln += ";PE=." if overflowed else ";PE=%d" % n
        out.append(ln + "\n")
        if i == last_info:
            out.append(PE_INFO[svtype])
        if i == chrom - 1:
            out.append(PAIR_LINKS)
    return "".join(out).encode(), found


def render_of_bam(svtype, bam, fasta_path, q, depth=None):
    """(FILE without -M, FILE with -M, [(contig, POS, END, CT, PE)]) from BAM + FASTA at -q q; depth: -U's -D fields"""
    from tests.support import crossedpiles as cp
    from tests.support import invertedpiles as ip
    plain = cp.render_of_bam(bam, fasta_path, q, depth)[0] if svtype == "DUP" else ip.render_of_bam(bam, fasta_path, q)[0]
    names, clens, links = links_of_bam(bam, q)
    return (plain,) + with_pe(plain, svtype, names, clens, links)


# ---------------------------------------------------------------------- raw records for the scatter

def pack_records(records, qual=True):
    """[Rec] -> the device layout (raw uint8, rec_off uint32[n + 1]): the core with mtid and mpos, a name, one CIGAR operation, 10 packed
    bases, qualities (qual=False: without them and with bin = 0xFFFF, as the product's walkers deliver records), one aux tag"""
    blob, off = bytearray(), [0]
    for i, r in enumerate(records):
        qname = b"p%d\0" % i
        core = struct.pack("<iiBBHHHiiii", r.tid, r.pos, len(qname), r.mapq, 4680 if qual else 0xFFFF, 1, r.flag, 10, r.mtid, r.mpos, 0)
        body = core + qname + struct.pack("<I", 10 << 4) + b"\x12\x48\x12\x48\x12" + (b"\x28" * 10 if qual else b"") + b"NMC\x01"
        blob += body + b"\0" * (-len(body) % 4)
        off.append(len(blob))
    return np.frombuffer(bytes(blob), np.uint8).copy(), np.array(off, np.uint32)


# ---------------------------------------------------------------------- the planted data sets

MIN_SITE = 300          # the shortest planted site that gets pairs: a duplication shorter than a read leaves none
PAIRS_PER_JUNCTION = 4


def planted_pairs(a0, a1, b0, b1):
    """the four (pos, mpos) planted at one junction whose query is ([a0, a1], [b0, b1]): the leftmost read exactly on the window's lower
    edge, exactly on its upper edge, in its middle, and ONE BASE IN FRONT of the lower edge.  Where no pair can stand on the upper edge
    at all -- a duplication of 300 or 1 000 bases: a1 + MIN_SEP lies behind b1 -- the second stands on the last position that still
    has a mate, b1 - MIN_SEP, with its mate on b1: the mate window's upper edge and min_sep's edge at once.  Three of the four count."""
    hi = a1 if a1 + MIN_SEP <= b1 else b1 - MIN_SEP
    out = []
    for pos in (a0, hi, (a0 + hi) // 2, a0 - 1):
        out.append((pos, min(max(b0, pos + MIN_SEP) + 7, b1)))
    return out


def _rewrite(refs, rd, junctions):
    """junctions: [(kind, a0, a1, b0, b1)].  Takes plain proper pairs of the quiet stretch in front of the first site (both reads one M,
    the pair starting in [500, 5 500)), in arrival order, and moves each to a planted (pos, mpos) in the junction's orientation: both
    reads 100M on the reference's own bases there, no longer a proper pair.  Sorted again, stably, by (tid, pos).  Returns the planted
    [(kind, pos, mpos)]."""
    from indelminer_amd import synth
    ref, L = refs[0], rd.read_len
    plain = (rd.ncig == 1) & (rd.cig_op[:, 0] == synth.OP_M) & ((rd.flag & (0x4 | 0x8)) == 0) & ((rd.flag & 0x2) != 0)
    first = np.nonzero(plain & (rd.pos >= 500) & (rd.pos < 5_500) & (rd.pos < rd.mpos))[0]
    by_pair = {}
    for i in np.nonzero(plain)[0]:
        by_pair.setdefault(int(rd.pair_id[i]), []).append(int(i))
    free = iter([(int(i), [j for j in by_pair[int(rd.pair_id[i])] if j != i]) for i in first])
    planted = []
    strands = {EVERTED: (1, 0), FORWARD: (0, 0), REVERSE: (1, 1)}
    for kind, a0, a1, b0, b1 in junctions:
        for pos, mpos in planted_pairs(a0, a1, b0, b1):
            i, mates = next(free)
            while len(mates) != 1:
                i, mates = next(free)
            j = mates[0]
            r, m = strands[kind]
            for k, p, mp, rev, mrev, sign in ((i, pos, mpos, r, m, 1), (j, mpos, pos, m, r, -1)):
                rd.pos[k] = p; rd.mpos[k] = mp
                rd.flag[k] = (int(rd.flag[k]) & ~(0x2 | 0x10 | 0x20)) | (0x10 if rev else 0) | (0x20 if mrev else 0)
                rd.isize[k] = sign * (mpos + L - pos)
                rd.seq[k] = ref[p:p + L]
            planted.append((kind, pos, mpos))
    order = np.lexsort((rd.pos, rd.tid))                # stable
    for k, v in list(vars(rd).items()):
        if isinstance(v, np.ndarray) and len(v) == rd.n:
            setattr(rd, k, v[order])
    return planted


def planted_dup_reads():
    """(refs, rd, planted): crossedpiles' planted duplications, with four everted pairs at every site of at least 300 bases"""
    from tests.support import crossedpiles as cp
    refs, rd = cp.planted_reads()
    return refs, rd, _rewrite(refs, rd, [window_of("DUP", None, pl, pl + n) for pl, n in cp.SITES if n >= MIN_SITE])


def planted_inv_reads():
    """(refs, rd, planted): invertedpiles' planted inversions, with four forward pairs at the left junction and four reverse pairs at the
    right junction of every site of at least 300 bases"""
    from tests.support import invertedpiles as ip
    refs, rd = ip.planted_reads()
    return refs, rd, _rewrite(refs, rd, [window_of("INV", ct, a, a + n) for a, n in ip.SITES if n >= MIN_SITE for ct in ("3to3", "5to5")])


def planted_overflow_reads(n_pairs=2_100):
    """(refs, rd): crossedpiles' planted duplications with the first n_pairs plain proper pairs (both reads one M) turned everted in
    their flags alone -- more links than the 2 048 the driver's smallest table keeps"""
    from indelminer_amd import synth
    from tests.support import crossedpiles as cp
    refs, rd = cp.planted_reads()
    plain = (rd.ncig == 1) & (rd.cig_op[:, 0] == synth.OP_M) & ((rd.flag & (0x4 | 0x8)) == 0) & ((rd.flag & 0x2) != 0)
    by_pair = {}
    for i in np.nonzero(plain)[0]:
        by_pair.setdefault(int(rd.pair_id[i]), []).append(int(i))
    done = 0
    for i in np.nonzero(plain & (rd.pos < rd.mpos))[0]:
        both = by_pair[int(rd.pair_id[i])]
        if len(both) != 2 or done == n_pairs:
            continue
        j = both[0] if both[1] == i else both[1]
        rd.flag[i] = (int(rd.flag[i]) & ~(0x2 | 0x20)) | 0x10
        rd.flag[j] = (int(rd.flag[j]) & ~(0x2 | 0x10)) | 0x20
        done += 1
    assert done == n_pairs
    return refs, rd


def write_planted(d, refs, rd):
    """ref.fa, aln.bam (+ .bai) and cfg.txt in directory d"""
    from tests.support import facingpiles
    return facingpiles.write_planted(d, refs, rd)
