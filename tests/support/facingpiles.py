"""What tests/test_gpu_facing.py and tests/test_facing_host.py share: the plain restatement of the facing piles and of the consensus of a
pile (-I), written from the definitions in include/indelminer_amd.h (seam 5, "Facing piles" and "The consensus of a pile"), not from the
code under test.  tests/test_facing_host.py pins it to cases worked by hand (no GPU needed).  The clip arrays come from
tests/support/clipcounts.py (arrays_of*), the table from tests/support/cliptails.py (table_of*).

FACING PILES of one contig, R = clipR, L = clipL (clen + 1 counts each), m = min_reads, T = max_overlap: p is a pile iff R[p] >= m,
R[p] > R[x] for x in [p - T, p), R[p] >= R[x] for x in (p, p + T] (both clipped to [0, clen]) and the largest L[x] over [p - T, p]
(clipped), the largest x among equals, is >= m.  The answer is (pr = p, pl = x, cr = R[p], cl = L[x]), sorted by pr.

CONSENSUS of the entries at one key, c = min_cover: cover(i) = entries with more than i bases, len = #{i < 32: cover(i) >= c}, cons[i] =
the base most entries hold at i (the smallest code among equals), an entry agrees iff it differs from cons in at most min(n, len) >> 4 of
its first min(n, len) bases.  The answer is (entries, len, cons, agree), agree = 0 when len = 0.
"""
import numpy as np

from tests.support import clipcounts as cc
from tests.support import cliptails as ct
from tests.support.clipcounts import LEFT, RIGHT

MIN_READS, MAX_OVERLAP, MIN_COVER = 3, 30, 2        # what the host driver uses
NONE = 0xFFFFFFFF


def facing(R, L, m, T):
    """[(pr, pl, cr, cl)] of one contig's two arrays, pr ascending"""
    clen = len(R) - 1
    out = []
    for p in range(clen + 1):
        v = int(R[p])
        if v < m:
            continue
        lo, hi = max(p - T, 0), min(p + T, clen)
        if any(int(R[x]) >= v for x in range(lo, p)) or any(int(R[x]) > v for x in range(p + 1, hi + 1)):
            continue
        best, at = -1, p
        for x in range(p, lo - 1, -1):                  # downwards and strictly: the largest x among equal counts stays
            if int(L[x]) > best:
                best, at = int(L[x]), x
        if best >= m:
            out.append((p, at, v, best))
    return out


def facing_many(R, L, m, T):
    """the same with numpy doing the first cut (R >= m), for long contigs; the tests check it against facing first"""
    R, L = np.asarray(R), np.asarray(L)
    clen = len(R) - 1
    out = []
    for p in np.nonzero(R >= m)[0]:
        p = int(p)
        v, lo, hi = int(R[p]), max(p - T, 0), min(p + T, clen)
        if (R[lo:p] >= v).any() or (R[p + 1:hi + 1] > v).any():
            continue
        seg = L[lo:p + 1][::-1]
        k = int(np.argmax(seg))                         # numpy returns the first of equal maxima: the largest x
        if seg[k] >= m:
            out.append((p, p - k, v, int(seg[k])))
    return out


def consensus(entries, c):
    """(entries, len, cons, agree) of the entries (tuples of 2-bit codes, base 0 nearest the junction) stored at one key"""
    entries = list(entries)
    ln = sum(1 for i in range(ct.BASES) if sum(1 for e in entries if len(e) > i) >= c)
    cons = []
    for i in range(ln):
        votes = [sum(1 for e in entries if len(e) > i and e[i] == code) for code in range(4)]
        cons.append(votes.index(max(votes)))            # index: the smallest code among equals
    agree = 0
    for e in entries:
        k = min(len(e), ln)
        agree += ln > 0 and sum(1 for i in range(k) if e[i] != cons[i]) <= k >> 4
    return len(entries), ln, tuple(cons), int(agree)


def answer(table, tid, pos, side, c, clen):
    """what the device answers for one query: (entries, len, low-bit plane, high-bit plane, agree)"""
    if not 0 <= pos <= clen:
        return 0, 0, 0, 0, 0
    n, ln, cons, agree = consensus(table.get((tid, side, pos), []), c)
    lo, hi = ct.planes_of(cons)
    return n, ln, lo, hi, agree


HEADER = (
    "##fileformat=VCFv4.1\n"
    "##ALT=<ID=INS,Description=\"Insertion too long for a read to span: clipped reads from either side face each other\">\n"
    "##INFO=<ID=SVTYPE,Number=1,Type=String,Description=\"Type of structural variant\">\n"
    "##INFO=<ID=END,Number=1,Type=Integer,Description=\"Where the reads from the left stop aligning (POS: where the reads from the right start)\">\n"
    "##INFO=<ID=HOMLEN,Number=1,Type=Integer,Description=\"END - POS: bases aligned from both sides (target-site duplication or micro-homology)\">\n"
    "##INFO=<ID=CR,Number=2,Type=Integer,Description=\"Clipped reads that stop aligning at END, clipped reads that start aligning at POS\">\n"
    "##INFO=<ID=CN,Number=2,Type=Integer,Description=\"Of those, the reads whose clipped bases were kept, either side\">\n"
    "##INFO=<ID=CA,Number=2,Type=Integer,Description=\"Of those, the reads that agree with the consensus of their side\">\n"
    "##INFO=<ID=LSEQ,Number=1,Type=String,Description=\"First bases of the inserted sequence: consensus of the clipped bases behind END\">\n"
    "##INFO=<ID=RSEQ,Number=1,Type=String,Description=\"Last bases of the inserted sequence: consensus of the clipped bases in front of POS\">\n"
    "##largeInsertion=\"a record per position END at which at least 3 reads of mapping quality >= -q stop aligning with a soft clip of at least 20 bases, "
    "more than at any of the 30 positions in front and no fewer than at any of the 30 behind, when at least 3 such reads start aligning at one of "
    "the positions END - 30 .. END (POS: the one with the most, the nearest to END among equals); LSEQ and RSEQ: per base the majority of up to 32 "
    "clipped bases per read (A before C before G before T among equals), as far as at least 2 reads reach; CA: reads with at most 1 difference "
    "in 16 from it; CN, CA, LSEQ and RSEQ are . once the clip-tail table has overflowed (stderr says so); contig ends are skipped\"\n"
    "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\n")


def records_of(names, fasta, right, left, table):
    """[(contig, pr, pl, cr, cl, (entries, len, cons, agree) right, the same left)] the driver prints: contig ends are skipped"""
    out = []
    for tid, name in enumerate(names):
        clen = len(right[tid]) - 1
        for pr, pl, cr, cl in facing_many(right[tid], left[tid], MIN_READS, MAX_OVERLAP):
            if pl == 0 or pr == clen:
                continue
            out.append((name, pr, pl, cr, cl, consensus(table.get((tid, RIGHT, pr), []), MIN_COVER),
                        consensus(table.get((tid, LEFT, pl), []), MIN_COVER)))
    return out


def render(names, fasta, right, left, table):
    """FILE as the driver writes it, from the restatement"""
    text = lambda cons: "".join("ACGT"[b] for b in cons) or "."
    lines = [HEADER]
    for name, pr, pl, cr, cl, (nr, _lr, consr, ar), (nl, _ll, consl, al) in records_of(names, fasta, right, left, table):
        lines.append("%s\t%d\t.\t%s\t<INS>\t.\t.\tSVTYPE=INS;END=%d;HOMLEN=%d;CR=%d,%d;CN=%d,%d;CA=%d,%d;LSEQ=%s;RSEQ=%s\n" % (
            name, pl, fasta[name][pl - 1:pl].decode().upper(), pr, pr - pl, cr, cl, nr, nl, ar, al, text(consr), text(consl[::-1])))
    return "".join(lines).encode()


def render_of_bam(bam, fasta_path, q):
    """(FILE, records, table) from BAM + FASTA at -q q"""
    names, right, left = cc.arrays_of_bam(bam, cc.MIN_CLIP, q)
    table = ct.table_of_bam(bam, cc.MIN_CLIP, q)[1]
    fasta = ct.read_fasta(fasta_path)
    return render(names, fasta, right, left, table), records_of(names, fasta, right, left, table), table


# ---------------------------------------------------------------------- the planted data set

SITES = [(6700 + 5000 * k, 3 * k) for k in range(10)]       # (p, d): insertion point and target-site duplication
INS_LEN = 400


def planted_reads():
    """(refs, rd, insertions): the simulator's 60 kb contig at 30x with ten insertions of 400 bases planted into its reads.  At each
    site (p, d), of the mapped single-M reads with pos <= p - d - 25 and pos + 100 >= p + 25 in arrival order, the 1st, 4th, ... become
    aM(100 - a)S at p and carry the insertion's first bases, the 2nd, 5th, ... become cS(100 - c)M, start at p - d and carry its last
    bases, every third stays; then the columns are sorted again, stably, by (tid, pos)."""
    from indelminer_amd import synth
    refs, rd = synth.simulate(seed=31, ref_len=60_000, coverage=30, n_contigs=1)
    rng = np.random.default_rng(77)
    insertions = [synth.ACGT[rng.integers(0, 4, INS_LEN)] for _ in SITES]
    L = rd.read_len
    for (p, d), ins in zip(SITES, insertions):
        plain = (rd.ncig == 1) & (rd.cig_op[:, 0] == synth.OP_M) & ((rd.flag & 0x4) == 0)
        over = np.nonzero(plain & (rd.pos <= p - d - 25) & (rd.pos + L >= p + 25))[0]
        for j, i in enumerate(over):
            pos = int(rd.pos[i])
            if j % 3 == 0:
                a = p - pos
                rd.cig_op[i, :2] = (synth.OP_M, synth.OP_S); rd.cig_len[i, :2] = (a, L - a); rd.ncig[i] = 2
                rd.seq[i, a:] = ins[:L - a]
            elif j % 3 == 1:
                c = p - d - pos
                rd.cig_op[i, :2] = (synth.OP_S, synth.OP_M); rd.cig_len[i, :2] = (c, L - c); rd.ncig[i] = 2
                rd.seq[i, :c] = ins[INS_LEN - c:]
                rd.pos[i] = p - d
    order = np.lexsort((rd.pos, rd.tid))                # stable
    for k, v in list(vars(rd).items()):
        if isinstance(v, np.ndarray) and len(v) == rd.n:
            setattr(rd, k, v[order])
    return refs, rd, insertions


def write_planted(d, refs, rd, lower_mapq_of_every_second_clipped_read=False):
    """ref.fa, aln.bam (+ .bai) and cfg.txt in directory d"""
    from indelminer_amd import bamwrite, synth
    if lower_mapq_of_every_second_clipped_read:
        last = np.maximum(rd.ncig.astype(np.int64) - 1, 0)
        clipped = np.nonzero((rd.ncig > 1) & ((rd.cig_op[:, 0] == synth.OP_S) | (rd.cig_op[np.arange(rd.n), last] == synth.OP_S)))[0]
        rd.overrides = {int(i): {"mapq": 20} for i in clipped[::2]}
    contigs = [("ctg0", len(refs[0]))]
    bamwrite.write_fasta(d + "/ref.fa", contigs, refs)
    bamwrite.write_bam(d + "/aln.bam", contigs, rd)
    open(d + "/cfg.txt", "w").write("IL generic 300 700\n")
    return d
