"""What tests/test_gpu_crossed.py and tests/test_crossed_host.py share: the plain restatement of the peaks of a clip array and of the
crossed piles (-U), written from the definition in include/indelminer_amd.h (seam 5, "Crossed piles"), not from the code under test.
tests/test_crossed_host.py pins it to cases worked by hand (no GPU needed).  The clip arrays come from tests/support/clipcounts.py
(arrays_of*), the table and the match rule from tests/support/cliptails.py (table_of*, matches).

PEAK of an array A (clen + 1 counts), m = min_reads, T = reach: A[p] >= m, A[p] > A[x] for x in [p - T, p), A[p] >= A[x] for x in
(p, p + T], both clipped to [0, clen].
CANDIDATE: a peak pr of clipR and a peak pl of clipL with dmin <= pr - pl <= dmax.  vR(s): the right entries at pr that match
ref[pl + s + i], vL(s): the left entries at pl that match ref[pr - 1 - s - i] (cliptails.matches).  The chosen s in 0 .. S has the
largest vR + vL, the smallest among equals; the candidate qualifies iff vR >= mv and vL >= mv there.  The answer is
(pr, pl, cr, cl, vR, vL, s, stored right, stored left) per qualifying pair, sorted by (pr, pl).
"""
import numpy as np

from tests.support import clipcounts as cc
from tests.support import cliptails as ct
from tests.support.clipcounts import LEFT, RIGHT

MIN_READS, REACH, MIN_LEN, MAX_LEN, MAX_SHIFT, MIN_VERIFIED = 3, 30, 50, 100_000, 32, 2       # what the host driver uses


def peaks(A, m, T):
    """[(p, A[p])] of one array, p ascending"""
    clen = len(A) - 1
    out = []
    for p in range(clen + 1):
        v = int(A[p])
        if v < m:
            continue
        lo, hi = max(p - T, 0), min(p + T, clen)
        if any(int(A[x]) >= v for x in range(lo, p)) or any(int(A[x]) > v for x in range(p + 1, hi + 1)):
            continue
        out.append((p, v))
    return out


def peaks_many(A, m, T):
    """the same with numpy doing the first cut (A >= m), for long contigs; the tests check it against peaks first"""
    A = np.asarray(A)
    clen = len(A) - 1
    out = []
    for p in np.nonzero(A >= m)[0]:
        p = int(p)
        v, lo, hi = int(A[p]), max(p - T, 0), min(p + T, clen)
        if (A[lo:p] >= v).any() or (A[p + 1:hi + 1] > v).any():
            continue
        out.append((p, v))
    return out


def chosen(R, Lf, ref, pr, pl, S):
    """(vR, vL, s) at the chosen shift of one candidate; R, Lf: the entries at (pr, right) and (pl, left)"""
    best = (0, 0, 0)
    for s in range(S + 1):
        vr = sum(ct.matches(b, ref, pl + s, 1) for b in R)
        vl = sum(ct.matches(b, ref, pr - 1 - s, -1) for b in Lf)
        if s == 0 or vr + vl > best[0] + best[1]:           # strictly: the smallest shift among equal sums stays
            best = (vr, vl, s)
    return best


def shift_counts(entries, code, start, step, S):
    """v(0 .. S) of one pile through numpy: entry base i at shift s is expected to be code[start + step * (s + i)]"""
    v = np.zeros(S + 1, np.int64)
    if not entries:
        return v
    n = np.array([len(b) for b in entries])
    B = np.full((len(entries), ct.BASES), 254, np.uint8)
    for k, b in enumerate(entries):
        B[k, :len(b)] = b
    idx = start + step * (np.arange(S + 1)[:, None] + np.arange(ct.BASES)[None, :])
    want = np.where((idx >= 0) & (idx < len(code)), code[np.clip(idx, 0, len(code) - 1)], 255)
    bad = ((want[None, :, :] != B[:, None, :]) & (np.arange(ct.BASES)[None, None, :] < n[:, None, None])).sum(2)
    return (bad <= (n >> 4)[:, None]).sum(0)


def crossed(R, L, table, ref, tid, m, T, dmin, dmax, S, mv, many=True):
    """[(pr, pl, cr, cl, vR, vL, s, stored right, stored left)] of one contig, sorted by (pr, pl); many: the numpy forms (the tests
    check them against the plain ones).  Also returns the number of candidates."""
    find = peaks_many if many else peaks
    pr_list, pl_list = find(R, m, T), find(L, m, T)
    code = ct.ref_codes(ref) if many else None
    out, n_cand = [], 0
    for pr, cr in pr_list:
        for pl, cl in pl_list:
            if not dmin <= pr - pl <= dmax:
                continue
            n_cand += 1
            Re, Le = table.get((tid, RIGHT, pr), []), table.get((tid, LEFT, pl), [])
            if many:
                vr, vl = shift_counts(Re, code, pl, 1, S), shift_counts(Le, code, pr - 1, -1, S)
                s = int(np.argmax(vr + vl))                 # numpy returns the first of equal maxima
                vr, vl = int(vr[s]), int(vl[s])
            else:
                vr, vl, s = chosen(Re, Le, ref, pr, pl, S)
            if vr >= mv and vl >= mv:
                out.append((pr, pl, cr, cl, vr, vl, s, len(Re), len(Le)))
    return out, n_cand


def header(depth):
    h = (
        "##fileformat=VCFv4.1\n"
        "##ALT=<ID=DUP:TANDEM,Description=\"Tandem duplication: reads clipped at its end continue at its start\">\n"
        "##INFO=<ID=SVTYPE,Number=1,Type=String,Description=\"Type of structural variant\">\n"
        "##INFO=<ID=END,Number=1,Type=Integer,Description=\"Last duplicated base: where the reads from the left stop aligning (POS + 1: the first, where the reads from the right start)\">\n"
        "##INFO=<ID=SVLEN,Number=1,Type=Integer,Description=\"END - POS: bases duplicated\">\n"
        "##INFO=<ID=HOMLEN,Number=1,Type=Integer,Description=\"Bases by which the clipped reads continue behind the other breakpoint (micro-homology the aligner extended into)\">\n"
        "##INFO=<ID=CR,Number=2,Type=Integer,Description=\"Clipped reads that stop aligning at END, clipped reads that start aligning at POS\">\n"
        "##INFO=<ID=CN,Number=2,Type=Integer,Description=\"Of those, the reads whose clipped bases were kept, either side\">\n"
        "##INFO=<ID=CV,Number=2,Type=Integer,Description=\"Of those, the reads whose clipped bases are the reference at the other breakpoint\">\n")
    if depth:
        h += ("##INFO=<ID=DM,Number=3,Type=Integer,Description=\"Median depth over the duplicated bases POS+1..END, over the 1000 bases in front of them and over the 1000 bases behind them\">\n"
              "##INFO=<ID=DFC,Number=1,Type=Integer,Description=\"Depth fold change in thousandths: the first DM value over the mean of the other two\">\n")
    return h + (
        "##tandemDuplication=\"a record per pair of positions END and POS, 50 <= END - POS <= 100000, where END is a position at which at least 3 reads of mapping "
        "quality >= -q stop aligning with a soft clip of at least 20 bases, more than at any of the 30 positions in front and no fewer than at any of the 30 "
        "behind, and POS is such a position of the reads that start aligning with such a clip, when for one shift s in 0 .. 32 at least 2 of the reads at END "
        "continue with the reference from POS + s on and at least 2 of the reads at POS continue backwards with the reference from END - 1 - s on, in up to 32 "
        "clipped bases per read with at most 1 difference in 16 (HOMLEN: the s with the most such reads, the smallest among equals; CV: those reads); "
        "the file has no records once the clip-tail table has overflowed (stderr says so); POS 0 is skipped\"\n"
        "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\n")


def records_of(names, fasta, right, left, table):
    """([(contig, pr, pl, cr, cl, vR, vL, s, stored right, stored left)] the driver prints (POS 0 is skipped), candidates, peaks)"""
    out, n_cand, n_peaks = [], 0, [0, 0]
    for tid, name in enumerate(names):
        pairs, n = crossed(right[tid], left[tid], table, fasta[name], tid, MIN_READS, REACH, MIN_LEN, MAX_LEN, MAX_SHIFT, MIN_VERIFIED)
        n_cand += n
        n_peaks[0] += len(peaks_many(right[tid], MIN_READS, REACH)); n_peaks[1] += len(peaks_many(left[tid], MIN_READS, REACH))
        out += [(name,) + p for p in pairs if p[1] != 0]
    return out, n_cand, tuple(n_peaks)


def render(names, fasta, right, left, table, depth=None):
    """FILE as the driver writes it, from the restatement; depth: per contig the depth array (-D), or None"""
    from tests.support.depthmedian import evidence_of
    lines = [header(depth is not None)]
    for name, pr, pl, cr, cl, vr, vl, s, nr, nl in records_of(names, fasta, right, left, table)[0]:
        more = ""
        if depth is not None:
            more = ";DM=%s;DFC=%s" % evidence_of(depth[names.index(name)], pl, pr)
        lines.append("%s\t%d\t.\t%s\t<DUP:TANDEM>\t.\t.\tSVTYPE=DUP;END=%d;SVLEN=%d;HOMLEN=%d;CR=%d,%d;CN=%d,%d;CV=%d,%d%s\n" % (
            name, pl, fasta[name][pl - 1:pl].decode().upper(), pr, pr - pl, s, cr, cl, nr, nl, vr, vl, more))
    return "".join(lines).encode()


def render_of_bam(bam, fasta_path, q, depth=None):
    """(FILE, records, candidates, peaks) from BAM + FASTA at -q q"""
    names, right, left = cc.arrays_of_bam(bam, cc.MIN_CLIP, q)
    table = ct.table_of_bam(bam, cc.MIN_CLIP, q)[1]
    fasta = ct.read_fasta(fasta_path)
    return (render(names, fasta, right, left, table, depth),) + records_of(names, fasta, right, left, table)


# ---------------------------------------------------------------------- the planted data set

# (pl, length): a tandem duplication of the bases [pl, pl + length).  Every 5 000 bases from 6 700 on, except where the simulator's own
# variants leave too few plain reads across a breakpoint (36 700 and 41 700): those two stand 500 and 1 000 further on.
LENGTHS = [50, 60, 75, 100, 150, 300, 1_000, 3_000, 4_990]
STARTS = [6_700 + 5_000 * k for k in range(9)]
STARTS[6] += 500; STARTS[7] += 1_000
SITES = list(zip(STARTS, LENGTHS))


def planted_reads():
    """(refs, rd): the simulator's 60 kb contig at 30x with nine tandem duplications planted into its reads.  At each site (pl, n),
    pr = pl + n: of the mapped single-M reads that span pl with 25 bases on either side, in arrival order, every second becomes
    cS(100 - c)M, starts at pl and carries ref[pl - c .. ] replaced by the end of the copy in front, ref[pr - c, pr); then of those that
    span pr (and are still single-M) every second becomes aM(100 - a)S and carries the start of the copy behind, ref[pl, pl + 100 - a).
    The columns are sorted again, stably, by (tid, pos)."""
    from indelminer_amd import synth
    refs, rd = synth.simulate(seed=31, ref_len=60_000, coverage=30, n_contigs=1)
    ref = refs[0]
    L = rd.read_len
    for pl, n in SITES:
        pr = pl + n
        plain = lambda: (rd.ncig == 1) & (rd.cig_op[:, 0] == synth.OP_M) & ((rd.flag & 0x4) == 0)
        for j, i in enumerate(np.nonzero(plain() & (rd.pos <= pl - 25) & (rd.pos + L >= pl + 25))[0]):
            if j % 2 == 0:
                c = pl - int(rd.pos[i])
                rd.cig_op[i, :2] = (synth.OP_S, synth.OP_M); rd.cig_len[i, :2] = (c, L - c); rd.ncig[i] = 2
                rd.seq[i, :c] = ref[pr - c:pr]
                rd.pos[i] = pl
        for j, i in enumerate(np.nonzero(plain() & (rd.pos <= pr - 25) & (rd.pos + L >= pr + 25))[0]):
            if j % 2 == 0:
                a = pr - int(rd.pos[i])
                rd.cig_op[i, :2] = (synth.OP_M, synth.OP_S); rd.cig_len[i, :2] = (a, L - a); rd.ncig[i] = 2
                rd.seq[i, a:] = ref[pl:pl + L - a]
    order = np.lexsort((rd.pos, rd.tid))                # stable
    for k, v in list(vars(rd).items()):
        if isinstance(v, np.ndarray) and len(v) == rd.n:
            setattr(rd, k, v[order])
    return refs, rd


def write_planted(d, refs, rd, lower_mapq_of_every_second_clipped_read=False):
    """ref.fa, aln.bam (+ .bai) and cfg.txt in directory d"""
    from tests.support import facingpiles
    return facingpiles.write_planted(d, refs, rd, lower_mapq_of_every_second_clipped_read)
