"""What tests/test_gpu_inverted.py and tests/test_inverted_host.py share: the plain restatement of the inverted piles (-N), written from
the definition in include/indelminer_amd.h (seam 5, "Inverted piles"), not from the code under test.  tests/test_inverted_host.py pins
it to cases worked by hand (no GPU needed).  The peaks come from tests/support/crossedpiles.py (peaks, peaks_many), the clip arrays from
tests/support/clipcounts.py (arrays_of*), the table and ref_codes from tests/support/cliptails.py.

CANDIDATE of side sigma (0 = clipR, 1 = clipL): two peaks x < y of the SAME array with dmin <= y - x <= dmax.  An entry of n bases matches
iff at most n >> 4 of its bases differ from what is expected; no base (outside the contig, not A / C / G / T) is a mismatch.  Base i at
shift s is expected to be
    sigma = 0:  at x  comp(ref[y - 1 - s - i])      at y  comp(ref[x - 1 - s - i])
    sigma = 1:  at x  comp(ref[y + s + i])          at y  comp(ref[x + s + i])
v1(s), v2(s): the matching entries at x and at y.  The chosen s in 0 .. S has the largest v1 + v2, the smallest among equals; the
candidate qualifies iff v1 >= mv and v2 >= mv there.  The answer is (side, x, y, c1, c2, v1, v2, s, stored at x, stored at y) per
qualifying pair, sorted by (x, y, side).
"""
import numpy as np

from tests.support import clipcounts as cc
from tests.support import cliptails as ct
from tests.support.clipcounts import LEFT, RIGHT
from tests.support.crossedpiles import peaks, peaks_many, shift_counts

MIN_READS, REACH, MIN_LEN, MAX_LEN, MAX_SHIFT, MIN_VERIFIED = 3, 30, 50, 1_000_000, 32, 2     # what the host driver uses
COMP = {ord("A"): 3, ord("C"): 2, ord("G"): 1, ord("T"): 0}                                   # the code of the complement of a reference byte


def matches(bases, ref, start, step):
    """whether an entry matches the other strand: base i is expected to be comp(ref[start + step * i]) (ref: the contig's bytes)"""
    bad = 0
    for i, b in enumerate(bases):
        p = start + step * i
        if not 0 <= p < len(ref) or COMP.get(ref[p]) != b:
            bad += 1
    return bad <= len(bases) >> 4


def windows(side, x, y):
    """((start, step) of what the entries at x are compared with at shift 0, the same for the entries at y)"""
    return ((y - 1, -1), (x - 1, -1)) if side == RIGHT else ((y, 1), (x, 1))


def chosen(E1, E2, ref, side, x, y, S):
    """(v1, v2, s) at the chosen shift of one candidate; E1, E2: the entries at (x, side) and (y, side)"""
    (a1, d1), (a2, d2) = windows(side, x, y)
    best = (0, 0, 0)
    for s in range(S + 1):
        v1 = sum(matches(b, ref, a1 + d1 * s, d1) for b in E1)
        v2 = sum(matches(b, ref, a2 + d2 * s, d2) for b in E2)
        if s == 0 or v1 + v2 > best[0] + best[1]:           # strictly: the smallest shift among equal sums stays
            best = (v1, v2, s)
    return best


def comp_codes(ref):
    """the contig's complement as 2-bit codes, 255 where the byte is not A, C, G or T"""
    code = ct.ref_codes(ref)
    return np.where(code < 4, 3 - code, 255).astype(np.uint8)


def inverted(R, L, table, ref, tid, m, T, dmin, dmax, S, mv, many=True):
    """[(side, x, y, c1, c2, v1, v2, s, stored at x, stored at y)] of one contig, sorted by (x, y, side); many: the numpy forms (the
    tests check them against the plain ones), with the partners of a peak looked up in the sorted list instead of tried one by one.
    Also returns the candidates per side."""
    find = peaks_many if many else peaks
    code = comp_codes(ref) if many else None
    out, n_cand = [], [0, 0]
    for side, A in ((RIGHT, R), (LEFT, L)):
        found = find(A, m, T)
        at = np.array([p for p, _ in found], np.int64)
        for x, c1 in found:
            partners = found[int(np.searchsorted(at, x + dmin)):int(np.searchsorted(at, x + dmax, "right"))] if many else found
            for y, c2 in partners:
                if not dmin <= y - x <= dmax:
                    continue
                n_cand[side] += 1
                E1, E2 = table.get((tid, side, x), []), table.get((tid, side, y), [])
                if many:
                    (a1, d1), (a2, d2) = windows(side, x, y)
                    v1, v2 = shift_counts(E1, code, a1, d1, S), shift_counts(E2, code, a2, d2, S)
                    s = int(np.argmax(v1 + v2))             # numpy returns the first of equal maxima
                    v1, v2 = int(v1[s]), int(v2[s])
                else:
                    v1, v2, s = chosen(E1, E2, ref, side, x, y, S)
                if v1 >= mv and v2 >= mv:
                    out.append((side, x, y, c1, c2, v1, v2, s, len(E1), len(E2)))
    return sorted(out, key=lambda r: (r[1], r[2], r[0])), tuple(n_cand)


def header():
    return (
        "##fileformat=VCFv4.1\n"
        "##ALT=<ID=INV,Description=\"Inversion breakpoint: reads clipped on one side at POS and at END continue on the other strand at each other\">\n"
        "##INFO=<ID=SVTYPE,Number=1,Type=String,Description=\"Type of structural variant\">\n"
        "##INFO=<ID=END,Number=1,Type=Integer,Description=\"The second pile of clipped reads (POS: the first)\">\n"
        "##INFO=<ID=SVLEN,Number=1,Type=Integer,Description=\"END - POS: bases inverted\">\n"
        "##INFO=<ID=CT,Number=1,Type=String,Description=\"Junction: 3to3, both piles of reads that stop aligning with a clip (the left junction), or 5to5, both of reads that start aligning with one (the right junction)\">\n"
        "##INFO=<ID=HOMLEN,Number=1,Type=Integer,Description=\"Bases by which the clipped reads continue behind the other breakpoint (micro-homology the aligner extended into, both piles together)\">\n"
        "##INFO=<ID=CR,Number=2,Type=Integer,Description=\"Clipped reads at POS, clipped reads at END\">\n"
        "##INFO=<ID=CN,Number=2,Type=Integer,Description=\"Of those, the reads whose clipped bases were kept, either pile\">\n"
        "##INFO=<ID=CV,Number=2,Type=Integer,Description=\"Of those, the reads whose clipped bases are the reverse complement of the reference at the other pile\">\n"
        "##inversion=\"a record per pair of positions POS < END, 50 <= END - POS <= 1000000, at both of which at least 3 reads of mapping quality >= -q stop aligning "
        "(CT=3to3) or at both of which such reads start aligning (CT=5to5) with a soft clip of at least 20 bases, more than at any of the 30 positions in front "
        "and no fewer than at any of the 30 behind, when for one shift s in 0 .. 32 at least 2 of the reads at POS and at least 2 of the reads at END "
        "continue with the complement of the reference running away from the other position, backwards from its base - 1 - s (3to3) or forwards from its "
        "base + s (5to5), in up to 32 clipped bases per read with at most 1 difference in 16 (HOMLEN: the s with the most such reads, the smallest among "
        "equals; CV: those reads); the two junctions of an inversion are two records; the file has no records once the clip-tail table has overflowed "
        "(stderr says so); POS 0 is skipped\"\n"
        "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\n")


def records_of(names, fasta, right, left, table):
    """([(contig, side, x, y, c1, c2, v1, v2, s, stored at x, stored at y)] the driver prints (POS 0 is skipped), candidates per side,
    peaks per side)"""
    out, n_cand, n_peaks = [], [0, 0], [0, 0]
    for tid, name in enumerate(names):
        pairs, n = inverted(right[tid], left[tid], table, fasta[name], tid, MIN_READS, REACH, MIN_LEN, MAX_LEN, MAX_SHIFT, MIN_VERIFIED)
        n_cand[0] += n[0]; n_cand[1] += n[1]
        n_peaks[0] += len(peaks_many(right[tid], MIN_READS, REACH)); n_peaks[1] += len(peaks_many(left[tid], MIN_READS, REACH))
        out += [(name,) + p for p in pairs if p[1] != 0]
    return out, tuple(n_cand), tuple(n_peaks)


def render(names, fasta, right, left, table):
    """FILE as the driver writes it, from the restatement"""
    lines = [header()]
    for name, side, x, y, c1, c2, v1, v2, s, n1, n2 in records_of(names, fasta, right, left, table)[0]:
        lines.append("%s\t%d\t.\t%s\t<INV>\t.\t.\tSVTYPE=INV;END=%d;SVLEN=%d;CT=%s;HOMLEN=%d;CR=%d,%d;CN=%d,%d;CV=%d,%d\n" % (
            name, x, fasta[name][x - 1:x].decode().upper(), y, y - x, "5to5" if side == LEFT else "3to3", s, c1, c2, n1, n2, v1, v2))
    return "".join(lines).encode()


def render_of_bam(bam, fasta_path, q):
    """(FILE, records, candidates per side, peaks per side) from BAM + FASTA at -q q"""
    names, right, left = cc.arrays_of_bam(bam, cc.MIN_CLIP, q)
    table = ct.table_of_bam(bam, cc.MIN_CLIP, q)[1]
    fasta = ct.read_fasta(fasta_path)
    return (render(names, fasta, right, left, table),) + records_of(names, fasta, right, left, table)


# ---------------------------------------------------------------------- the planted data set

# (a, length): an inversion of the bases [a, a + length).  Every 5 000 bases from 6 700 on, except where the simulator's own variants
# leave too few plain reads across a breakpoint (36 700 and 41 700): those two stand 500 and 1 000 further on, as in crossedpiles.
LENGTHS = [50, 60, 75, 100, 150, 300, 1_000, 3_000, 4_990]
STARTS = [6_700 + 5_000 * k for k in range(9)]
STARTS[6] += 500; STARTS[7] += 1_000
SITES = list(zip(STARTS, LENGTHS))


def planted_reads():
    """(refs, rd): the simulator's 60 kb contig at 30x with nine inversions planted into its reads.  At each site (a, n), b = a + n,
    first for (x, y) = (a, b), then for (b, a): of the mapped single-M reads with pos <= x - 25 and pos + 100 >= x + 25 (selected anew
    at each step), in arrival order j with k = x - pos, the 1st, 4th, ... become kM(100 - k)S and their clipped base t is
    comp(ref[y - 1 - t]); the 2nd, 5th, ... become kS(100 - k)M, start at x, and their head base at distance t from the junction is
    comp(ref[y + t]); every third stays.  The columns are sorted again, stably, by (tid, pos)."""
    from indelminer_amd import synth
    refs, rd = synth.simulate(seed=31, ref_len=60_000, coverage=30, n_contigs=1)
    ref = refs[0]
    lut = np.arange(256, dtype=np.uint8)
    for c, o in zip(b"ACGT", b"TGCA"):
        lut[c] = o
    comp = lut[np.asarray(ref, dtype=np.uint8)]
    L = rd.read_len
    for a, n in SITES:
        b = a + n
        for x, y in ((a, b), (b, a)):
            plain = (rd.ncig == 1) & (rd.cig_op[:, 0] == synth.OP_M) & ((rd.flag & 0x4) == 0)
            for j, i in enumerate(np.nonzero(plain & (rd.pos <= x - 25) & (rd.pos + L >= x + 25))[0]):
                k = x - int(rd.pos[i])
                if j % 3 == 0:
                    rd.cig_op[i, :2] = (synth.OP_M, synth.OP_S); rd.cig_len[i, :2] = (k, L - k); rd.ncig[i] = 2
                    rd.seq[i, k:] = comp[y - 1 - np.arange(L - k)]
                elif j % 3 == 1:
                    rd.cig_op[i, :2] = (synth.OP_S, synth.OP_M); rd.cig_len[i, :2] = (k, L - k); rd.ncig[i] = 2
                    rd.seq[i, k - 1 - np.arange(k)] = comp[y + np.arange(k)]
                    rd.pos[i] = x
    order = np.lexsort((rd.pos, rd.tid))                # stable
    for k, v in list(vars(rd).items()):
        if isinstance(v, np.ndarray) and len(v) == rd.n:
            setattr(rd, k, v[order])
    return refs, rd


def write_planted(d, refs, rd, lower_mapq_of_every_second_clipped_read=False):
    """ref.fa, aln.bam (+ .bai) and cfg.txt in directory d"""
    from tests.support import facingpiles
    return facingpiles.write_planted(d, refs, rd, lower_mapq_of_every_second_clipped_read)
