"""Inputs with one locus deeper than samtools' pileup buffers (bam_pileup.c:172,244: 8000 nodes): a small simulated contig in
which one plain proper pair (no indel, no clip: no evidence, trivial for the reference) that ends inside the DP= range of a
called deletion is present `depth` times over (same positions, own names).  DP= of that deletion comes from a pileup that stops
taking the records that start at the stack's position once its buffer is full -- the reference prints a smaller DP= than a plain
depth count gives.

INPUTS names every geometry the suite holds (goldens: tests/golden/vcf/<name>.vcf, made by make_golden_deep.py from the compiled
reference).  With b1 = the first deleted base of the called deletion and L = the read length, the DP= window of that deletion is
[b1 - lw - 1, b2 + rw + 1) (lw, rw: the deletion's wiggle), and the stacked first mates cover [b1 - L + shift, b1 + shift):

  deep_locus_9000 / _7900   shift 0: the stack ends exactly on the window's first base (the two inputs of the first deep-locus test)
  boundary_7998 .. _8001    the same geometry, at another deletion of the contig, around the depth at which the push rule (pool count
                            > 8000) first binds: the deletion is the one where a single refused record changes the printed floor
  stack_inside              the stack STARTS inside the window: the iterator stands at or after the window's first base
  stack_in_front            the stack starts 60 bases in front of b1 and reaches the window with its tail; 60 more plain pairs start on
                            ONE position inside the stack's span and cover the window (they meet the full buffer, too)
  stack_contig1             the same stack on the second of two contigs (the iterator starts out on contig 0, position 0)
  stack_pos0                the stack at position 0 of contig 0: the position the iterator starts out on
  stack_on_piece_edge       the stack lies across base 16384, where the walkers' pieces are cut: its records belong to one piece, the
                            depth they add reaches into the next
  stack_flagged             9000 stacked pairs, 1000 of them duplicates (0x400), 1000 secondary (0x100): the pileup skips those before
                            they take a node, 7000 remain, nothing is refused
  staggered_9000            a depth of 9000 at the window's first base from unpaired records whose starts all differ
                            (50M <k>D 50M, all ending at b1): every record is taken
  stack_spanning_d          8100 unpaired 40M160D60M records at one position, the window inside their D: no M/=/X depth in the
                            window, 8100 pileup nodes over it; 60 plain pairs on one position cover the window
  spanning_d_long_deletion  the same beside a planted deletion of 50 bases, the shortest that carries the product's own DM= (-D)
The unpaired records (flag 0, mapping quality 0) are turned away by the reference's fetch_func at once (is_se) and are no
realignment candidates; the pileup counts them all the same."""
import numpy as np

from indelminer_amd import synth

COLS = ("tid", "pos", "flag", "mpos", "isize", "seq", "cig_op", "cig_len", "ncig", "mate_first", "pair_id")

# the boundary inputs: the deletion of the simulated contig at which ONE refused record shows in the printed mean (DP= is a floor over
# the window's bases, the stack covers one of them: at most deletions a few refused records change nothing that is printed)
BOUNDARY_WHICH = 47

PIECE_EDGE = 16384               # the walkers' pieces are cut at the BAM index's 16 KiB windows (hostio.c, bai_split_points)

INPUTS = {
    "deep_locus_9000": dict(depth=9000),
    "deep_locus_7900": dict(depth=7900),
    "boundary_7998": dict(depth=7998, which=BOUNDARY_WHICH),
    "boundary_7999": dict(depth=7999, which=BOUNDARY_WHICH),
    "boundary_8000": dict(depth=8000, which=BOUNDARY_WHICH),
    "boundary_8001": dict(depth=8001, which=BOUNDARY_WHICH),
    "stack_inside": dict(depth=9000, shift=101),
    "stack_in_front": dict(depth=9000, shift=40, pile=60, pile_shift=70),
    "stack_contig1": dict(depth=9000, n_contigs=2, contig=1),
    "stack_pos0": dict(depth=9000, deletion_at=100),
    "stack_on_piece_edge": dict(depth=9000, deletion_at=PIECE_EDGE + 16),
    "stack_flagged": dict(depth=9000, flagged=((0, 9, 0x400), (1, 9, 0x100))),
    "staggered_9000": dict(depth=0, staggered=9000, min_pos=12_000),
    "stack_spanning_d": dict(depth=0, spanning_d=8100, pile=60, pile_shift=70),
    "spanning_d_long_deletion": dict(depth=0, spanning_d=8100, pile=60, pile_shift=70, deletion_at=20_000, deletion_size=50),
}

# the inputs that run on every route (tests/test_deep_locus_routes.py); each has two more goldens: <name>_five_indels (the input with
# one read of five indels planted far from the stack: the pipelined product hands such a run to its record-at-a-time child) and
# <name>_region (the input under -c region_flags(where))
ROUTE_INPUTS = ("deep_locus_9000", "stack_in_front", "stack_contig1")
# 100 read bases with five indels that pass check_variants' end-distance rule: 16M 1I 16M 2D 16M 1I 16M 2D 16M 1I 17M
FIVE_INDELS = [(0, 16), (1, 1), (0, 16), (2, 2), (0, 16), (1, 1), (0, 16), (2, 2), (0, 16), (1, 1), (0, 17)]


def region_flags(where):
    """-c around the stack: 2000 bases to either side of the deletion"""
    return ["-c", "ctg%d:%d-%d" % (where["contig"], max(1, where["deletion_start"] - 2000), where["deletion_start"] + 2000)]

def _events_with(seed, ref_len, at, size):
    """deletion_at: the planted indels of a plain simulation (their own stream), and among them one deletion of `size` bases whose first
    deleted base is `at` (stack_pos0: base 100, the base behind a stack at position 0); planted indels within 500 bases of it go"""
    pos, sz, is_ins = synth.plant_indels(np.random.default_rng(seed + 1), ref_len)
    far = np.abs(pos - at) > 500
    pos, sz, is_ins = np.concatenate([[at], pos[far]]), np.concatenate([[size], sz[far]]), np.concatenate([[False], is_ins[far]])
    o = np.argsort(pos, kind="stable")
    return pos[o], sz[o], is_ins[o]


def make(seed=71, depth=9000, ref_len=40_000, coverage=20, n_contigs=1, contig=0, shift=0, deletion_at=None, deletion_size=12, min_pos=5000, which=3,
         pile=0, pile_shift=0, flagged=(), stack_mapq=None, staggered=0, spanning_d=0, five_indels=False):
    """refs, reads, where.  which: the deletion-carrying record, counted along the contig from min_pos on, whose deletion is the one
    (deletion_at: a deletion planted with its first deleted base there, in place of a choice).  depth: plain pairs stacked so that the first mates cover [b1 - L + shift, b1 + shift) on `contig`.
    pile, pile_shift: that many more of the same pair at shift pile_shift.  flagged: (first, every, flag bits) -- the stacked pairs
    first, first + every, ... carry those bits on both mates.  stack_mapq: the mapping quality of the stacked rows (default: the
    data set's).  staggered / spanning_d: that many unpaired records (flag 0, mapping quality 0) as the module's text describes.
    five_indels: one plain read of a proper pair, 20 000 bases and more from the deletion, gets the CIGAR FIVE_INDELS."""
    events = _events_with(seed, ref_len, deletion_at, deletion_size) if deletion_at is not None else None
    refs, rd = synth.simulate(seed=seed, ref_len=ref_len, coverage=coverage, n_contigs=n_contigs, events=events)
    L = rd.read_len
    # a deletion that reads carry in their CIGARs: 50M <d>D 50M-like records; its start on the contig
    has_d = ((rd.flag & 0x2) != 0) & (rd.ncig == 3) & (rd.cig_op[:, 1] == synth.OP_D) & (rd.tid == contig)
    if deletion_at is not None:
        k = int(np.nonzero(has_d & (rd.pos + rd.cig_len[:, 0] == deletion_at))[0][0])
    else:
        k = int(np.nonzero(has_d & (rd.pos > min_pos) & (rd.pos < ref_len - 5000))[0][which])
    b1 = int(rd.pos[k]) + int(rd.cig_len[k, 0])
    # a plain forward first mate (100M, proper pair, both mates plain) from anywhere, moved so that it ENDS at the deletion's start:
    # it covers the base in front of the deletion, the first base of the DP= range (plain reads are not realigned, their bases
    # are never compared with the reference)
    plain = ((rd.flag & 0x2) != 0) & (rd.ncig == 1) & (rd.cig_op[:, 0] == synth.OP_M) & ((rd.flag & 0x10) == 0) & (rd.pos < rd.mpos)
    i = None
    for c in np.nonzero(plain)[0]:
        j = [int(x) for x in np.nonzero(rd.pair_id == rd.pair_id[c])[0] if int(x) != int(c)]
        if len(j) == 1 and rd.ncig[j[0]] == 1 and rd.cig_op[j[0], 0] == synth.OP_M:
            i, j = int(c), j[0]
            break
    assert i is not None
    if five_indels:
        width = len(FIVE_INDELS)
        op = np.zeros((rd.n, width), dtype=rd.cig_op.dtype); ln = np.zeros((rd.n, width), dtype=rd.cig_len.dtype)
        op[:, :rd.cig_op.shape[1]] = rd.cig_op; ln[:, :rd.cig_len.shape[1]] = rd.cig_len
        far = (rd.tid == contig) & ((rd.flag & 0x3) == 0x3) & (rd.ncig == 1) & (np.abs(rd.pos - b1) > 20_000) & (rd.pos > 1000) & (rd.pos < ref_len - 1000)
        r5 = int(np.nonzero(far)[0][7])
        assert r5 not in (i, j) and sum(l for o, l in FIVE_INDELS if o != synth.OP_D) == L
        for s5, (o, l) in enumerate(FIVE_INDELS):
            op[r5, s5] = o; ln[r5, s5] = l
        rd.cig_op, rd.cig_len = op, ln
        rd.ncig = rd.ncig.copy(); rd.ncig[r5] = width
    add = {c: [] for c in COLS}
    add_mapq = []
    next_id = int(rd.pair_id.max()) + 1
    where = dict(deletion_start=b1, contig=contig)

    def stack_pairs(count, delta):
        nonlocal next_id
        rep = np.tile(np.array([i, j], dtype=np.int64), count)
        for c in COLS:
            col = getattr(rd, c)
            new = col[rep] if c != "pair_id" else next_id + np.repeat(np.arange(count, dtype=rd.pair_id.dtype), 2)
            if c in ("pos", "mpos"):
                new = new + delta
            if c == "tid":
                new = np.full(len(rep), contig, dtype=col.dtype)
            add[c].append(new)
        next_id += count
        return int(rd.pos[i]) + delta, int(rd.pos[j]) + delta

    def unpaired(starts, ops):
        """one record per start: flag 0, mapping quality 0, the bases of the plain first mate; ops[k] = its (op, length) list"""
        nonlocal next_id
        n = len(starts)
        op = np.zeros((n, rd.cig_op.shape[1]), dtype=rd.cig_op.dtype); ln = np.zeros((n, rd.cig_len.shape[1]), dtype=rd.cig_len.dtype)
        for r, row in enumerate(ops):
            for s, (o, l) in enumerate(row):
                op[r, s] = o; ln[r, s] = l
        new = dict(tid=np.full(n, contig, rd.tid.dtype), pos=np.asarray(starts, rd.pos.dtype), flag=np.zeros(n, rd.flag.dtype),
                   mpos=np.asarray(starts, rd.mpos.dtype), isize=np.zeros(n, rd.isize.dtype), seq=np.tile(rd.seq[i], (n, 1)), cig_op=op, cig_len=ln,
                   ncig=np.array([len(row) for row in ops], rd.ncig.dtype), mate_first=np.ones(n, rd.mate_first.dtype),
                   pair_id=next_id + np.arange(n, dtype=rd.pair_id.dtype))
        for c in COLS:
            add[c].append(new[c])
        add_mapq.append(np.zeros(n, np.int64))
        next_id += n

    if depth:
        delta = b1 - L + shift - int(rd.pos[i])
        where["stack_at"] = stack_pairs(depth, delta)
        flags = add["flag"][-1] = add["flag"][-1].copy()
        for first, every, bits in flagged:
            sel = np.arange(first, depth, every)
            flags[2 * sel] |= bits; flags[2 * sel + 1] |= bits
        add_mapq.append(np.full(2 * depth, rd.mapq if stack_mapq is None else stack_mapq, np.int64))
    if staggered:
        # record k: 50M <x>D 50M ending at b1; x grows with k, so every start differs -- and none is the start of a simulated record
        taken = set(int(p) for p in rd.pos[rd.tid == contig])
        starts = []
        s = b1 - L - 1
        while len(starts) < staggered:
            if s not in taken:
                starts.append(s)
            s -= 1
        assert s >= 0
        starts = starts[::-1]
        unpaired(starts, [[(synth.OP_M, L // 2), (synth.OP_D, b1 - L - s0), (synth.OP_M, L - L // 2)] for s0 in starts])
        where["staggered_from"] = starts[0]
    if spanning_d:
        unpaired([b1 - L] * spanning_d, [[(synth.OP_M, 40), (synth.OP_D, 160), (synth.OP_M, 60)]] * spanning_d)
        where["spanning_at"] = b1 - L
    if pile:
        where["pile_at"] = stack_pairs(pile, b1 - L + pile_shift - int(rd.pos[i]))
        add_mapq.append(np.full(2 * pile, rd.mapq, np.int64))
    out = synth.Reads()
    for c in COLS:
        setattr(out, c, np.concatenate([getattr(rd, c)] + add[c]))
    mapq = np.concatenate([np.full(rd.n, rd.mapq, np.int64)] + add_mapq)
    order = np.lexsort((np.arange(len(out.pos)), out.pos, out.tid))       # coordinate order, earlier rows first among equals
    for c in COLS:
        setattr(out, c, getattr(out, c)[order])
    out.n = len(out.pos)
    out.read_len = rd.read_len; out.range_max = rd.range_max
    out.mapq = rd.mapq if (mapq == rd.mapq).all() else mapq[order]          # one value for the data set, or one per row (rawrec.build)
    return refs, out, where


def write(td, **kw):
    from indelminer_amd import bamwrite, rawrec
    refs, rd, where = make(**kw)
    contigs = [("ctg%d" % k, len(r)) for k, r in enumerate(refs)]
    bamwrite.write_fasta(td + "/ref.fa", contigs, refs)
    rawrec.write_bam_fast(td + "/aln.bam", contigs, rd)
    open(td + "/cfg.txt", "w").write("IL generic 300 %d\n" % rd.range_max)
    return rd.n, where
