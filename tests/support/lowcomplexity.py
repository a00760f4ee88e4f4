"""Low-complexity inputs: contigs that alternate random stretches with homopolymers and short tandem repeats, reads whose
indel sits inside such a repeat, and annotate-mode Smith-Waterman cases whose variant is a whole number of repeat units.
Real indels sit there, and the kernels' shortcuts behave differently there: most k-mers of a read piece are not unique
(no vote, tied diagonals, select_band's nearest-the-anchor rule), a deletion inside a repeat has a run of equally good cut
points (the reference's left/right placement), and equal-score paths are the norm for the band kernel's traceback, the
general pass and the forward-carried path statistics of the support kernel.

Pure Python, seeded; regenerated wherever the tests run.  The reference's answers are committed in
tests/golden/ref_lowcomplexity.json (tests/golden/make_golden_lowcomplexity.py)."""
import random

# periods 1 to 6
UNITS = ["A", "T", "C", "AC", "AG", "CT", "AT", "AAT", "ACG", "CAG", "TTTG", "GATA", "AAAAC", "AACCCT"]
DEL_SIZES = [1, 2, 3, 4, 6, 10, 50, 300]

GOLDEN_NAME = "ref_lowcomplexity.json"
# (k, g, seed) of the committed attempt_pe_alignment runs; k stops at 11 (tests/support/refcases.py)
REALIGN_RUNS = [(6, 0, 101), (5, 0, 102), (4, 0, 103), (7, 0, 104), (10, 0, 105), (11, 0, 106),
                (6, 1, 107), (6, 3, 108), (6, 5, 109), (6, 12, 110), (8, 1, 111), (8, 3, 112), (8, 5, 113), (8, 12, 114)]
SW_SEED, SW_N = 177, 300


def _random(rng, n):
    return "".join(rng.choice("ACGT") for _ in range(n))


def _run(unit, n, phase=0):
    return (unit * ((n + phase) // len(unit) + 2))[phase:phase + n]


def contig(rng, clen):
    """(sequence, repeats): random stretches of 20..120 bases alternating with repeat stretches of 8..90 bases whose units
    have periods 1 to 6, plus one homopolymer of at least 160 bases (longer than a read) and one dinucleotide run of at
    least 120, so that a whole read piece can lie inside a repeat.  repeats = [(start, stop, unit)], half-open."""
    at_homo = rng.randint(clen // 8, clen // 3)
    at_di = rng.randint(clen // 2, 3 * clen // 4)
    parts, repeats, n = [], [], 0
    while n < clen:
        s = _random(rng, rng.randint(20, 120))
        parts.append(s)
        n += len(s)
        if at_homo is not None and n >= at_homo:
            unit, ln, at_homo = rng.choice("ACT"), rng.randint(160, 200), None
        elif at_di is not None and n >= at_di:
            unit, ln, at_di = rng.choice(["AC", "AG", "CT", "AT"]), rng.randint(120, 160), None
        else:
            unit, ln = rng.choice(UNITS), rng.randint(8, 90)
        s = _run(unit, ln, rng.randrange(len(unit)))
        repeats.append((n, n + ln, unit))
        parts.append(s)
        n += ln
    seq = "".join(parts)[:clen]
    repeats = [(a, min(b, clen), u) for a, b, u in repeats if a < clen]
    return seq, repeats


def in_repeat(repeats, pos):
    """the repeat stretch that holds contig position `pos` or ends right in front of it (a cut at the stretch's edge), or None"""
    for a, b, u in repeats:
        if a <= pos <= b:
            return a, b, u
    return None


def realign_cases(seed, n=150, clen=6000, lengths=(76, 100, 100, 150), first=0, range_max=705):
    """(contig, [dict(anchor, range_max, read, in_repeat)], share): reads with one deletion (60 %, sizes of DEL_SIZES) or one
    insertion (half of them a copy of the bases just in front of the cut -- a repeat expansion -- and half random bases),
    30 % with one substitution, the read's start within +-700 of the anchor.  The cut point is drawn inside a repeat stretch
    for one read in five and anywhere for the rest, which puts about half of all cuts into repeats; share = the part of all
    reads whose cut lies inside or at the edge of one.  first = the lowest contig position any read or anchor touches."""
    rng = random.Random(seed)
    seq, repeats = contig(rng, clen)
    usable = [r for r in repeats if r[0] >= first + max(lengths) and r[1] <= clen - max(lengths) - max(DEL_SIZES) - 2]
    cases = []
    for _ in range(n):
        L = rng.choice(lengths)
        d = rng.choice(DEL_SIZES)
        cut = rng.randint(5, L - 5)
        if rng.random() < 0.2:
            a, b, _u = rng.choice(usable)
            at = rng.randint(a, b)
        else:
            at = rng.randint(first + cut, clen - 1)
        p = max(first, min(clen - L - d - 2, at - cut))
        at = p + cut
        anchor = max(first, min(clen - 1, p + rng.randint(-700, 700)))
        if rng.random() < 0.6:
            read = seq[p:at] + seq[at + d:at + d + (L - cut)]
        else:
            m = min(d, 30)
            ins = seq[max(0, at - m):at] if rng.random() < 0.5 else _random(rng, m)
            read = (seq[p:at] + ins + seq[at:p + L])[:L]
        if rng.random() < 0.3:
            i = rng.randrange(len(read))
            read = read[:i] + rng.choice("ACGT") + read[i + 1:]
        cases.append(dict(anchor=anchor, range_max=range_max, read=read, in_repeat=in_repeat(repeats, at) is not None))
    return seq, cases, sum(c["in_repeat"] for c in cases) / float(n)


def _event(rng, seq, repeats, lo, hi):
    """(vstart, size, is_del, inserted bases, in-repeat flag, period-multiple flag): an event whose base in front is the
    1-based position vstart in [lo, hi); inside or at the edge of a repeat stretch for 60 % of the draws, its size then a
    whole number of repeat units for two in three"""
    is_del = rng.random() < 0.5
    inside = [r for r in repeats if r[0] >= lo and r[1] < hi and r[1] - r[0] >= 2 * len(r[2])]
    size = rng.randint(1, 29)
    whole = False
    rep = None
    if inside and rng.random() < 0.6:
        rep = rng.choice(inside)
        a, b, u = rep
        vstart = rng.randint(a, b)
        if rng.random() < 0.67:
            size = len(u) * rng.randint(1, max(1, min(29 // len(u), (b - a) // len(u) - 1, 6)))
            whole = True
    else:
        vstart = rng.randint(lo, hi - 1)
        rep = in_repeat(repeats, vstart)
    ins = ""
    if not is_del:
        ins = seq[vstart - size:vstart] if (rep is not None and rng.random() < 0.75) or rng.random() < 0.5 else _random(rng, size)
    return vstart, size, is_del, ins, rep is not None, whole


def sw_cases(seed, n):
    """[dict] in the shape of sw_case (tests/golden/make_golden_units.py): a read against its own reference span widened by
    the indel, the way check_for_indel calls realign_with_indel (src/variant.c:1536-1546); the contig comes from contig(),
    cut down to the stretch around the span.  Two extra keys say how the case was drawn: in_repeat, whole_units."""
    rng = random.Random(seed)
    out = []
    seq, repeats = None, None
    for i in range(n):
        if i % 25 == 0:
            seq, repeats = contig(rng, 3000)
        vstart, size, is_del, ins, inrep, whole = _event(rng, seq, repeats, 200, len(seq) - 300)
        if is_del:
            vstop = vstart + size + 1
            alt = seq[vstart - 1:vstart]
            sample = seq[:vstart] + seq[vstart + size:]
        else:
            vstop = vstart
            alt = seq[vstart - 1:vstart] + ins
            sample = seq[:vstart] + ins + seq[vstart:]
        rl = rng.choice([76, 100, 150])
        # the read as the aligner placed it WITHOUT the indel: it starts left of the event on the reference
        pos = rng.randint(max(0, vstart - rl + 10), vstart - 6)
        # fewer reads carry the variant than in sw_case (38 % against 60 %) and more do not (50 % against 25 %): the window
        # holds the variant, so a carrying read aligns without a gap, and it is the other reads that put indels on the
        # path -- the statistic a repeat makes ambiguous.  110 of the 300 committed cases have indels; the tests ask for 100
        kind = rng.random()
        if kind < 0.38:
            read = sample[pos:pos + rl]                   # carries the variant
        elif kind < 0.88:
            read = seq[pos:pos + rl]                      # does not
        elif kind < 0.94:
            read = _random(rng, rl)
        else:
            read = _run(rng.choice(UNITS), rl)            # nothing but a repeat
        rate = rng.choice([0, 0.02, 0.08])
        read = "".join(rng.choice("ACGT") if rng.random() < rate else ch for ch in read)
        if rng.random() < 0.1:
            j = rng.randrange(len(read))
            read = read[:j] + "N" + read[j + 1:]
        qstart, qstop = rng.choice([0, 0, 5, 20]), len(read)
        rstart = max(0, pos - size)
        rstop = min(len(seq), pos + rl + size)
        base = max(0, rstart - 8)                         # the stretch of the contig the case keeps, coordinates re-based
        out.append(dict(contig=seq[base:rstop + 8], rstart=rstart - base, rstop=rstop - base, read=read, qstart=qstart, qstop=qstop,
                        is_deletion=int(is_del), vstart=vstart - base, vstop=vstop - base, alternate=alt,
                        in_repeat=int(inrep), whole_units=int(whole)))
    return out


def sw_inputs(c):
    """a case without the two keys that only describe how it was drawn"""
    return {k: v for k, v in c.items() if k not in ("in_repeat", "whole_units")}


def support_pairs(seed, shapes):
    """(targets, queries) as bytes for the support kernel: per (len1, len2) a target from contig() and a query of exactly
    len2 bases cut from it that carries a deletion or an expansion of a whole number of repeat units inside a repeat stretch;
    a query longer than what the target holds behind its start goes on with bases drawn the way contig() draws them"""
    rng = random.Random(seed)
    targets, queries = [], []
    for it, (len1, len2) in enumerate(shapes):
        seq, repeats = contig(rng, len1)
        cands = [r for r in repeats if r[1] - r[0] >= 3 * len(r[2]) and r[0] > 10 and r[1] < len1 - 10]
        a, b, u = rng.choice(cands)
        size = len(u) * rng.randint(1, max(1, min(4, (b - a) // len(u) - 1)))
        at = rng.randint(a + size, b)
        left = rng.randint(5, max(5, min(len2 - 10, at)))
        p = at - left
        if it % 2 == 0:
            q = seq[p:at] + seq[at + size:at + size + (len2 - left)]
        else:
            q = (seq[p:at] + seq[at - size:at] + seq[at:])[:len2]
        if len(q) < len2:                                 # the target ran out: go on as contig() would, past its end
            q += contig(rng, len2 - len(q) + 20)[0][:len2 - len(q)]
        targets.append(seq.encode())
        queries.append(q.encode())
    return targets, queries


def thin(ro):
    """a reference answer (tests/support/refcases.py: plain) as it is stored: segments without their bases, the shape
    golden.golden_vs_segments reads.  with_bases puts them back"""
    if ro is None or ro == "abort":
        return ro
    return [dict(e, aln1=[x[:4] for x in e["aln1"]], aln2=[x[:4] for x in e["aln2"]], aln3=[x[:4] for x in e["aln3"]]) for e in ro]


def with_bases(ro, read):
    """thin's inverse: a deletion's segment holds dashes, every other the read's bases from where the one before it ended
    (new_readseg, src/readaln.c:24-99); tests/golden/make_golden_lowcomplexity.py checks that this gives the reference's
    own strings back before it stores an answer"""
    if ro is None or ro == "abort":
        return ro
    out = []
    for e in ro:
        e, off = dict(e), 0
        for name in ("aln1", "aln2", "aln3"):
            segs = []
            for op, ln, start, end in e[name]:
                segs.append([op, ln, start, end, "-" * ln if op == 2 else read[off:off + ln]])
                off += 0 if op == 2 else ln
            e[name] = segs
        out.append(e)
    return out
