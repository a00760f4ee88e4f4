"""Reads at the bounds of the result record (IM_MAX_OPS = 64 segment words, IM_MAX_EV = 4 evidence records per read):
seeded generators, and a selector that runs candidates through the CPU oracle and keeps, per realign route, a fixed number
of reads in each CLASS -- an exact value of the oracle's n_ops or n_ev.  No GPU imports: tests/test_record_bounds_host.py
proves on the CPU that the batches are what they claim, tests/test_gpu_record_bounds.py runs them through the kernels.

The scoring is match +1, mismatch -10: a local alignment crosses a mismatch only with more than 10 matches on either side,
so a segment list grows by at most 2 words per ~12 read bases.  Uniform noise yields nothing: piece 2 starts behind the
FIRST '=' run of piece 1 (src/alignment.c:585-717), so with mismatches all over the larger piece the second band search
finds the first diagonal again.  The generators keep one stretch of the read clean for that reason.  A third generator
(plant_sites, even) gives the lists of even length -- 64 words exactly -- that the first two all but never do."""
import functools
import random

from . import oraclebind as ob

MAX_OPS, MAX_EV = 64, 4                 # include/indelminer_amd.h
IMO_OK, IMO_NONE, IMO_ABORT = 1, 0, -1  # oracle/im_oracle.h
ST_NONE, ST_EVIDENCE, ST_ABORT, ST_OVERFLOW = 0, 1, -1, -2
BIG = (("D", 30), ("D", 45), ("I", 20))


def _other(rng, ch):
    return rng.choice([c for c in "ACGT" if c != ch])


def _big_indel(rng, T, L, cut):
    """read of L bases from template T (T[0] is the read's first base) with one big indel at read offset cut"""
    typ, d = rng.choice(BIG)
    if typ == "D":
        return list(T[:cut] + T[cut + d:cut + d + (L - cut)])
    return list(T[:cut] + "".join(rng.choice("ACGT") for _ in range(d)) + T[cut:cut + (L - cut - d)])


def noisy(rng, T, L, sp):
    """generator 1: m clean bases at the read's start (m = 0.15 .. 0.25 L), the big indel at 0.46 .. 0.54 L, and from m on one
    substitution every sp + rand(0..3) bases to the other end"""
    m = int(L * rng.uniform(0.15, 0.25))
    read = _big_indel(rng, T, L, int(L * rng.uniform(0.46, 0.54)))
    x = m
    while x < L:
        read[x] = _other(rng, read[x])
        x += sp + rng.randint(0, 3)
    return "".join(read)


def stepped(rng, T, L, sp=0, k=0):
    """generator 2: the big indel at cut = 0.52 .. 0.6 L, the larger piece [0, cut) clean; one substitution every
    sp + rand(0..2) bases over [cut + 12, L - 14) (sp = 0: none), and k one-base indels spread evenly over [cut + 25, L - 25)"""
    cut = int(L * rng.uniform(0.52, 0.6))
    read = _big_indel(rng, T, L + k, cut)           # k spare bases for the one-base deletions
    if sp:
        x = cut + 12
        while x < L - 14:
            read[x] = _other(rng, read[x])
            x += sp + rng.randint(0, 2)
    lo, hi = cut + 25, L - 25
    for j in reversed(range(k)):                    # from the right, so that the offsets of the ones to come stay
        x = lo + int((j + 0.5) * (hi - lo) / k)
        if rng.random() < 0.5:
            del read[x]
        else:
            read.insert(x, _other(rng, read[x]))
    return "".join(read[:L])


HOMOLOGY = 22      # matches a local alignment needs in front of two mismatches to keep them (2 x -10)


def plant_sites(rng, contig, n, lo, hi):
    """For lists of EVEN length.  At numgaps == 0 a list is '=X..=', one D or I, '=X..=': odd, unless the second piece begins
    with an X.  The split point is the FIRST read offset with the most matches (find_best_del_candidate, src/alignment.c:306-339),
    so that takes a read offset where only the first piece matches, followed by one where neither does, both inside the second
    piece -- which keeps two mismatches only behind more than 20 matches.  A site is a deletion with that much microhomology:
    the HOMOLOGY bases in front of contig[s] copied in front of contig[s + d].  Returns (contig, [(s, d)])."""
    c = list(contig)
    sites = []
    for t in range(n):
        s = lo + (hi - lo) * t // n + rng.randint(0, 200)
        d = rng.choice((30, 45))
        c[s + d - HOMOLOGY:s + d] = c[s - HOMOLOGY:s]
        if c[s + d] == c[s]:
            c[s + d] = _other(rng, c[s])
        sites.append((s, d))
    return "".join(c), sites


def even(rng, T, L, sp, cut, d):
    """generator 3: generator 1 with its deletion (d bases at read offset cut) on a planted site.  Read base cut is the first
    piece's (contig[s]: a mismatch on the second piece's diagonal), base cut + 1 matches neither piece, and no other
    substitution comes near."""
    m = int(L * rng.uniform(0.15, 0.25))
    read = list(T[:cut] + T[cut + d:cut + d + (L - cut)])
    read[cut] = T[cut]
    read[cut + 1] = rng.choice([c for c in "ACGT" if c not in (T[cut + 1], T[cut + d + 1])])
    x = m
    while x < L:
        if not cut - HOMOLOGY - 2 <= x <= cut + HOMOLOGY + 2:
            read[x] = _other(rng, read[x])
        x += sp + rng.randint(0, 3)
    return "".join(read)


def ordinary(rng, T, L):
    """what the realign tests plant: one indel, no noise"""
    cut = rng.randint(14, L - 14)
    d = rng.randint(1, 40)
    if rng.random() < 0.5:
        return T[:cut] + T[cut + d:cut + d + (L - cut)]
    return (T[:cut] + "".join(rng.choice("ACGT") for _ in range(d)) + T[cut:])[:L]


def place(rng, contig, L, Rm, make, p=None):
    """One case: the read's stretch of the contig wholly on one side of the anchor and inside the first window, so that both
    pieces can be found (plan_piece2's four cases); for half of the cases the mirror image (template and read reversed).
    p: the read starts at contig[p], no mirror image."""
    span = L + 64
    clen = len(contig)
    fixed = p is not None
    if not fixed:
        p = rng.randint(Rm + 1200, clen - Rm - 1200 - span)
    gap = rng.randint(5, Rm - span - 20)
    anchor = p - gap if rng.random() < 0.5 else p + span + gap
    T = contig[p:p + span]
    if fixed or rng.random() < 0.5:
        read = make(rng, T, L)
    else:
        read = make(rng, T[::-1], L)[::-1]
    return dict(anchor=anchor, range_max=Rm, read=read)


PRODUCT_FLAGS = ["-i", "cfg.txt", "-f", "100"]       # -f: reads with some thirty substitutions count (the default allows 6 differences)


def product_dataset(dirpath):
    """ref.fa, aln.bam and cfg.txt of a simulated 2 x 1020 library in which THREE realign candidates with neighbouring anchors
    carry reads of generator 1's shape with the same 45-base deletion: one whose segment list has 65 words (one more than the
    result record holds) and two whose lists fit, so that the deletion is a variant the reference prints -- with three
    supporting reads.  tests/golden/vcf/record_bounds_65_segments.vcf is what the reference prints
    (tests/golden/make_golden_record_bounds.py).  Returns (the oracle's Info of the three reads, the deletion's 0-based start)."""
    import os
    import numpy as np
    from indelminer_amd import bamwrite, synth
    L, isz, d, sp = 1020, 3060, 45, 25
    Rm = isz + 200
    refs, rd = synth.simulate(seed=21, ref_len=60_000, coverage=12, read_len=L, isize_mean=isz, isize_min=isz - 200, isize_max=isz + 200)
    cand = synth.candidates(rd)
    contig = refs[0].tobytes().decode()
    cbytes = contig.encode()
    # FR proper pairs (their bases go to the realignment as stored) with anchors in the middle of the contig, 1500 bases apart at most
    ok = [j for j in range(len(cand["index"])) if 20_000 < cand["anchor"][j] < 40_000 and (int(rd.flag[cand["index"][j]]) & 0x33) in (0x13, 0x23)]
    ok.sort(key=lambda j: int(cand["anchor"][j]))
    three = next(ok[t:t + 3] for t in range(len(ok) - 2) if int(cand["anchor"][ok[t + 2]]) - int(cand["anchor"][ok[t]]) <= 1500)
    anchors = [int(cand["anchor"][j]) for j in three]
    p, cut = anchors[2] + 40, L // 2                    # right of all three anchors, inside all three first windows
    assert p + L + d + 64 < anchors[0] + Rm
    T = contig[p:p + L + d + 64]
    rng = random.Random(65)
    P = ob.params(klength=6, numgaps=0)
    wanted = [lambda x: x.n_ops == MAX_OPS + 1, lambda x: x.n_ops == MAX_OPS - 1, lambda x: x.n_ops == MAX_OPS - 3]
    infos = []
    rd.seq = rd.seq.copy()
    for j, anchor, pred in zip(three, anchors, wanted):
        for _ in range(3000):
            read = list(T[:cut] + T[cut + d:cut + d + (L - cut)])
            x = int(L * rng.uniform(0.15, 0.25))
            while x < L:
                read[x] = _other(rng, read[x])
                x += sp + rng.randint(0, 3)
            read = "".join(read)
            info = Info(P, cbytes, dict(anchor=anchor, range_max=Rm, read=read))
            if info.st == IMO_OK and info.n_ev == 1 and pred(info) and info.res.ev[0].b2 - info.res.ev[0].b1 == d and \
                    (not infos or (info.res.ev[0].b1, info.res.ev[0].b2) == (infos[0].res.ev[0].b1, infos[0].res.ev[0].b2)):
                break
        else:
            raise AssertionError("no read in 3000 tries")
        infos.append(info)
        rd.seq[int(cand["index"][j])] = np.frombuffer(read.encode(), np.uint8)
    contigs = [("ctg0", len(refs[0]))]
    bamwrite.write_fasta(os.path.join(dirpath, "ref.fa"), contigs, refs)
    bamwrite.write_bam(os.path.join(dirpath, "aln.bam"), contigs, rd)
    with open(os.path.join(dirpath, "cfg.txt"), "w") as fh:
        fh.write("IL generic %d %d\n" % (isz - 200, Rm))
    return infos, infos[0].res.ev[0].b1         # p + cut, give or take the bases that match on either side of the deletion


class Info:
    """the oracle's answer for one case, reduced to what the rule and the classes look at"""

    def __init__(self, P, contig, case):
        st, res = ob.realign(P, contig, len(contig), case["anchor"], case["range_max"], case["read"])
        self.st, self.res = st, res
        ok = st == IMO_OK
        self.L = len(case["read"])
        self.n_ops = res.n_ops if ok else 0
        self.n_ev = res.n_ev if ok else 0
        self.piece_ops = max(res.piece[0].n_ops, res.piece[1].n_ops) if ok else 0
        self.overflow = ok and (self.n_ops > MAX_OPS or self.n_ev > MAX_EV)
        self.fits = ok and not self.overflow
        self.ambiguous = self.fits and self.piece_ops > MAX_OPS       # the final list fits, a piece's CIGAR does not
        self.usable = st in (IMO_OK, IMO_NONE) and not self.ambiguous


def shim_status(info, max_ops=MAX_OPS, max_ev=MAX_EV):
    """the CPU shim's rule (tests/shim/im_shim.c, im_realign_batch) restated; the two bounds are arguments so that the host
    test can show that an off-by-one variant does not pass"""
    st = info.st
    if st != IMO_OK:
        return ST_NONE if st == IMO_NONE else ST_ABORT if st == IMO_ABORT else ST_OVERFLOW
    return ST_OVERFLOW if (info.res.n_ops > max_ops or info.res.n_ev > max_ev) else ST_EVIDENCE


# ---- the routes ------------------------------------------------------------------------------------------------------
#
# sources: (generator name, its keywords, (shortest, longest read), candidates); "even" takes its cut and its site from select()
# classes: (label, predicate over Info, reads wanted, reads that must be found)

def _ops(n):
    return ("n_ops=%d" % n, lambda i, n=n: i.n_ops == n and i.n_ev <= MAX_EV, 3, 3)


def _ev(n):
    return ("n_ev=%d" % n, lambda i, n=n: i.n_ev == n and i.n_ops <= MAX_OPS, 3, 3)


def _route(kernel, kw, sources, classes, ordinary_lengths, Rm, reaches, clen=70000):
    """reaches: the bounds the route's candidates get beyond, "ops" and / or "ev" """
    return dict(kernel=kernel, kw=kw, sources=sources, classes=classes, ordinary_lengths=ordinary_lengths, Rm=Rm, clen=clen,
                reaches=reaches)


# the indel bound on reads of up to 255 bases; the last two sources are there for the densest list such reads give
_EV_SOURCES_255 = [("stepped", dict(k=k), (235, 255), n) for k, n in ((1, 60), (2, 60), (3, 80), (4, 500))] + [
    ("stepped", dict(sp=12), (236, 255), 400), ("noisy", dict(sp=12), (236, 255), 400)]

ROUTES = {
    # realign_kernel: the segment bound is out of reach (the host test asserts the densest list found), n_ev is always 1
    "short": _route("realign_kernel", dict(klength=6, numgaps=0),
                    [("noisy", dict(sp=12), (236, 255), 300), ("noisy", dict(sp=14), (236, 255), 700), ("noisy", dict(sp=15), (236, 255), 500),
                     ("noisy", dict(sp=12), (110, 128), 300), ("noisy", dict(sp=15), (110, 128), 800), ("noisy", dict(sp=14), (110, 128), 500)],
                    [("dense, L near 255", lambda i: i.L > 128 and i.fits and i.n_ops >= 21, 10, 10),
                     ("dense, L near 128", lambda i: i.L <= 128 and i.fits and i.n_ops >= 11, 10, 10)],
                    [100, 128, 129, 200, 255], 705, ""),
    "long_k6": _route("realign_long_kernel", dict(klength=6, numgaps=0),
                      [("noisy", dict(sp=25), (1020, 1020), 300), ("noisy", dict(sp=15), (580, 600), 300),
                       ("noisy", dict(sp=12), (450, 480), 300), ("noisy", dict(sp=25), (1000, 1020), 900),
                       ("even", dict(sp=25), (1000, 1020), 200)],
                      [_ops(59), _ops(61), _ops(63), _ops(65), _ops(67), _ops(62), _ops(64), _ops(66)],
                      [450, 600, 1020, 1020, 300], 1500, "ops"),
    "long_k9": _route("realign_long_kernel", dict(klength=9, numgaps=0),
                      [("noisy", dict(sp=25), (1020, 1020), 300), ("noisy", dict(sp=15), (580, 600), 300),
                       ("noisy", dict(sp=25), (1000, 1020), 900), ("even", dict(sp=25), (1000, 1020), 200)],
                      [_ops(59), _ops(61), _ops(63), _ops(65), _ops(67), _ops(62), _ops(64), _ops(66)],
                      [450, 600, 1020, 1020, 300], 1500, "ops"),
    "band_g2": _route("realign_band_kernel", dict(klength=6, numgaps=2), _EV_SOURCES_255,
                      [_ev(2), _ev(3), _ev(4), _ev(5)], [100, 150, 255], 705, "ev"),
    "band_g8": _route("realign_band_kernel", dict(klength=6, numgaps=8), _EV_SOURCES_255,
                      [_ev(2), _ev(3), _ev(4), _ev(5)], [100, 150, 255], 705, "ev"),
    "band_g60": _route("realign_band_kernel", dict(klength=6, numgaps=60), _EV_SOURCES_255,
                       [_ev(2), _ev(3), _ev(4), _ev(5)], [100, 150, 255], 705, "ev"),
    "any_g0": _route("realign_any_kernel", dict(klength=6, numgaps=0),
                     [("noisy", dict(sp=35), (1380, 1400), 500), ("noisy", dict(sp=25), (1021, 1060), 300),
                      ("noisy", dict(sp=37), (1480, 1500), 300), ("even", dict(sp=35), (1380, 1400), 200)],
                     [_ops(61), _ops(63), _ops(65), _ops(67), _ops(62), _ops(64), _ops(66)], [1021, 1200, 1500, 100, 300], 2000, "ops", clen=80000),
    "any_g3": _route("realign_any_kernel", dict(klength=6, numgaps=3),
                     [("stepped", dict(sp=12), (980, 1000), 500), ("stepped", dict(sp=13), (880, 900), 300),
                      ("stepped", dict(sp=12, k=1), (880, 1000), 500), ("stepped", dict(sp=10), (700, 760), 300)],
                     [_ops(61), _ops(63), _ops(65), _ops(69),
                      ("n_ev=2 at n_ops>=60", lambda i: i.n_ev == 2 and 60 <= i.n_ops <= MAX_OPS, 3, 3)],
                     [700, 900, 1000, 150, 300], 1500, "ops"),
    "any_g8": _route("realign_any_kernel", dict(klength=6, numgaps=8),
                     [("stepped", dict(k=k), (480, 500), n) for k, n in ((1, 30), (2, 30), (3, 40), (4, 60), (5, 300))],
                     [_ev(2), _ev(3), _ev(4), _ev(5), _ev(6)], [500, 400, 300, 150], 1000, "ev"),
    "any_g61": _route("realign_any_kernel", dict(klength=6, numgaps=61), _EV_SOURCES_255,
                      [_ev(2), _ev(3), _ev(4), _ev(5)], [100, 150, 255], 705, "ev"),
}

GENERATORS = dict(noisy=noisy, stepped=stepped)


class Batch:
    """contig (bytes), kw (the run's parameters), cases (dicts: anchor, range_max, read, label -- None for an ordinary read),
    info (the oracle's answer per case), counts (reads per class), n_candidates, rejected_ambiguous, densest (the longest
    fitting or overflowing list among ALL candidates, chosen or not) and densest_ev."""


@functools.lru_cache(maxsize=None)
def select(name):
    """The batch of route `name`: per class the first reads the seeded candidates give, shuffled among about as many ordinary
    reads; where the route has overflow classes, one overflow read is the batch's first read and another its last."""
    R = ROUTES[name]
    rng = random.Random("recordbounds " + name)
    contig = "".join(rng.choice("ACGT") for _ in range(R["clen"]))
    contig, sites = plant_sites(rng, contig, 8, R["Rm"] + 3000, R["clen"] - R["Rm"] - 4500)
    cbytes = contig.encode()
    P = ob.params(**R["kw"])
    B = Batch()
    B.name, B.kernel, B.kw, B.contig = name, R["kernel"], dict(R["kw"]), cbytes
    B.counts = {c[0]: 0 for c in R["classes"]}
    B.n_candidates = B.rejected_ambiguous = B.densest = B.densest_ev = B.with_evidence = 0
    chosen = []
    for gen, gkw, (lmin, lmax), n_cand in R["sources"]:
        for _ in range(n_cand):
            L = rng.randint(lmin, lmax)
            if gen == "even":
                (site, d), cut = rng.choice(sites), int(L * rng.uniform(0.46, 0.54))
                case = place(rng, contig, L, R["Rm"], functools.partial(even, cut=cut, d=d, **gkw), p=site - cut)
            else:
                case = place(rng, contig, L, R["Rm"], functools.partial(GENERATORS[gen], **gkw))
            info = Info(P, cbytes, case)
            B.n_candidates += 1
            B.with_evidence += info.st == IMO_OK
            B.densest = max(B.densest, info.n_ops)
            B.densest_ev = max(B.densest_ev, info.n_ev)
            if info.ambiguous:
                B.rejected_ambiguous += 1
            if info.st != IMO_OK or not info.usable:
                continue
            for label, pred, want, _ in R["classes"]:
                if B.counts[label] < want and pred(info):
                    B.counts[label] += 1
                    chosen.append((dict(case, label=label), info))
                    break
    n_ord = max(len(chosen), 100 - len(chosen))
    plain = []
    while len(plain) < n_ord:
        case = place(rng, contig, rng.choice(R["ordinary_lengths"]), R["Rm"], ordinary)
        info = Info(P, cbytes, case)
        if info.usable and not info.overflow:
            plain.append((dict(case, label=None), info))
    both = chosen + plain
    rng.shuffle(both)
    over = [j for j, (_, i) in enumerate(both) if i.overflow]
    if len(over) >= 2:
        both[0], both[over[0]] = both[over[0]], both[0]
        both[-1], both[over[-1]] = both[over[-1]], both[-1]
    B.cases = [c for c, _ in both]
    B.info = [i for _, i in both]
    B.missing = {c[0]: (B.counts[c[0]], c[3]) for c in R["classes"] if B.counts[c[0]] < c[3]}
    B.reaches = R["reaches"]
    return B


def report(B):
    """one line for assertion messages: class counts, the ambiguous-read count, the densest list over all candidates"""
    return ("%s (%s, %r): %d candidates, %d with evidence, classes %r, ambiguous rejected %d, ambiguous chosen %d, densest list "
            "%d segments, most indels %d, batch of %d reads"
            % (B.name, B.kernel, B.kw, B.n_candidates, B.with_evidence, B.counts, B.rejected_ambiguous,
               sum(i.ambiguous for i in B.info), B.densest, B.densest_ev, len(B.cases)))
