"""Realign inputs on SEVERAL resident contigs: six contigs whose lengths put the smallest and the largest pad of im_set_reference's
layout behind them, and reads that sit on, end at, or would run over a contig's first and last base.

The layout (im_capi.hip, im_set_reference): [256 zero bytes][contig 0][>= 64 zero bytes, next start 256-aligned][contig 1]...  The
2-bit copy packs a zero byte as 'A'.  A kernel that votes, scans or loads past clen therefore meets a run of 'A' in the packed copy
and, 64 bytes on at the least, the NEIGHBOUR's real bases in the ASCII copy.  On one random contig both are harmless; here they are not:

  indel            planted deletions / insertions as in tests/test_gpu_realign.py, on every contig that holds the read; half of them
                   within one read length of the contig's first or last base, anchors 0 and clen - 1 among them
  continue_right   the last a bases of contig i, then the first L - a bases of contig i + 1; tid = i.  On contig i alone there is
                   nothing to find; on the memory image (contig i, the pad, contig i + 1, read as ONE contig) it is a deletion of the pad
  continue_left    the same read with tid = i + 1
  a_run            the contig's last (or first) 40 .. 70 bases carried on with 'A', as the packed pad carries the contig on
  bad_tid          tid = -1 and tid = n_contigs

tests/test_contig_edges_host.py proves on the CPU oracle that the cases are what they claim; tests/test_gpu_realign_contigs.py
holds the kernels to the oracle on them.  Pure Python, seeded."""
import random

LENGTHS = [1472, 448, 2497, 300, 20160, 5000]
# pad bytes behind each contig but the last, by the layout rule: 192 mod 256 -> the minimum, 193 mod 256 -> the maximum
PADS = [64, 64, 319, 212, 64]
A_RUN = 24
ENDS_IN_A, BEGINS_WITH_A = (0, 3), (1, 4)
SEED = 20240
MAX_READS = 320
MARGIN = 82                 # a planted read of L bases with its deletion needs L + MARGIN bases of contig
FILLER = "N"                # the pad in a memory image: the k-mer code maps it to 0 as it maps a zero byte, and no read holds it

# name: (klength, numgaps, read lengths, range_max, maxdelsize)
BATCHES = {
    "a": (6, 0, (100, 128, 129, 200, 255), 700, 1000),      # specialised table, both lane layouts
    "b": (5, 0, (100, 200), 700, 1000),                     # direct table
    "c": (9, 0, (100, 200), 700, 1000),                     # prefix table
    "d": (14, 0, (100,), 700, 1000),                        # hash
    "e": (6, 2, (100, 250), 700, 1000),                     # band kernel
    "f": (6, 40, (100, 150), 700, 1000),                    # wide band
    "g": (6, 0, (256, 300, 1020, 100), 2500, 3000),         # long kernel beside the short one, windows of several histogram passes
    "h": (9, 0, (300, 100), 700, 1000),                     # long kernel, hash side
    "i": (6, 2, (300, 100), 700, 1000),                     # general pass beside the band kernel
    "j": (6, 0, (1100, 100), 2500, 3000),                   # general pass beside both laid-out kernels
    "k": (6, 61, (100,), 700, 1000),                        # general pass for every read
}


def pads(lengths):
    """bytes between the end of each contig and the start of the next, from the layout rule"""
    out, pos = [], 256
    for ln in lengths[:-1]:
        nxt = (pos + ln + 64 + 255) // 256 * 256
        out.append(nxt - (pos + ln))
        pos = nxt
    return out


_contigs = None


def contigs():
    """the six contigs (str), the same for every batch"""
    global _contigs
    if _contigs is None:
        assert pads(LENGTHS) == PADS, pads(LENGTHS)
        assert [ln % 256 for ln in LENGTHS[:3]] == [192, 192, 193] and LENGTHS[4] % 256 == 192
        rng = random.Random(SEED)
        out = []
        for t, ln in enumerate(LENGTHS):
            s = "".join(rng.choice("ACGT") for _ in range(ln))
            if t in ENDS_IN_A:
                s = s[:ln - A_RUN] + "A" * A_RUN
            if t in BEGINS_WITH_A:
                s = "A" * A_RUN + s[A_RUN:]
            out.append(s)
        _contigs = out
    return _contigs


def image(t):
    """contig t, its pad as filler, contig t + 1: what lies in device memory from contig t's first base on, read as one contig.
    Returns (sequence, position of contig t + 1's first base in it)."""
    c = contigs()
    return c[t] + FILLER * PADS[t] + c[t + 1], LENGTHS[t] + PADS[t]


def _noisy(rng, read, rate=0.005):
    return "".join((rng.choice("ACGT") if rng.random() < rate else ch) for ch in read)


def _indel_cases(rng, t, L, Rm, n):
    """n planted reads on contig t; every second one within L of the contig's first or last base"""
    contig = contigs()[t]
    clen = len(contig)
    out = []
    for j in range(n):
        d = rng.randint(1, 50)
        typ = rng.random()
        where = ("first", "last", "any", "any")[j % 4]
        last_start = clen - L - 51
        if where == "first":
            p = rng.choice([0, 0, rng.randint(0, min(L, last_start))])
        elif where == "last":
            # the read's last base this many bases in front of the contig's last
            p = None
            back = rng.choice([0, 0, rng.randint(0, min(L, last_start))])
        else:
            p = rng.randint(0, last_start)
        cut = rng.randint(12, L - 12)
        if typ < 0.5:           # deletion of d bases: the read spans L + d
            if p is None:
                p = clen - back - L - d
            read = contig[p:p + cut] + contig[p + cut + d:p + d + L]
            span = L + d
        elif typ < 0.9:         # insertion of up to 30 bases: the read spans L - d, or the part in front of the cut alone
            d = min(d, 30)
            span = max(cut, L - d)
            if p is None:
                p = clen - back - span
            read = (contig[p:p + cut] + "".join(rng.choice("ACGT") for _ in range(d)) + contig[p + cut:p + L])[:L]
        else:
            if p is None:
                p = clen - back - L
            read = contig[p:p + L]
            span = L
        assert 0 <= p and p + span <= clen and len(read) == L, (t, L, p, span, len(read))
        if where == "first" and j % 8 == 0:
            anchor = 0
        elif where == "last" and j % 8 == 1:
            anchor = clen - 1
        else:
            anchor = max(0, min(clen - 1, p + rng.randint(-Rm + 150, Rm - 50)))
        near_edge = p <= L or p + span >= clen - L
        out.append(dict(tid=t, anchor=anchor, range_max=Rm, read=_noisy(rng, read), kind="indel", near_edge=near_edge))
    return out


def _continue_cases(rng, t, L, Rm):
    """one read over the boundary t | t + 1, as continue_right (tid t) and as continue_left (tid t + 1)"""
    c = contigs()
    L = min(L, min(LENGTHS[t], LENGTHS[t + 1]) - 1)          # no read longer than the contig it is said to lie on
    a = rng.randint((L + 2) // 3, 2 * L // 3)
    read = c[t][LENGTHS[t] - a:] + c[t + 1][:L - a]
    assert len(read) == L
    right = dict(tid=t, anchor=max(0, LENGTHS[t] - rng.randint(100, 400)), range_max=Rm, read=read, kind="continue_right", own=a)
    left = dict(tid=t + 1, anchor=min(LENGTHS[t + 1] - 1, rng.randint(100, 400)), range_max=Rm, read=read, kind="continue_left", own=L - a)
    return [right, left]


def _a_run_cases(rng, t, L, Rm):
    contig = contigs()[t]
    clen = len(contig)
    m = rng.randint(40, 70)
    if t in ENDS_IN_A:
        read = contig[clen - m:] + "A" * (L - m)
        anchor = max(0, clen - rng.randint(1, 400))
    else:
        read = "A" * (L - m) + contig[:m]
        anchor = min(clen - 1, rng.randint(0, 400))
    return dict(tid=t, anchor=anchor, range_max=Rm, read=read, kind="a_run")


def _holds(t, L):
    """the length a planted read of L bases gets on contig t, or 0 when the contig takes none of that length"""
    clen = LENGTHS[t]
    if clen >= L + MARGIN:
        return L
    if L > 1020 or (t == 3 and L >= 300):
        return 0
    return clen - MARGIN


def params(name):
    k, g, _lengths, _Rm, maxdel = BATCHES[name]
    return dict(klength=k, numgaps=g, maxdelsize=maxdel, ethreshold=10)


_batches = {}


def batch(name):
    """the cases of one realign_batch call, shuffled: dict(tid, anchor, range_max, read, kind) each"""
    if name in _batches:
        return _batches[name]
    k, g, lengths, Rm, maxdel = BATCHES[name]
    rng = random.Random(SEED + 97 * (ord(name) - ord("a") + 1))
    nc = len(LENGTHS)
    cases = []
    for t in range(nc - 1):                  # 12 reads per boundary: 60 in all
        for j in range(6):
            cases += _continue_cases(rng, t, lengths[j % len(lengths)], Rm)
    for t in ENDS_IN_A + BEGINS_WITH_A:
        held = [x for x in (_holds(t, L) for L in lengths) if x]
        for j in range(4):
            cases.append(_a_run_cases(rng, t, held[j % len(held)], Rm))
    # bad_tid: one read of the batch's first length and one of its last.  In batches i and j the first is a length the laid-out
    # kernels pass on before they look at the contig index; the general pass used to leave such a read IM_ST_UNSUPPORTED.
    c0 = contigs()[0]
    cases.append(dict(tid=-1, anchor=500, range_max=Rm, read=c0[300:300 + lengths[0]], kind="bad_tid"))
    cases.append(dict(tid=nc, anchor=500, range_max=Rm, read=c0[300:300 + lengths[-1]], kind="bad_tid"))
    per_contig = (MAX_READS - len(cases)) // nc
    for t in range(nc):
        held = [x for x in (_holds(t, L) for L in lengths) if x]
        assert held, (name, t)
        for j, L in enumerate(held):
            cases += _indel_cases(rng, t, L, Rm, per_contig // len(held) + (1 if j < per_contig % len(held) else 0))
    assert len(cases) <= MAX_READS
    rng.shuffle(cases)
    indel = [c for c in cases if c["kind"] == "indel"]
    assert 3 * sum(c["near_edge"] for c in indel) >= len(indel)
    for t in range(nc):
        anchors = {c["anchor"] for c in indel if c["tid"] == t}
        assert 0 in anchors and LENGTHS[t] - 1 in anchors, (name, t)
    _batches[name] = cases
    return cases


def has_evidence(st, res):
    return st == 1 and res.n_ev > 0


_checked = {}


def checked(name):
    """(cases, want, dropped): the batch with the oracle's answer on each read's OWN contig beside it (None for bad_tid), computed
    once per process.  A continue_* read for which the own contig alone yields evidence (a chance match of the neighbour's bases)
    is dropped; dropped = how many were."""
    if name not in _checked:
        from tests.support import oraclebind as ob
        P = ob.params(**params(name))
        c = [s.encode() for s in contigs()]
        cases, want, dropped = [], [], 0
        for case in batch(name):
            if case["kind"] == "bad_tid":
                cases.append(case); want.append(None)
                continue
            t = case["tid"]
            st, res = ob.realign(P, c[t], len(c[t]), case["anchor"], case["range_max"], case["read"])
            if case["kind"].startswith("continue") and has_evidence(st, res):
                dropped += 1
                continue
            cases.append(case); want.append((st, res))
        _checked[name] = (cases, want, dropped)
    return _checked[name]


def evidence_per_contig(cases, has):
    """per contig the indel reads that came back with evidence; has[i]: whether case i did"""
    n = [0] * len(LENGTHS)
    for case, h in zip(cases, has):
        if case["kind"] == "indel" and h:
            n[case["tid"]] += 1
    return n


MIN_EVIDENCE = 5            # indel reads with evidence, per contig and batch


# ---- the pipeline runs of tests/test_gpu_realign_contigs.py::test_pipeline_paths_on_several_contigs ----
# (read length, numgaps, coverage): the long kernel behind the device-resident candidate count, and the band kernel
PIPELINE_REF_LENS = [20160, 1472 + 256 * 40, 5000]
PIPELINE_RUNS = [(300, 0, 30), (100, 2, 12)]


def pipeline_input(read_len, coverage):
    from indelminer_amd import synth
    return synth.simulate(seed=7, ref_lens=PIPELINE_REF_LENS, coverage=coverage, read_len=read_len, indel_spacing=700)
