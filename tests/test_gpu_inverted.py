"""Inversion breakpoints from same-side clip piles (-N): the candidate enumeration and verification of im_cliptail.hip's
cliptail_pairs_kernel<true> behind im_clip_inverted_tid / im_clip_inverted, and what the host driver makes of them (-N FILE).

The yardstick is the plain restatement in tests/support/invertedpiles.py, written from the definition in include/indelminer_amd.h (seam 5,
"Inverted piles"), not from the code under test; tests/test_inverted_host.py pins it to cases worked by hand.  Every answer is compared
exactly.
"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests.support import clipcounts as cc
from tests.support import cliptails as ct
from tests.support import invertedpiles as ip
from tests.support.clipcounts import LEFT, RIGHT
from tests.support.spanarrays import _product
from tests.test_gpu_facing import CLENS, Device, contigs, empty_arrays

pytestmark = pytest.mark.gpu

PAR = (3, 30, 50, 400, 32, 2)       # m, T, dmin, dmax, S, mv of the hand-made cases: the sites stand 1 000 apart, no site sees another's piles


def comp_codes(ref, start, n, step=1):
    """n 2-bit codes of comp(ref[start]), comp(ref[start + step]), ...; A where there is no base"""
    return tuple(3 - b"ACGT".index(ref[p:p + 1]) if 0 <= p < len(ref) and ref[p:p + 1] in (b"A", b"C", b"G", b"T") else 0 for p in (start + step * i for i in range(n)))


def rows(got):
    return None if got is None else [tuple(int(x) for x in row) for row in zip(*got)]


def inverted_of(dev, tid, par, cap=65536):
    return rows(dev.ctx.clip_inverted_tid(tid, *par, cap))


def check_inverted(dev, R, L, table, par, at_least=0, tids=range(len(CLENS))):
    n = 0
    for tid in tids:
        want = ip.inverted(R[tid], L[tid], table, dev.refs[tid], tid, *par)[0]
        if CLENS[tid] <= 5_000 and par[3] <= 5_000:
            assert ip.inverted(R[tid], L[tid], table, dev.refs[tid], tid, *par, many=False)[0] == want
        got = inverted_of(dev, tid, par)
        assert got == want, (tid, par, [x for x in got if x not in want][:8], [x for x in want if x not in got][:8])
        n += len(want)
    assert n >= at_least, (par, n)
    return n


def build(dev, tid, R, L):
    """contig tid's two arrays through im_clip_build"""
    pos = np.concatenate([np.repeat(np.arange(len(R[tid])), R[tid]), np.repeat(np.arange(len(L[tid])), L[tid])])
    side = np.concatenate([np.zeros(int(R[tid].sum()), np.uint8), np.ones(int(L[tid].sum()), np.uint8)])
    dev.ctx.clip_build(CLENS[tid], pos, side)


class Scenario:
    """hand-made junctions on the three contigs: the arrays, the table and what some sites must answer whatever the restatement says.
    known: {(tid, side, x): [(y, c1, c2, v1, v2, s)]}"""

    def __init__(self, seed=12):
        rng = np.random.default_rng(seed)
        refs = [bytearray(bytes(rng.choice(np.frombuffer(b"ACGT", np.uint8), n))) for n in CLENS]
        self.R, self.L = empty_arrays()
        self.A = (self.R, self.L)
        self.table, self.known = {}, {}
        at = iter(range(3_000, 148_000, 1_000))
        # what has to be planted into the reference comes first.  Two partners: the 40 bases the pile at P is compared with behind
        # P + 200 stand behind P + 300 as well (right clips: in front of them, left clips: from them on)
        self.P = {RIGHT: next(at), LEFT: next(at)}
        refs[0][self.P[RIGHT] + 260:self.P[RIGHT] + 300] = refs[0][self.P[RIGHT] + 160:self.P[RIGHT] + 200]
        refs[0][self.P[LEFT] + 300:self.P[LEFT] + 340] = refs[0][self.P[LEFT] + 200:self.P[LEFT] + 240]
        # Ns where a pile's clipped bases continue: one (within the tolerance of 30 bases) and two
        self.N = {(side, k): next(at) for side in (RIGHT, LEFT) for k in (1, 2)}
        for (side, k), p in self.N.items():
            for j in (3, 9)[:k]:
                refs[0][p + 200 - 1 - j if side == RIGHT else p + 200 + j] = ord("N")
        self.refs = [bytes(r) for r in refs]
        junction, put, ref = self.junction, self.put, self.refs[0]
        for side in (RIGHT, LEFT):
            sign = 1 if side == RIGHT else -1
            p = self.P[side]
            junction(side, p, p + 200); junction(side, p, p + 300, n1=0, n2=4)
            self.known[(0, side, p)] = [(p + 200, 3, 3, 3, 3, 0), (p + 300, 3, 4, 3, 4, 0)]
            for k in (1, 2):
                p = self.N[(side, k)]; junction(side, p, p + 200); self.known[(0, side, p)] = [(p + 200, 3, 3, 3, 3, 0)] if k == 1 else []
            # entries that are the reference itself, entries in the wrong direction, and the other junction's entries
            p = next(at); junction(side, p, p + 200, plain=True); self.known[(0, side, p)] = []
            p = next(at); self.known[(0, side, p)] = []
            put(side, p, [comp_codes(ref, p + 200 if side == RIGHT else p + 199, 30, sign)] * 3)
            put(side, p + 200, [comp_codes(ref, p if side == RIGHT else p - 1, 30, sign)] * 3)
            p = next(at); self.known[(0, side, p)] = []
            put(side, p, [comp_codes(ref, p + 200, 30) if side == RIGHT else comp_codes(ref, p + 199, 30, -1)] * 3)
            put(side, p + 200, [comp_codes(ref, p, 30) if side == RIGHT else comp_codes(ref, p - 1, 30, -1)] * 3)
            # the distance window's four edges
            for d, ok in ((49, False), (50, True), (400, True), (401, False)):
                p = next(at); junction(side, p, p + d); self.known[(0, side, p)] = [(p + d, 3, 3, 3, 3, 0)] if ok else []
            # homology of 5 at the first pile and 3 at the second: the one shift 8; 20 and 12: shift 32; 20 and 13: nothing
            for h1, h2 in ((5, 3), (20, 12), (20, 13), (0, 6)):
                p = next(at); junction(side, p, p + 150, h1=h1, h2=h2)
                self.known[(0, side, p + sign * h1)] = [(p + 150 + sign * h2, 3, 3, 3, 3, h1 + h2)] if h1 + h2 <= 32 else []
            # equal sums at shifts 0 and 7: the smaller shift
            p = next(at); junction(side, p, p + 150, n1=2, n2=2); junction(side, p, p + 150, n1=2, n2=2, s=7); self.known[(0, side, p)] = [(p + 150, 4, 4, 2, 2, 0)]
            # min_verified: enough at one pile, one short at the other (the other entries are somebody else's bases), either way round
            p = next(at); junction(side, p, p + 150, n1=4, n2=1); put(side, p + 150, [comp_codes(ref, 777 + 40 * i, 30) for i in range(3)]); self.known[(0, side, p)] = []
            p = next(at); junction(side, p, p + 150, n1=1, n2=4); put(side, p, [comp_codes(ref, 555 + 40 * i, 30) for i in range(3)]); self.known[(0, side, p)] = []
            # v1 >= mv at shift 5 only, the largest sum at shift 0, where v1 is one short: the first cut passes, the pair does not
            p = next(at); junction(side, p, p + 150, n1=1, n2=4); junction(side, p, p + 150, n1=2, n2=0, s=5); self.known[(0, side, p)] = []
            # the tolerance at n = 15, 16, 31 and 32: n >> 4 differences match, one more does not
            flip = lambda t, where: tuple((b + 1) % 4 if i in where else b for i, b in enumerate(t))
            for n, allowed in ((15, 0), (16, 1), (31, 1), (32, 2)):
                p = next(at); junction(side, p, p + 150, n1=1, n2=3, n=n)
                e = self.table[(0, side, p)][0]
                put(side, p, [flip(e, range(3, 3 + allowed)), flip(e, range(3, 4 + allowed)), flip(e, range(3, 4 + allowed))])
                self.known[(0, side, p)] = [(p + 150, 4, 3, 2, 3, 0)]
            # a peak that is the y of one pair and the x of another
            p = next(at); junction(side, p, p + 200); junction(side, p + 200, p + 400)
            self.known[(0, side, p)] = [(p + 200, 3, 6, 3, 3, 0)]; self.known[(0, side, p + 200)] = [(p + 400, 6, 3, 3, 3, 0)]
            # piles of 1, 63, 64, 65 and 130 entries at x and at y, across the held batch and the walked pile; lengths 20 .. 32 mixed
            for n in (1, 63, 64, 65, 130):
                p = next(at); junction(side, p, p + 120, n1=n, n2=3, mixed=True); self.known[(0, side, p)] = [(p + 120, n, 3, n, 3, 0)] if n >= 3 else []
                p = next(at); junction(side, p, p + 120, n1=3, n2=n, mixed=True); self.known[(0, side, p)] = [(p + 120, 3, n, 3, n, 0)] if n >= 3 else []
            p = next(at); junction(side, p, p + 120, n1=130, n2=130, mixed=True); self.known[(0, side, p)] = [(p + 120, 130, 130, 130, 130, 0)]
            # half of a big pile is somebody else's: the count says 66, 33 verify
            p = next(at); junction(side, p, p + 120, n1=33, n2=3); put(side, p, [comp_codes(ref, 999 + 3 * i, 32) for i in range(33)]); self.known[(0, side, p)] = [(p + 120, 66, 3, 33, 3, 0)]
        # a right pair and a left pair on the same positions
        self.both_at = p = next(at)
        junction(RIGHT, p, p + 200); junction(LEFT, p, p + 200)
        self.known[(0, RIGHT, p)] = self.known[(0, LEFT, p)] = [(p + 200, 3, 3, 3, 3, 0)]
        self.foreign_at = next(at); junction(RIGHT, self.foreign_at, self.foreign_at + 100, n1=12); self.known[(0, RIGHT, self.foreign_at)] = [(self.foreign_at + 100, 12, 3, 12, 3, 0)]
        # windows that reach past either end of a contig: contig 2 as a whole (70 bases), contig 1's last bases, contig 0's first
        junction(RIGHT, 5, 60, tid=2, n=5); self.known[(2, RIGHT, 5)] = [(60, 3, 3, 3, 3, 0)]
        junction(LEFT, 4, 60, tid=2, n=10); self.known[(2, LEFT, 4)] = [(60, 3, 3, 3, 3, 0)]
        c1 = CLENS[1]
        junction(LEFT, c1 - 80, c1 - 20, tid=1, n=20); self.known[(1, LEFT, c1 - 80)] = [(c1 - 20, 3, 3, 3, 3, 0)]
        junction(LEFT, c1 - 280, c1 - 220, tid=1, n=20, h1=0, h2=0)
        self.table[(1, LEFT, c1 - 280)] = [comp_codes(self.refs[1], c1 - 10, 20)] * 3; self.known[(1, LEFT, c1 - 280)] = []     # its last 10 bases lie behind the contig
        junction(RIGHT, 6, 70, n=6); junction(RIGHT, 500, 570, n=20)
        self.table[(0, RIGHT, 570)] = [comp_codes(self.refs[0], 9, 20, -1)] * 3                 # its last 10 bases lie in front of the contig
        self.known[(0, RIGHT, 6)] = [(70, 3, 3, 3, 3, 0)]; self.known[(0, RIGHT, 500)] = []
        junction(LEFT, 0, 200, tid=0); self.known[(0, LEFT, 0)] = [(200, 3, 3, 3, 3, 0)]
        # a pair on contig 1 at the positions of contig 0's first site, where contig 0 holds entries of its own and, at the second
        # position, six that would verify on contig 1: the table is keyed by contig
        assert self.P[RIGHT] == 3_000
        junction(RIGHT, 3_000, 3_200, tid=1); self.known[(1, RIGHT, 3_000)] = [(3_200, 3, 3, 3, 3, 0)]
        self.table[(0, RIGHT, 3_200)].extend(self.table[(1, RIGHT, 3_200)] * 2)

    def put(self, side, p, entries, tid=0):
        self.A[side][tid][p] += len(entries)
        self.table.setdefault((tid, side, p), []).extend(entries)

    def junction(self, side, a, b, tid=0, n1=3, n2=3, h1=0, h2=0, s=None, n=30, mixed=False, plain=False):
        """one junction of an inversion of [a, b): n1 entries at a's pile, n2 at b's, moved by h1 and h2 bases of homology (or, with s,
        not moved, holding what they would hold at shift s); plain: the reference as it stands, not complemented"""
        ref = self.refs[tid]
        s1, s2 = (s, s) if s is not None else (h1, h2)
        if s is not None:
            h1 = h2 = 0
        ln = lambda k: 20 + k % 13 if mixed else n
        if side == RIGHT:
            x, y = a + h1, b + h2
            e1 = [comp_codes(ref, b - 1 - s1, ln(k), -1) for k in range(n1)]; e2 = [comp_codes(ref, a - 1 - s2, ln(k), -1) for k in range(n2)]
        else:
            x, y = a - h1, b - h2
            e1 = [comp_codes(ref, b + s1, ln(k)) for k in range(n1)]; e2 = [comp_codes(ref, a + s2, ln(k)) for k in range(n2)]
        if plain:
            e1, e2 = [tuple(3 - c for c in e) for e in e1], [tuple(3 - c for c in e) for e in e2]
        self.put(side, x, e1, tid); self.put(side, y, e2, tid)


@pytest.fixture(scope="module")
def scenario():
    sc = Scenario()
    # the restatement agrees with the figures worked by hand, before any device is asked
    n = 0
    for tid in range(3):
        want = ip.inverted(sc.R[tid], sc.L[tid], sc.table, sc.refs[tid], tid, *PAR)[0]
        for (t, side, x), answers in sc.known.items():
            if t == tid:
                assert [w[2:8] for w in want if w[0] == side and w[1] == x] == answers, (t, side, x, [w for w in want if w[1] == x], answers)
        n += len(want)
    assert n == sum(len(v) for v in sc.known.values())              # and nothing else qualifies: no chance pair
    return sc


def test_inverted_pairs_made_by_hand(scenario):
    sc = scenario
    log2 = 13
    h = ct.home_slot(0, RIGHT, sc.foreign_at, log2)
    foreign = next((side, q) for q in range(1_000, 140_000) for side in (RIGHT, LEFT) if ct.home_slot(0, side, q, log2) == (h + 3) % (1 << log2))
    rng = np.random.default_rng(4)
    theirs = [tuple(int(x) for x in rng.integers(0, 4, 32)) for _ in range(12)]
    mine = sc.table[(0, RIGHT, sc.foreign_at)]
    dev = Device(log2_slots=log2, refs=sc.refs)
    try:
        dev.counts(sc.R, sc.L)
        # a foreign key interleaved in the same probe run: its home slot lies three behind, and the entries of the two arrive in turns
        for k in range(0, 12, 3):
            dev.add({(0, RIGHT, sc.foreign_at): mine[k:k + 3]})
            dev.add({(0, foreign[0], foreign[1]): theirs[k:k + 3]})
        table = dict(sc.table)
        dev.add({k: v for k, v in table.items() if k != (0, RIGHT, sc.foreign_at)})
        table[(0, foreign[0], foreign[1])] = table.get((0, foreign[0], foreign[1]), []) + theirs
        assert dev.ctx.cliptail_stats() == (sum(len(v) for v in table.values()), 0)
        total = check_inverted(dev, sc.R, sc.L, table, PAR, at_least=55)
        for tid in range(3):
            got = inverted_of(dev, tid, PAR)
            for (t, side, x), answers in sc.known.items():
                if t == tid:
                    assert [g[2:8] for g in got if g[0] == side and g[1] == x] == answers, (t, side, x)
        # the pair on contig 1 did not read contig 0's entries at its positions
        got = [g for g in inverted_of(dev, 1, PAR) if g[:3] == (RIGHT, 3_000, 3_200)]
        assert got == [(RIGHT, 3_000, 3_200, 3, 3, 3, 3, 0, 3, 3)] and len(table[(0, RIGHT, 3_000)]) == 3 and len(table[(0, RIGHT, 3_200)]) == 9
        assert [g for g in inverted_of(dev, 0, PAR) if g[:3] == (RIGHT, 3_000, 3_200)] == [(RIGHT, 3_000, 3_200, 3, 3, 3, 3, 0, 3, 9)]
        # a right pair and a left pair on the same positions come back in the order (x, y, side)
        got = [g[:3] for g in inverted_of(dev, 0, PAR) if g[1] == sc.both_at]
        assert got == [(RIGHT, sc.both_at, sc.both_at + 200), (LEFT, sc.both_at, sc.both_at + 200)]
        # other parameters: piles of one read, no reach, no shift, a shift that stops in front of the planted ones, every distance (the
        # first cut drops the thousands of chance pairs), one distance, mv above most piles and above all
        for par, n in (((1, 30, 50, 400, 32, 1), 65), ((3, 0, 50, 400, 32, 2), 55), ((3, 64, 50, 400, 0, 2), 40), ((3, 30, 50, 400, 7, 2), 40),
                       ((3, 30, 1, 2_000_000_000, 32, 2), 60), ((3, 30, 120, 120, 32, 3), 14), ((3, 30, 50, 400, 32, 64), 2), ((2, 1, 50, 5_000, 31, 131), 0)):
            check_inverted(dev, sc.R, sc.L, table, par, at_least=n)
        # cap below the total: n_found is exact and the call succeeds; with room for all the pairs come sorted by (x, y, side)
        lib, ptr = dev.capi.lib(), lambda a: a.ctypes.data_as(C.c_void_p)
        want = ip.inverted(sc.R[0], sc.L[0], table, sc.refs[0], 0, *PAR)[0]
        assert 50 < len(want) < total and want == sorted(want, key=lambda r: (r[1], r[2], r[0]))
        out, found = [np.zeros(len(want), k) for k in dev.ctx._INVERTED], C.c_int32(-7)
        for cap in (0, 1, len(want) - 1):
            assert lib.im_clip_inverted_tid(dev.ctx.h, 0, *PAR, cap, *[ptr(o) for o in out], C.byref(found)) == 0 and found.value == len(want), cap
        assert lib.im_clip_inverted_tid(dev.ctx.h, 0, *PAR, 0, *[None] * 10, C.byref(found)) == 0 and found.value == len(want)
        assert lib.im_clip_inverted_tid(dev.ctx.h, 0, *PAR, len(want), *[ptr(o) for o in out], C.byref(found)) == 0 and found.value == len(want)
        assert rows(out) == want
        assert inverted_of(dev, 0, PAR, cap=2) == want              # the binding asks again by itself
        # the build form, contig by contig: the arrays of the last im_clip_build, the table and the reference of the contig named
        for tid in (1, 0, 2):
            build(dev, tid, sc.R, sc.L)
            assert rows(dev.ctx.clip_inverted(tid, *PAR)) == inverted_of(dev, tid, PAR), tid
            other = (tid + 1) % 3
            assert lib.im_clip_inverted(dev.ctx.h, other, *PAR, 4, *[ptr(o) for o in out], C.byref(found)) != 0 and b"are not contig" in lib.im_last_error(dev.ctx.h)
    finally:
        dev.close()


def test_inverted_one_list_empty_and_empty_arrays(scenario):
    """n_right = 0 with left peaks only, and the reverse: the one launch serves the list that is there; no peaks at all: no launch"""
    sc = scenario
    zeros = empty_arrays()[0]
    dev = Device(log2_slots=13, refs=sc.refs)
    try:
        dev.add(sc.table)
        want_all = [ip.inverted(sc.R[tid], sc.L[tid], sc.table, sc.refs[tid], tid, *PAR)[0] for tid in range(3)]
        for R, L, side in ((zeros, sc.L, LEFT), (sc.R, zeros, RIGHT)):
            dev.counts(R, L)
            n = check_inverted(dev, R, L, sc.table, PAR, at_least=25)
            assert [inverted_of(dev, tid, PAR) for tid in range(3)] == [[w for w in want_all[tid] if w[0] == side] for tid in range(3)]
            assert n < sum(len(w) for w in want_all)
            build(dev, 0, R, L)
            assert rows(dev.ctx.clip_inverted(0, *PAR)) == inverted_of(dev, 0, PAR)
        # a single peak on either list has no partner; then nothing at all, with the table still full
        one_r, one_l = empty_arrays()
        one_r[0][sc.both_at] = 3; one_l[0][sc.both_at + 200] = 3
        dev.counts(one_r, one_l)
        assert check_inverted(dev, one_r, one_l, sc.table, PAR) == 0
        dev.counts(zeros, zeros)
        assert [inverted_of(dev, tid, PAR) for tid in range(3)] == [[], [], []]
        assert [inverted_of(dev, tid, (1, 0, 1, 2_000_000_000, 32, 1)) for tid in range(3)] == [[], [], []]
    finally:
        dev.close()


def test_the_searches_share_the_workspace(scenario):
    """the crossed, inverted and facing searches lay their lists and columns over one workspace: asked in turns on one context, each
    answers as the restatement does, whatever ran before it -- also when every search asks again, with cap = 1, between the others.
    The scenario's own piles make no crossed pair, so four duplications are planted into a copy of it, clear of its sites."""
    from tests.support import crossedpiles as cp
    from tests.support import facingpiles as fp
    from tests.test_gpu_crossed import codes
    sc, ref = scenario, scenario.refs[0]
    R, L = [a.copy() for a in sc.R], [a.copy() for a in sc.L]
    table = {k: list(v) for k, v in sc.table.items()}
    planted = ((3_700, 3), (10_700, 4), (50_700, 70), (120_700, 3))
    for p, n in planted:                                            # [p - 150, p) duplicated: n right entries at p, 3 left ones at p - 150
        R[0][p] += n; L[0][p - 150] += 3
        table.setdefault((0, RIGHT, p), []).extend([codes(ref, p - 150, 30)] * n)
        table.setdefault((0, LEFT, p - 150), []).extend([codes(ref, p - 1, 30, -1)] * 3)
    want = {"crossed": cp.crossed(R[0], L[0], table, ref, 0, *PAR)[0], "inverted": ip.inverted(R[0], L[0], table, ref, 0, *PAR)[0],
            "facing": fp.facing_many(R[0], L[0], 3, 30)}
    assert [w[:7] for w in want["crossed"]] == [(p, p - 150, n, 3, n, 3, 0) for p, n in planted]
    assert want["inverted"] == ip.inverted(sc.R[0], sc.L[0], sc.table, ref, 0, *PAR)[0] and len(want["inverted"]) > 50 and len(want["facing"]) >= 3
    dev = Device(log2_slots=13, refs=sc.refs)
    ask = {"crossed": lambda cap: rows(dev.ctx.clip_crossed_tid(0, *PAR, cap)), "inverted": lambda cap: inverted_of(dev, 0, PAR, cap),
           "facing": lambda cap: dev.facing(0, 3, 30, cap)}
    try:
        dev.counts(R, L)
        dev.add(table)
        turns = ("crossed", "inverted", "crossed", "facing")
        for cap in (65536, 1):
            for order in (turns, turns[::-1]):
                for kind in order:
                    assert ask[kind](cap) == want[kind], (cap, order, kind)
    finally:
        dev.close()


def test_inverted_more_peaks_than_waves():
    """a contig of 20 000 positions with a count of 1 on every second position of either array, m = 1, T = 0: 20 000 peaks on a grid
    that is capped at 8 192 waves, three partners each; some dozens of planted pairs among them, a few with two partners"""
    from indelminer_amd import capi
    clen = 20_000
    rng = np.random.default_rng(8)
    ref = bytes(rng.choice(np.frombuffer(b"ACGT", np.uint8), clen))
    R, L = np.zeros(clen + 1, np.int64), np.zeros(clen + 1, np.int64)
    R[0:clen:2] = 1; L[1:clen:2] = 1
    table = {}
    for k, x in enumerate(range(400, 19_600, 400)):
        # right clips on even positions: [x, x + 4) inverted, and every third time the pile at x + 6 as well, at shift 2
        table[(0, RIGHT, x)] = [comp_codes(ref, x + 3, 30, -1)]; table[(0, RIGHT, x + 4)] = [comp_codes(ref, x - 1, 30, -1)]
        if k % 3 == 0:
            table[(0, RIGHT, x + 6)] = [comp_codes(ref, x - 1 - 2, 30, -1)]
        # left clips on odd positions, 200 further on
        table[(0, LEFT, x + 201)] = [comp_codes(ref, x + 207, 30)]; table[(0, LEFT, x + 207)] = [comp_codes(ref, x + 201, 30)]
    par = (1, 0, 2, 6, 32, 1)
    want, n_cand = ip.inverted(R, L, table, ref, 0, *par)
    assert sum(n_cand) > 3 * 8_192 * 2 and len(want) >= 2 * 48 + 16 and sum(1 for w in want if w[7] == 2) >= 16
    ctx = capi.Context(0)
    try:
        ctx.set_reference([ref])
        ctx.clip_enable(20, 10)
        ctx.cliptail_enable(20, 10, 12)
        ent = [(p, side, b) for (_, side, p), lst in table.items() for b in lst]
        ctx.cliptail_add(0, [e[0] for e in ent], [e[1] for e in ent], [len(e[2]) for e in ent], np.array([ct.planes_of(e[2]) for e in ent], np.uint32).reshape(-1, 2))
        pos = np.concatenate([np.nonzero(R)[0], np.nonzero(L)[0]])
        ctx.clip_build(clen, pos, np.concatenate([np.zeros(clen // 2, np.uint8), np.ones(clen // 2, np.uint8)]))
        assert len(ctx.clip_peaks(RIGHT, 1, 0)[0]) + len(ctx.clip_peaks(LEFT, 1, 0)[0]) == 20_000
        assert rows(ctx.clip_inverted(0, *par)) == want
        assert rows(ctx.clip_inverted(0, *par, cap=5)) == want
        assert rows(ctx.clip_inverted(0, 1, 0, 2, 6, 1, 1)) == ip.inverted(R, L, table, ref, 0, 1, 0, 2, 6, 1, 1)[0]
    finally:
        ctx.close()


def test_inverted_table_at_its_smallest_overflow_and_reset():
    """64 slots: two junctions whose keys' home slots are the table's last ones and its first, so the probe runs collide and wrap"""
    refs = contigs()
    homes = {}
    for p in range(1_000, 140_000):
        for side in (RIGHT, LEFT):
            homes.setdefault((side, ct.home_slot(0, side, p, 6)), []).append(p)

    def pick(side, hx, hy, taken):
        for x in homes[(side, hx)]:
            for y in homes[(side, hy)]:
                if 50 <= y - x <= 400 and all(abs(x - t) > 1_000 for t in taken):
                    return x, y
        raise AssertionError("no such pair")

    a = pick(RIGHT, 63, 62, [])
    b = pick(LEFT, 61, 0, [a[0]])
    R, L = empty_arrays()
    table = {}
    R[0][a[0]] = R[0][a[1]] = 6; L[0][b[0]] = L[0][b[1]] = 5
    table[(0, RIGHT, a[0])] = [comp_codes(refs[0], a[1] - 1, 30, -1)] * 6; table[(0, RIGHT, a[1])] = [comp_codes(refs[0], a[0] - 1, 30, -1)] * 6
    table[(0, LEFT, b[0])] = [comp_codes(refs[0], b[1], 30)] * 5; table[(0, LEFT, b[1])] = [comp_codes(refs[0], b[0], 30)] * 5
    want = sorted([(RIGHT, a[0], a[1], 6, 6, 6, 6, 0, 6, 6), (LEFT, b[0], b[1], 5, 5, 5, 5, 0, 5, 5)], key=lambda r: (r[1], r[2], r[0]))
    dev = Device(log2_slots=6, refs=refs)
    lib, ptr = dev.capi.lib(), lambda x: x.ctypes.data_as(C.c_void_p)
    try:
        dev.counts(R, L)
        dev.add(table)
        assert dev.ctx.cliptail_stats() == (22, 0)
        assert want == ip.inverted(R[0], L[0], table, refs[0], 0, *PAR)[0]
        check_inverted(dev, R, L, table, PAR, at_least=2)
        # 15 more make 37: 32 stored, 5 dropped; no answer, and nothing is written
        dev.add({(1, LEFT, 2_000): [comp_codes(refs[1], 100, 25)] * 15})
        assert dev.ctx.cliptail_stats() == (32, 5)
        assert inverted_of(dev, 0, PAR) is None and inverted_of(dev, 1, PAR) is None
        out, found = [np.full(4, 77, k) for k in dev.ctx._INVERTED], C.c_int32(0)
        assert lib.im_clip_inverted_tid(dev.ctx.h, 0, *PAR, 4, *[ptr(o) for o in out], C.byref(found)) == 0 and found.value == -1
        assert all((o == 77).all() for o in out)
        dev.ctx.cliptail_reset()
        dev.add(table)
        check_inverted(dev, R, L, table, PAR, at_least=2)
    finally:
        dev.close()


def test_inverted_arguments():
    from indelminer_amd import capi
    lib, ptr = capi.lib(), lambda a: a.ctypes.data_as(C.c_void_p)
    out, found = [np.zeros(4, k) for k in capi.Context._INVERTED], C.c_int32(-7)
    args = lambda: [ptr(o) for o in out] + [C.byref(found)]
    ctx = capi.Context(0)
    try:
        ctx.set_reference(contigs())
        assert lib.im_clip_inverted_tid(ctx.h, 0, *PAR, 4, *args()) != 0                # before im_clip_enable
        ctx.clip_enable(20, 10)
        assert lib.im_clip_inverted_tid(ctx.h, 0, *PAR, 4, *args()) != 0 and lib.im_last_error(ctx.h) == b"im_cliptail_enable has not been called"
        assert lib.im_clip_inverted(ctx.h, 0, *PAR, 4, *args()) != 0 and lib.im_last_error(ctx.h) == b"im_clip_build has not been called"
        ctx.cliptail_enable(20, 10, 6)
        for tid in range(3):
            assert lib.im_clip_inverted_tid(ctx.h, tid, *PAR, 4, *args()) == 0 and found.value == 0         # empty arrays, an empty table
        ctx.clip_build(CLENS[1], np.zeros(0, np.int32), np.zeros(0, np.uint8))
        assert lib.im_clip_inverted(ctx.h, 1, *PAR, 4, *args()) == 0 and found.value == 0
        assert lib.im_clip_inverted(ctx.h, 0, *PAR, 4, *args()) != 0 and b"are not contig 0's" in lib.im_last_error(ctx.h)
        m, T, dmin, dmax, S, mv = PAR
        for bad, word in (((0, T, dmin, dmax, S, mv, 4), b"min_reads 0"), ((m, 65, dmin, dmax, S, mv, 4), b"reach 65"), ((m, -1, dmin, dmax, S, mv, 4), b"reach -1"),
                          ((m, T, 0, dmax, S, mv, 4), b"min_len 0"), ((m, T, dmin, dmin - 1, S, mv, 4), b"max_len 49"), ((m, T, dmin, dmax, 33, mv, 4), b"max_shift 33"),
                          ((m, T, dmin, dmax, -1, mv, 4), b"max_shift -1"), ((m, T, dmin, dmax, S, 0, 4), b"min_verified 0"), ((m, T, dmin, dmax, S, mv, -1), b"cap -1")):
            assert lib.im_clip_inverted_tid(ctx.h, 0, *bad, *args()) != 0 and word in lib.im_last_error(ctx.h), bad
            assert lib.im_clip_inverted(ctx.h, 1, *bad, *args()) != 0 and word in lib.im_last_error(ctx.h), bad
        assert lib.im_clip_inverted_tid(ctx.h, 3, *PAR, 4, *args()) != 0 and lib.im_clip_inverted_tid(ctx.h, -1, *PAR, 4, *args()) != 0
        assert lib.im_clip_inverted(ctx.h, 3, *PAR, 4, *args()) != 0 and lib.im_clip_inverted(ctx.h, -1, *PAR, 4, *args()) != 0
        assert lib.im_clip_inverted_tid(None, 0, *PAR, 4, *args()) != 0 and lib.im_clip_inverted(None, 1, *PAR, 4, *args()) != 0
        assert lib.im_clip_inverted_tid(ctx.h, 0, *PAR, 4, *[ptr(o) for o in out], None) != 0
        for k in range(10):
            holed = [ptr(o) for o in out]; holed[k] = None
            assert lib.im_clip_inverted_tid(ctx.h, 0, *PAR, 4, *holed, C.byref(found)) != 0, k
            assert lib.im_clip_inverted(ctx.h, 1, *PAR, 4, *holed, C.byref(found)) != 0, k
        assert lib.im_clip_inverted_tid(ctx.h, 0, m, T, dmin, dmin, 0, 1, 0, *[None] * 10, C.byref(found)) == 0 and found.value == 0
    finally:
        ctx.close()


# ------------------------------------------------------------------------------------------ the soak

def inv_read(ref, tid, side, at, other, s, Lc, m, flips=(), n_at=(), mapq=60):
    """a read clipped at `at` whose Lc clipped bases continue on the other strand at `other`, at shift s: side RIGHT: m aligned bases in
    front of `at`, clipped base i = comp(ref[other - 1 - s - i]); side LEFT: aligned from `at`, clipped base i (counted from the junction) =
    comp(ref[other + s + i]).  Outside the contig the base is A.  flips / n_at: clipped bases (counted from the junction) that get another
    base / an N"""
    from tests.test_gpu_cliptail import CODE, M, S

    def base(p, i):
        c = b"TGCA"[b"ACGT".index(ref[p:p + 1])] if 0 <= p < len(ref) else ord("A")
        if i in flips:
            c = b"ACGT"[(b"ACGT".index(bytes([c])) + 1 + i % 3) % 4]
        return CODE[ord("N")] if i in n_at else CODE[c]
    aligned = lambda lo: [CODE[ref[p]] if 0 <= p < len(ref) else CODE[65] for p in range(lo, lo + m)]
    if side == RIGHT:
        return (tid, at - m, mapq, 0, [(M, m), (S, Lc)], m + Lc, aligned(at - m) + [base(other - 1 - s - i, i) for i in range(Lc)])
    return (tid, at, mapq, 0, [(S, Lc), (M, m)], m + Lc, [base(other + s + i, i) for i in range(Lc)][::-1] + aligned(at))


def soak_records(refs, seed, n_records=20_000, n_hot=300):
    """records with clips at 300 hot positions: 150 inversions [a, b) of 50 .. 3 000 bases on two contigs, some sharing a breakpoint's
    neighbourhood; at each, four piles (right clips at a and at b, left clips at a and at b) of up to 15 reads whose clipped bases are
    the complement of the reference running backwards from the other breakpoint at the junction's shift (or now and then at another),
    with flipped bases, Ns and low mapping qualities; clipped reads of random bases at random places and at the piles; and the many
    reads that do not clip.  The reads are planted as an inversion leaves them, on a random reference."""
    from tests.test_gpu_cliptail import M, S, with_bases
    rng = np.random.default_rng(seed)
    recs = []
    sites = [(0, int(a), int(w)) for a, w in zip(range(4_000, 146_000, 1_000), rng.integers(50, 3_000, 142))]
    sites += [(1, int(a), int(w)) for a, w in zip(range(300, 4_300, 500), rng.integers(50, 600, 8))]
    assert 2 * len(sites) == n_hot
    for tid, a, w in sites:
        b = min(a + w, CLENS[tid] - 100)
        for side in (RIGHT, LEFT):
            s = int(rng.choice([0, 0, 0, 1, 3, 7, 32, 33]))
            for at, other in ((a, b), (b, a)):
                for _ in range(int(rng.integers(0, 16))):
                    Lc = int(rng.integers(15, 71))
                    m = int(rng.integers(10, 81))
                    k = int(rng.choice([0, 0, 0, 1, 2, 3]))
                    n_at = [int(rng.integers(0, Lc))] if rng.random() < 0.05 else []
                    jitter = int(rng.choice([0, 0, 0, 0, 0, 1, 2, 31]))     # a few reads clip beside the pile
                    recs.append(inv_read(refs[tid], tid, side, at + jitter, other, s if rng.random() < 0.9 else int(rng.integers(0, 40)), Lc, m,
                                         flips=[int(x) for x in rng.integers(0, min(Lc, 32), k)], n_at=n_at, mapq=int(rng.choice([60, 60, 60, 9, 10]))))
    noise = []
    for _ in range(2_000):
        tid = int(rng.random() < 0.1)
        Lc, m = int(rng.integers(1, 80)), int(rng.integers(1, 90))
        pos = int(rng.integers(0, CLENS[tid] - 100)) if rng.random() < 0.7 else sites[int(rng.integers(0, len(sites)))][1]
        noise.append((tid if pos < CLENS[tid] - 100 else 0, pos, 60, int(rng.choice([0, 0, 0, 0x10, 0x400])), [[(M, m), (S, Lc)], [(S, Lc), (M, m)], [(S, Lc), (M, m), (S, Lc)]][int(rng.integers(0, 3))]))
    recs += with_bases(noise, seed + 1)
    assert len(recs) < n_records
    plain = [(int(rng.random() < 0.03), int(rng.integers(0, 4_800)), 60, 0, [(M, 100)]) for _ in range(n_records - len(recs))]
    recs += with_bases(plain, seed + 2)
    order = rng.permutation(len(recs))
    return [recs[int(k)] for k in order]


def test_inverted_seeded_soak_scatter_against_add_and_the_build_form():
    """20 000 records through im_dev_clip_scatter and im_dev_cliptail_scatter in three launches, both record forms, against the same
    events through im_clip_build and im_cliptail_add"""
    c, q = 20, 10
    refs = contigs()
    recs = soak_records(refs, 13)
    assert len(recs) == 20_000
    cuts = [0, 7_000, 13_001, len(recs)]
    parsed = []
    pars = ((3, 30, 50, 3_000, 32, 2), (2, 5, 50, 1_500, 32, 1), (3, 30, 300, 40_000, 8, 3))
    answers = []
    dev = Device(c, q, log2_slots=15, refs=refs)
    try:
        for k in range(3):
            raw, off = ct.pack_records(recs[cuts[k]:cuts[k + 1]], qual=k != 1)
            parsed += ct.parse_raw(raw, off)
            d_recs = dev.records(raw, off)
            dev.ctx.clip_scatter(d_recs)
            dev.ctx.cliptail_scatter(d_recs)
        dev.sync()
        R, L = cc.arrays_of(parsed, CLENS, c, q)
        table = ct.table_of(parsed, CLENS, c, q)
        assert 3_000 < sum(len(v) for v in table.values()) < 16_384 and max(len(v) for v in table.values()) >= 10
        assert dev.ctx.cliptail_stats() == (sum(len(v) for v in table.values()), 0)
        assert check_inverted(dev, R, L, table, pars[0], at_least=60) > check_inverted(dev, R, L, table, pars[2], at_least=15)
        check_inverted(dev, R, L, table, pars[1], at_least=50)
        want = ip.inverted(R[0], L[0], table, refs[0], 0, *pars[0])[0]
        assert sum(1 for w in want if w[7] > 0) >= 10 and sum(1 for w in want if w[5] < w[8] or w[6] < w[9]) >= 20      # shifts, and piles that verify in part
        assert sum(1 for w in want if w[0] == RIGHT) >= 20 and sum(1 for w in want if w[0] == LEFT) >= 20
        answers.append([inverted_of(dev, tid, par) for par in pars for tid in range(3)])
    finally:
        dev.close()
    dev = Device(c, q, log2_slots=15, refs=refs)
    try:
        dev.add(table)
        got = []
        for par in pars:
            for tid in range(3):
                build(dev, tid, R, L)
                got.append(rows(dev.ctx.clip_inverted(tid, *par)))
        answers.append(got)
    finally:
        dev.close()
    assert answers[0] == answers[1] and sum(len(x) for x in answers[0]) > 120


# ------------------------------------------------------------------------------------------ the product

def _run(binary, flags, cwd, env=None):
    e = dict(os.environ)
    e.update(env or {})
    return subprocess.run([binary] + flags + ["ref.fa", "sample=aln.bam"], cwd=cwd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=e)


def _ok(r):
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    assert b"overflowed" not in r.stderr
    return r


@pytest.fixture(scope="module")
def planted(tmp_path_factory):
    refs, rd = ip.planted_reads()
    d = ip.write_planted(str(tmp_path_factory.mktemp("inverted_planted")), refs, rd)
    text, recs, n_cand, n_peaks = ip.render_of_bam(d + "/aln.bam", d + "/ref.fa", 10)
    return d, text, recs, n_cand, n_peaks


BASE = ["-i", "cfg.txt", "-s", "100"]
ENVS = ({"INDELMINER_PIPELINE": "host"}, {"INDELMINER_PIECE_BYTES": "60000", "INDELMINER_WALKERS": "3"})


def test_product_inversion_breakpoints(planted, tmp_path):
    d, text, recs, n_cand, n_peaks = planted
    prod = _product()
    # the figures of the planted data set, from the restatement (tests/test_inverted_host.py has them without a GPU)
    assert n_peaks == (28, 28) and n_cand == (378, 378) and len(recs) == 18
    for side in (RIGHT, LEFT):
        assert [(r[2], r[3] - r[2]) for r in recs if r[1] == side] == ip.SITES
    f = str(tmp_path / "inv.vcf")
    gcv = _ok(_run(prod, BASE + ["-G", "-C", "-V"], d))
    gcvn = _ok(_run(prod, BASE + ["-G", "-C", "-V", "-N", f], d))
    got = open(f, "rb").read()
    assert got == text                                              # FILE is the restatement's rendering, byte for byte
    assert gcvn.stdout == gcv.stdout and gcvn.stderr == gcv.stderr and len(gcv.stdout) > 1000       # stdout and stderr do not know about -N
    for a, n in ip.SITES:                                           # every planted site is in FILE, once per junction
        for junction in ("3to3", "5to5"):
            assert sum(1 for ln in got.decode().split("\n") if ln.startswith("ctg0\t%d\t" % a) and ";END=%d;SVLEN=%d;CT=%s;" % (a + n, n, junction) in ln) == 1, (a, n)
    # the record-at-a-time path and three walkers on small pieces write the same bytes
    for k, env in enumerate(ENVS):
        fk = str(tmp_path / ("inv%d.vcf" % k))
        r = _ok(_run(prod, BASE + ["-G", "-C", "-V", "-N", fk], d, env=env))
        assert open(fk, "rb").read() == text and r.stdout == gcv.stdout, env
    # -D adds nothing to FILE: an inversion changes no depth
    fd = str(tmp_path / "invd.vcf")
    gdcv = _ok(_run(prod, BASE + ["-G", "-D", "-C", "-V"], d))
    r = _ok(_run(prod, BASE + ["-G", "-D", "-C", "-V", "-N", fd], d))
    assert open(fd, "rb").read() == text and r.stdout == gdcv.stdout and r.stderr == gdcv.stderr
    # with -I and -U beside it: all three files are what they are alone, and so are stdout and stderr
    for k, env in enumerate(({},) + ENVS[:1]):
        fi, fu, fi2, fu2, fn2 = (str(tmp_path / (name % k)) for name in ("ins%d.vcf", "dup%d.vcf", "ins%d_n.vcf", "dup%d_n.vcf", "inv%d_n.vcf"))
        r0 = _ok(_run(prod, BASE + ["-G", "-C", "-V", "-I", fi, "-U", fu], d, env=env))
        r1 = _ok(_run(prod, BASE + ["-G", "-C", "-V", "-I", fi2, "-U", fu2, "-N", fn2], d, env=env))
        assert open(fn2, "rb").read() == text and open(fi2, "rb").read() == open(fi, "rb").read() and open(fu2, "rb").read() == open(fu, "rb").read(), env
        assert r1.stdout == r0.stdout == gcv.stdout and r1.stderr == r0.stderr, env
        assert open(fi, "rb").read().count(b"<INS>") == 28          # what these inversions are printed as without -N, and still are with it
    # -o detailed ignores -N and writes no FILE; without -V it is refused
    fo = str(tmp_path / "none.vcf")
    d0 = _ok(_run(prod, BASE + ["-o", "detailed"], d))
    d1 = _ok(_run(prod, BASE + ["-o", "detailed", "-G", "-C", "-V", "-N", fo], d))
    assert d1.stdout == d0.stdout and d1.stderr == d0.stderr and len(d0.stdout) > 0 and not os.path.exists(fo)
    r = _run(prod, BASE + ["-G", "-C", "-N", fo], d)
    assert r.returncode != 0 and r.stdout == b"" and b"indelminer: -N needs -V" in r.stderr and not os.path.exists(fo)


def test_product_mapping_quality_gates_the_piles_and_duplications_are_not_inversions(tmp_path):
    """every second clipped read gets mapping quality 20: at -q 30 the piles are half as high, and fewer pairs qualify.  On the planted
    set of tandem duplications -N finds nothing: the header alone"""
    from tests.support import crossedpiles as cp
    (tmp_path / "inv").mkdir(); (tmp_path / "dup").mkdir()
    refs, rd = ip.planted_reads()
    d = ip.write_planted(str(tmp_path / "inv"), refs, rd, lower_mapq_of_every_second_clipped_read=True)
    prod = _product()
    n = {}
    for q in (10, 30):
        text, recs, _, _ = ip.render_of_bam(d + "/aln.bam", d + "/ref.fa", q)
        f = str(tmp_path / ("inv_q%d.vcf" % q))
        _ok(_run(prod, BASE + ["-q", str(q), "-G", "-C", "-V", "-N", f], d))
        assert open(f, "rb").read() == text, q
        n[q] = len(recs)
    assert n[10] == 2 * len(ip.SITES) and 0 < n[30] < n[10], n
    refs, rd = cp.planted_reads()
    d = cp.write_planted(str(tmp_path / "dup"), refs, rd)
    f = str(tmp_path / "inv_of_dup.vcf")
    _ok(_run(prod, BASE + ["-G", "-C", "-V", "-N", f], d))
    assert open(f, "rb").read() == ip.header().encode() == ip.render_of_bam(d + "/aln.bam", d + "/ref.fa", 10)[0]
