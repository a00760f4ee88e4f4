"""Tandem duplications from crossed clip piles (-U): the peaks pass of im_span.hip's clip_peaks_kernel, the candidate enumeration and
verification of im_cliptail.hip's cliptail_pairs_kernel<false>, and what the host driver makes of them (-U FILE).

The yardstick is the plain restatement in tests/support/crossedpiles.py, written from the definition in include/indelminer_amd.h (seam 5,
"Crossed piles"), not from the code under test; tests/test_crossed_host.py pins it to cases worked by hand.  Every answer is compared
exactly.
"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests.support import clipcounts as cc
from tests.support import cliptails as ct
from tests.support import crossedpiles as cp
from tests.support.clipcounts import LEFT, RIGHT
from tests.support.spanarrays import _product
from tests.test_gpu_facing import CLENS, LANE, SWEEP, TILE, WAVE, Device, contigs, empty_arrays, hot_arrays

pytestmark = pytest.mark.gpu

NONE = 0xFFFFFFFF


def peaks_of(dev, tid, side, m, T, cap=65536):
    return [(int(p), int(c)) for p, c in zip(*dev.ctx.clip_peaks_tid(tid, side, m, T, cap))]


def check_peaks(dev, R, L, m, T, at_least=0):
    n = 0
    for tid in range(len(CLENS)):
        for side, A in ((RIGHT, R[tid]), (LEFT, L[tid])):
            want = cp.peaks_many(A, m, T)
            if len(A) <= 5_001:
                assert cp.peaks(A, m, T) == want                    # the fast form against the plain one
            got = peaks_of(dev, tid, side, m, T)
            assert got == want, (tid, side, m, T, [x for x in got if x not in want][:8], [x for x in want if x not in got][:8])
            n += len(want)
    assert n >= at_least, n
    return n


# ------------------------------------------------------------------------------------------ peaks

def peak_cases(T, delta):
    """piles of both arrays whose four-position group and whose windows straddle the kernel's lane, wave, load and workgroup boundaries at
    delta, equal and higher neighbours at the reach and one beyond it, the contigs' ends and the boundaries between contigs"""
    R, L = empty_arrays()
    c0, c1, c2 = CLENS
    bounds = (LANE * 25, WAVE, SWEEP, SWEEP + WAVE * 3, TILE, TILE + SWEEP, 2 * TILE, 17 * TILE + 3 * SWEEP, 36 * TILE, 146 * SWEEP)
    for A, some, up in ((R, bounds, 0), (L, bounds[1::2] + (5 * TILE,), 1)):
        for b in some:
            p = b + delta
            A[0][p + 2 * T + 2] = 2                                 # below m, beside ...
            A[0][p + 2 * T + 1] = 3 + up                            # ... a pile of its own, just out of reach of the hidden one
            A[0][p - T - 1] = 6                                     # a higher pile just out of reach in front
            A[0][p + T] = 4 + up                                    # an equal pile T behind: hidden, its own window reaches back across
            A[0][p] = 4 + up
        b = 30 * TILE + delta                                       # a higher pile T behind hides, one T + 1 behind does not
        A[0][b] = 4; A[0][b + T] = 5 if T else 4
        A[0][b + 1_000] = 4; A[0][b + 1_000 + T + 1] = 5
        for b in (SWEEP, TILE):                                     # contig 1 has one workgroup boundary, and ends inside a four-position group
            p = b + delta
            A[1][p] = 3 + up; A[1][p - 1] = 2; A[1][p + 1] = 3 + up
        # the contigs' ends: nothing leaks across the boundaries of the genome-wide arrays
        A[0][0] = 3; A[0][c0] = 3 + up
        A[1][0] = 4; A[1][1] = 9 - up
        A[1][c1] = 5; A[1][c1 - 1] = 5
        A[2][0] = 3 + up; A[2][40] = 4; A[2][c2] = 4
    return R, L


@pytest.mark.parametrize("T", [30, 0, 64, 1])
def test_peaks_of_both_sides_at_kernel_and_contig_boundaries(T):
    dev = Device()
    try:
        for delta in (-1, 0, 1, 3):
            R, L = peak_cases(T, delta)
            dev.counts(R, L)
            check_peaks(dev, R, L, 3, T, at_least=40)
            if delta == 0:
                check_peaks(dev, R, L, 1, T, at_least=40)
                check_peaks(dev, R, L, 5, T, at_least=10)
                # a few answers, whatever the restatement says
                got = dict(peaks_of(dev, 0, RIGHT, 3, T))
                assert got.get(TILE) == 4 and got.get(TILE - T - 1) == 6 and (T == 0 or TILE + T not in got) and got.get(TILE + 2 * T + 1) == 3
                assert (T == 64 or got.get(0) == 3) and got.get(CLENS[0]) == 3      # contig 1's larger piles behind the boundary do not hide it
                got = dict(peaks_of(dev, 1, LEFT, 3, T))
                assert got.get(1) == 8 and (0 in got) == (T == 0) and got.get(CLENS[1] - 1) == 5 and (CLENS[1] in got) == (T == 0)
    finally:
        dev.close()


def test_peaks_seeded_soak_cap_the_build_form_empty_arrays_and_arguments():
    R, L = hot_arrays(23)
    assert sum(int(a.sum()) for a in R + L) == 20_000
    dev = Device()
    lib, ptr = dev.capi.lib(), lambda a: a.ctypes.data_as(C.c_void_p)
    out, found = [np.zeros(4, np.int32), np.zeros(4, np.uint32)], C.c_int32(-1)
    args = lambda: [ptr(o) for o in out] + [C.byref(found)]
    try:
        # empty arrays, and the build form before a build
        for tid in range(3):
            for side in (RIGHT, LEFT):
                assert lib.im_clip_peaks_tid(dev.ctx.h, tid, side, 1, 0, 4, *args()) == 0 and found.value == 0, (tid, side)
        assert lib.im_clip_peaks(dev.ctx.h, 0, 3, 30, 4, *args()) != 0 and lib.im_last_error(dev.ctx.h) == b"im_clip_build has not been called"
        dev.counts(R, L)
        n = check_peaks(dev, R, L, 3, 30, at_least=300)
        check_peaks(dev, R, L, 3, 64, at_least=200)
        check_peaks(dev, R, L, 1, 0, at_least=n)
        check_peaks(dev, R, L, 20, 30)
        # cap smaller than the total: n_found is exact, the call succeeds; a second call with enough room answers
        want = cp.peaks_many(L[0], 3, 30)
        assert len(want) > 100
        big = [np.zeros(len(want), np.int32), np.zeros(len(want), np.uint32)]
        for cap in (0, 1, len(want) - 1):
            assert lib.im_clip_peaks_tid(dev.ctx.h, 0, LEFT, 3, 30, cap, *[ptr(o) for o in big], C.byref(found)) == 0 and found.value == len(want), cap
        assert lib.im_clip_peaks_tid(dev.ctx.h, 0, LEFT, 3, 30, 0, None, None, C.byref(found)) == 0 and found.value == len(want)
        assert lib.im_clip_peaks_tid(dev.ctx.h, 0, LEFT, 3, 30, len(want), *[ptr(o) for o in big], C.byref(found)) == 0 and found.value == len(want)
        assert [(int(p), int(c)) for p, c in zip(*big)] == want
        assert peaks_of(dev, 0, LEFT, 3, 30, cap=7) == want         # the binding asks again by itself
        # im_clip_build + im_clip_peaks: the record-at-a-time form, contig by contig
        for tid in (1, 0, 2):
            pos = np.concatenate([np.repeat(np.arange(CLENS[tid] + 1), R[tid]), np.repeat(np.arange(CLENS[tid] + 1), L[tid])])
            side = np.concatenate([np.zeros(int(R[tid].sum()), np.uint8), np.ones(int(L[tid].sum()), np.uint8)])
            dev.ctx.clip_build(CLENS[tid], pos, side)
            for m, T in ((3, 30), (1, 0), (3, 64)):
                for s, A in ((RIGHT, R[tid]), (LEFT, L[tid])):
                    got = [(int(p), int(c)) for p, c in zip(*dev.ctx.clip_peaks(s, m, T))]
                    assert got == peaks_of(dev, tid, s, m, T) == cp.peaks_many(A, m, T), (tid, s, m, T)
        # the arguments: those of the facing search, and the side
        for bad, word in (((0, 0, 0, 30, 4), b"min_reads 0"), ((0, 0, 3, 65, 4), b"reach 65"), ((0, 1, 3, -1, 4), b"reach -1"), ((0, 0, 3, 30, -1), b"cap -1"),
                          ((0, 2, 3, 30, 4), b"side 2"), ((0, -1, 3, 30, 4), b"side -1")):
            assert lib.im_clip_peaks_tid(dev.ctx.h, *bad, *args()) != 0 and word in lib.im_last_error(dev.ctx.h), bad
            assert lib.im_clip_peaks(dev.ctx.h, *bad[1:], *args()) != 0 and word in lib.im_last_error(dev.ctx.h), bad
        assert lib.im_clip_peaks_tid(dev.ctx.h, 3, 0, 3, 30, 4, *args()) != 0 and lib.im_clip_peaks_tid(dev.ctx.h, -1, 0, 3, 30, 4, *args()) != 0
        assert lib.im_clip_peaks_tid(dev.ctx.h, 0, 0, 3, 30, 4, ptr(out[0]), ptr(out[1]), None) != 0
        assert lib.im_clip_peaks_tid(dev.ctx.h, 0, 0, 3, 30, 4, None, ptr(out[1]), C.byref(found)) != 0
        from indelminer_amd import capi
        ctx = capi.Context(0)
        try:
            ctx.set_reference(contigs())
            assert lib.im_clip_peaks_tid(ctx.h, 0, 0, 3, 30, 4, *args()) != 0       # before im_clip_enable
        finally:
            ctx.close()
    finally:
        dev.close()


# ------------------------------------------------------------------------------------------ crossed pairs

PAR = (3, 30, 50, 400, 32, 2)       # m, T, dmin, dmax, S, mv of the hand-made cases: the sites stand 2 000 apart, no site sees another's piles


def codes(ref, start, n, step=1):
    """n 2-bit codes of ref[start], ref[start + step], ...; A where there is no base"""
    return tuple(b"ACGT".index(ref[p:p + 1]) if 0 <= p < len(ref) and ref[p:p + 1] in (b"A", b"C", b"G", b"T") else 0 for p in (start + step * i for i in range(n)))


def crossed_of(dev, tid, par, cap=65536):
    got = dev.ctx.clip_crossed_tid(tid, *par, cap)
    return None if got is None else [tuple(int(x) for x in row) for row in zip(*got)]


def check_crossed(dev, R, L, table, par, at_least=0):
    n = 0
    for tid in range(len(CLENS)):
        want = cp.crossed(R[tid], L[tid], table, dev.refs[tid], tid, *par)[0]
        if CLENS[tid] <= 5_000:
            assert cp.crossed(R[tid], L[tid], table, dev.refs[tid], tid, *par, many=False)[0] == want
        got = crossed_of(dev, tid, par)
        assert got == want, (tid, par, [x for x in got if x not in want][:8], [x for x in want if x not in got][:8])
        n += len(want)
    assert n >= at_least, (par, n)
    return n


class Scenario:
    """hand-made duplications on the three contigs: the arrays, the table and what some sites must answer whatever the restatement says"""

    def __init__(self, seed=9):
        rng = np.random.default_rng(seed)
        refs = [bytearray(bytes(rng.choice(np.frombuffer(b"ACGT", np.uint8), n))) for n in CLENS]
        self.R, self.L = empty_arrays()
        self.table, self.known = {}, {}
        at = iter(range(3_000, 140_000, 2_000))
        # a planted repeat: the 40 bases at P - 300 are those at P - 200, so the right pile at P has two partners
        self.P = next(at)
        refs[0][self.P - 300:self.P - 260] = refs[0][self.P - 200:self.P - 160]
        # an N (two of them: more than the tolerance) where a right pile's clipped bases continue
        self.N = next(at)
        refs[0][self.N - 200 + 3] = refs[0][self.N - 200 + 9] = ord("N")
        self.refs = [bytes(r) for r in refs]
        dup = self.dup
        dup(self.P, self.P - 200); dup(self.P, self.P - 300, nr=0, nl=4)
        self.known[(0, self.P)] = [(self.P - 300, 3, 4, 3, 4, 0), (self.P - 200, 3, 3, 3, 3, 0)]
        dup(self.N, self.N - 200); self.known[(0, self.N)] = []
        # the distance window's four edges
        for d, ok in ((49, False), (50, True), (400, True), (401, False)):
            p = next(at); dup(p, p - d); self.known[(0, p)] = [(p - d, 3, 3, 3, 3, 0)] if ok else []
        # homology on both sides of 0, 5, 32 and 33 bases: the last finds nothing
        for s in (0, 5, 32, 33):
            p = next(at); dup(p, p - 150, sr=s, sl=s); self.known[(0, p)] = [(p - 150, 3, 3, 3, 3, s)] if s <= 32 else []
        # homology the reads of one side were extended into and the others were not: no shift verifies both sides ...
        p = next(at); dup(p, p - 150, sr=5, sl=0); self.known[(0, p)] = []
        p = next(at); dup(p, p - 150, sr=0, sl=7); self.known[(0, p)] = []
        # ... unless two reads of the other side were extended too: the larger sum decides the shift
        p = next(at); dup(p, p - 150, nr=3, nl=3, sr=5, sl=0); dup(p, p - 150, nr=0, nl=2, sl=5); self.known[(0, p)] = [(p - 150, 3, 5, 3, 2, 5)]
        # min_verified: enough on the right, one short on the left (the other left entries are somebody else's bases)
        p = next(at); dup(p, p - 150, nr=4, nl=1); self.add_left(p - 150, [codes(self.refs[0], 777 - i, 30, -1) for i in range(3)]); self.known[(0, p)] = []
        # piles of 1, 63, 64, 65 and 130 entries on the right, across the one-batch fast path, and of 130 on the left; lengths 20 .. 32 mixed
        self.sized = []
        for n in (1, 63, 64, 65, 130):
            p = next(at); dup(p, p - 120, nr=n, nl=3, mixed=True); self.sized.append(p)
            self.known[(0, p)] = [(p - 120, n, 3, n, 3, 0)] if n >= 3 else []
        p = next(at); dup(p, p - 120, nr=3, nl=130, mixed=True); self.known[(0, p)] = [(p - 120, 3, 130, 3, 130, 0)]
        # half of a big pile is somebody else's: the count says 66, 33 verify
        p = next(at); dup(p, p - 120, nr=33, nl=3); self.R[0][p] += 33
        self.table[(0, RIGHT, p)] += [codes(self.refs[0], 999 + 3 * i, 32) for i in range(33)]; self.known[(0, p)] = [(p - 120, 66, 3, 33, 3, 0)]
        self.foreign_at = next(at); dup(self.foreign_at, self.foreign_at - 100, nr=12, nl=3); self.known[(0, self.foreign_at)] = [(self.foreign_at - 100, 12, 3, 12, 3, 0)]
        # windows that reach past either end of a contig: contig 1's last bases, contig 2 as a whole, contig 0's first
        c1 = CLENS[1]
        dup(c1, c1 - 60, tid=1, n=20); self.known[(1, c1)] = [(c1 - 60, 3, 3, 3, 3, 0)]
        dup(60, 5, tid=2); self.known[(2, 60)] = [(5, 3, 3, 3, 3, 0)]
        dup(70, 0, tid=0, n=32); self.known[(0, 70)] = [(0, 3, 3, 3, 3, 0)]
        # a pair on contig 1 with the positions of a pair on contig 0: the table is keyed by contig
        dup(3_200, 3_000, tid=1); self.known[(1, 3_200)] = [(3_000, 3, 3, 3, 3, 0)]
        # the cut in front of the partner's walk: a right pile that reaches min_verified at no shift ends the pair before the left pile is
        # read (cut: {name: pr}, every left pile 150 in front).  One right entry continues at pl, three are somebody else's bases, the
        # left pile is good ...
        self.cut = {}
        foreign = lambda n, at: [codes(self.refs[0], at + 40 * i, 30) for i in range(n)]
        p = self.cut["none"] = next(at); dup(p, p - 150, nr=1, nl=4); self.add_right(p, foreign(3, 777)); self.known[(0, p)] = []
        # ... the right pile reaches it at shift 5 only and the left pile at shift 0 only: the cut passes, no shift serves both ...
        p = self.cut["no common shift"] = next(at); dup(p, p - 150, nr=3, nl=4, sr=5, sl=0); self.known[(0, p)] = []
        # ... a right pile of 65 entries, more than one batch of the walk, of which one verifies: the cut on the walked path ...
        p = self.cut["walked, one short"] = next(at); dup(p, p - 150, nr=1, nl=3); self.add_right(p, foreign(64, 5_555)); self.known[(0, p)] = []
        # ... and such a pile of which two verify, beside 63 of somebody else's: the cut passes on the walked path, and the pair stands
        p = self.cut["walked, enough"] = next(at); dup(p, p - 150, nr=2, nl=3); self.add_right(p, foreign(63, 9_999)); self.known[(0, p)] = [(p - 150, 65, 3, 2, 3, 0)]

    def dup(self, pr, pl, tid=0, nr=3, nl=3, sr=0, sl=0, n=30, mixed=False):
        ref = self.refs[tid]
        self.R[tid][pr] += nr; self.L[tid][pl] += nl
        self.table.setdefault((tid, RIGHT, pr), []).extend(codes(ref, pl + sr, 20 + k % 13 if mixed else n) for k in range(nr))
        self.table.setdefault((tid, LEFT, pl), []).extend(codes(ref, pr - 1 - sl, 20 + k % 13 if mixed else n, -1) for k in range(nl))

    def add_left(self, pl, entries, tid=0):
        self.L[tid][pl] += len(entries)
        self.table[(tid, LEFT, pl)] += entries

    def add_right(self, pr, entries, tid=0):
        self.R[tid][pr] += len(entries)
        self.table[(tid, RIGHT, pr)] += entries


@pytest.fixture(scope="module")
def scenario():
    sc = Scenario()
    # the restatement agrees with the figures worked by hand, before any device is asked
    for tid in range(3):
        want = cp.crossed(sc.R[tid], sc.L[tid], sc.table, sc.refs[tid], tid, *PAR)[0]
        for (t, pr), rows in sc.known.items():
            if t == tid:
                assert [w[1:7] for w in want if w[0] == pr] == rows, (t, pr, [w for w in want if w[0] == pr], rows)
    # the cut's sites are candidates under PAR -- both piles are peaks -- and v(.) of the held right pile is what each site says it is
    m, T, _, _, S, mv = PAR
    code, peaks_r, peaks_l = ct.ref_codes(sc.refs[0]), dict(cp.peaks_many(sc.R[0], m, T)), dict(cp.peaks_many(sc.L[0], m, T))
    reach = {"none": [], "no common shift": [5], "walked, one short": [], "walked, enough": [0]}
    for name, pr in sc.cut.items():
        assert pr in peaks_r and pr - 150 in peaks_l, name
        v1 = cp.shift_counts(sc.table[(0, RIGHT, pr)], code, pr - 150, 1, S)
        assert [s for s in range(S + 1) if v1[s] >= mv] == reach[name], (name, list(v1))
        assert (len(sc.table[(0, RIGHT, pr)]) > 64) == name.startswith("walked"), name          # more than one batch of 64 slots
    v2 = cp.shift_counts(sc.table[(0, LEFT, sc.cut["no common shift"] - 150)], code, sc.cut["no common shift"] - 1, -1, S)
    assert [s for s in range(S + 1) if v2[s] >= mv] == [0]
    return sc


def test_crossed_pairs_made_by_hand(scenario):
    sc = scenario
    log2 = 12
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
        total = check_crossed(dev, sc.R, sc.L, table, PAR, at_least=20)         # 19, and the one pair of the cut's sites
        for tid in range(3):
            got = crossed_of(dev, tid, PAR)
            for (t, pr), rows in sc.known.items():
                if t == tid:
                    assert [g[1:7] for g in got if g[0] == pr] == rows, (t, pr)
        # other parameters: piles of one read, no reach, no shift, a shift that stops in front of the planted ones, every distance, mv above the piles
        for par, n in (((1, 30, 50, 400, 32, 1), 20), ((3, 0, 50, 400, 32, 2), 19), ((3, 64, 50, 400, 0, 2), 10), ((3, 30, 50, 400, 4, 2), 10),
                       ((3, 30, 1, 2_000_000_000, 32, 2), 20), ((3, 30, 120, 120, 32, 3), 5), ((2, 1, 50, 5_000, 31, 64), 0)):
            check_crossed(dev, sc.R, sc.L, table, par, at_least=n)
        # cap below the total: n_found is exact and the call succeeds; with room for all the pairs come sorted by (pr, pl)
        lib, ptr = dev.capi.lib(), lambda a: a.ctypes.data_as(C.c_void_p)
        want = cp.crossed(sc.R[0], sc.L[0], table, sc.refs[0], 0, *PAR)[0]
        assert 15 < len(want) < total and want == sorted(want)
        out, found = [np.zeros(len(want), k) for k in dev.ctx._CROSSED], C.c_int32(-7)
        for cap in (0, 1, len(want) - 1):
            assert lib.im_clip_crossed_tid(dev.ctx.h, 0, *PAR, cap, *[ptr(o) for o in out], C.byref(found)) == 0 and found.value == len(want), cap
        assert lib.im_clip_crossed_tid(dev.ctx.h, 0, *PAR, 0, *[None] * 9, C.byref(found)) == 0 and found.value == len(want)
        assert lib.im_clip_crossed_tid(dev.ctx.h, 0, *PAR, len(want), *[ptr(o) for o in out], C.byref(found)) == 0 and found.value == len(want)
        assert [tuple(int(x) for x in row) for row in zip(*out)] == want
        assert crossed_of(dev, 0, PAR, cap=2) == want               # the binding asks again by itself
        # the build form, contig by contig: the arrays of the last im_clip_build, the table and the reference of the contig named
        for tid in (1, 0, 2):
            pos = np.concatenate([np.repeat(np.arange(CLENS[tid] + 1), sc.R[tid]), np.repeat(np.arange(CLENS[tid] + 1), sc.L[tid])])
            side = np.concatenate([np.zeros(int(sc.R[tid].sum()), np.uint8), np.ones(int(sc.L[tid].sum()), np.uint8)])
            dev.ctx.clip_build(CLENS[tid], pos, side)
            got = [tuple(int(x) for x in row) for row in zip(*dev.ctx.clip_crossed(tid, *PAR))]
            assert got == crossed_of(dev, tid, PAR), tid
            other = (tid + 1) % 3
            assert lib.im_clip_crossed(dev.ctx.h, other, *PAR, 4, *[ptr(o) for o in out], C.byref(found)) != 0 and b"are not contig" in lib.im_last_error(dev.ctx.h)
    finally:
        dev.close()


def test_crossed_more_peaks_than_waves():
    """a contig of 20 000 positions, R 1 on every even position and L 1 on every odd one, m = 1, T = 0, distances 1 .. 5: 10 000 right
    peaks on a grid that is capped at 8 192 waves, two or three partners each; some dozens of planted duplications among them, a third
    with a second partner at shift 2, and many behind the 8 192nd right peak, which only the second round of the grid's loop reaches"""
    from indelminer_amd import capi
    clen = 20_000
    rng = np.random.default_rng(18)
    ref = bytes(rng.choice(np.frombuffer(b"ACGT", np.uint8), clen))
    R, L = np.zeros(clen + 1, np.int64), np.zeros(clen + 1, np.int64)
    R[0:clen:2] = 1; L[1:clen:2] = 1
    table = {}
    sites = list(range(400, 17_000, 400)) + list(range(17_050, 19_950, 100))
    for k, x in enumerate(sites):
        # [x - 3, x) duplicated, and every third time the left pile at x - 5 verifies as well, at shift 2
        table[(0, RIGHT, x)] = [codes(ref, x - 3, 30)]; table[(0, LEFT, x - 3)] = [codes(ref, x - 1, 30, -1)]
        if k % 3 == 0:
            table[(0, LEFT, x - 5)] = [codes(ref, x - 1 - 2, 30, -1)]
    par = (1, 0, 1, 5, 32, 1)
    # The restatement tries every right peak with every left peak.  With T = 0 a peak is a position with a count, whatever stands beside
    # it, so the contig is asked slice by slice: the right peaks of [a, a + 500) and the left peaks they can reach, [a - 5, a + 500).
    want, n_cand = [], 0
    for a in range(0, clen + 1, 500):
        Rs, Ls = np.zeros_like(R), np.zeros_like(L)
        Rs[a:a + 500] = R[a:a + 500]; Ls[max(a - 5, 0):a + 500] = L[max(a - 5, 0):a + 500]
        rows, n = cp.crossed(Rs, Ls, table, ref, 0, *par)
        want += rows; n_cand += n
    assert n_cand > 2 * 8_192 and want == sorted(want) and len(want) >= len(sites) + len(sites) // 3 >= 36
    assert sum(1 for w in want if w[6] == 2) >= len(sites) // 3 and sum(1 for w in want if w[0] >= 17_000) >= 30     # 17 000: the 8 500th right peak
    ctx = capi.Context(0)
    try:
        ctx.set_reference([ref])
        ctx.clip_enable(20, 10)
        ctx.cliptail_enable(20, 10, 12)
        ent = [(p, side, b) for (_, side, p), lst in table.items() for b in lst]
        ctx.cliptail_add(0, [e[0] for e in ent], [e[1] for e in ent], [len(e[2]) for e in ent], np.array([ct.planes_of(e[2]) for e in ent], np.uint32).reshape(-1, 2))
        pos = np.concatenate([np.nonzero(R)[0], np.nonzero(L)[0]])
        ctx.clip_build(clen, pos, np.concatenate([np.zeros(clen // 2, np.uint8), np.ones(clen // 2, np.uint8)]))
        assert len(ctx.clip_peaks(RIGHT, 1, 0)[0]) == len(ctx.clip_peaks(LEFT, 1, 0)[0]) == 10_000
        rows = lambda got: [tuple(int(x) for x in row) for row in zip(*got)]
        assert rows(ctx.clip_crossed(0, *par)) == want
        assert rows(ctx.clip_crossed(0, *par, cap=5)) == want       # cap below the total: the binding asks again
    finally:
        ctx.close()


def test_crossed_table_at_its_smallest_overflow_and_reset():
    """64 slots: two duplications whose keys' home slots are the table's last ones and its first, so the probe runs collide and wrap"""
    refs = contigs()
    homes = {}
    for p in range(1_000, 140_000):
        for side in (RIGHT, LEFT):
            homes.setdefault((side, ct.home_slot(0, side, p, 6)), []).append(p)

    def pick(hr, hl, taken):
        for pr in homes[(RIGHT, hr)]:
            for pl in homes[(LEFT, hl)]:
                if 50 <= pr - pl <= 400 and all(abs(pr - t) > 1_000 for t in taken):
                    return pr, pl
        raise AssertionError("no such pair")

    a = pick(63, 62, [])
    b = pick(61, 0, [a[0]])
    R, L = empty_arrays()
    table = {}
    for (pr, pl), n in ((a, 6), (b, 5)):
        R[0][pr] = L[0][pl] = n
        table[(0, RIGHT, pr)] = [codes(refs[0], pl, 30)] * n
        table[(0, LEFT, pl)] = [codes(refs[0], pr - 1, 30, -1)] * n
    want = [(a[0], a[1], 6, 6, 6, 6, 0, 6, 6), (b[0], b[1], 5, 5, 5, 5, 0, 5, 5)]
    dev = Device(log2_slots=6, refs=refs)
    lib, ptr = dev.capi.lib(), lambda x: x.ctypes.data_as(C.c_void_p)
    try:
        dev.counts(R, L)
        dev.add(table)
        assert dev.ctx.cliptail_stats() == (22, 0)
        assert sorted(want) == cp.crossed(R[0], L[0], table, refs[0], 0, *PAR)[0]
        check_crossed(dev, R, L, table, PAR, at_least=2)
        # 15 more make 37: 32 stored, 5 dropped; no answer, and nothing is written
        dev.add({(1, LEFT, 2_000): [codes(refs[1], 100, 25)] * 15})
        assert dev.ctx.cliptail_stats() == (32, 5)
        assert crossed_of(dev, 0, PAR) is None and crossed_of(dev, 1, PAR) is None
        out, found = [np.full(4, 77, k) for k in dev.ctx._CROSSED], C.c_int32(0)
        assert lib.im_clip_crossed_tid(dev.ctx.h, 0, *PAR, 4, *[ptr(o) for o in out], C.byref(found)) == 0 and found.value == -1
        assert all((o == 77).all() for o in out)
        dev.ctx.cliptail_reset()
        dev.add(table)
        check_crossed(dev, R, L, table, PAR, at_least=2)
    finally:
        dev.close()


def test_crossed_arguments():
    from indelminer_amd import capi
    lib, ptr = capi.lib(), lambda a: a.ctypes.data_as(C.c_void_p)
    out, found = [np.zeros(4, k) for k in capi.Context._CROSSED], C.c_int32(-7)
    args = lambda: [ptr(o) for o in out] + [C.byref(found)]
    ctx = capi.Context(0)
    try:
        ctx.set_reference(contigs())
        assert lib.im_clip_crossed_tid(ctx.h, 0, *PAR, 4, *args()) != 0                 # before im_clip_enable
        ctx.clip_enable(20, 10)
        assert lib.im_clip_crossed_tid(ctx.h, 0, *PAR, 4, *args()) != 0 and lib.im_last_error(ctx.h) == b"im_cliptail_enable has not been called"
        assert lib.im_clip_crossed(ctx.h, 0, *PAR, 4, *args()) != 0 and lib.im_last_error(ctx.h) == b"im_clip_build has not been called"
        ctx.cliptail_enable(20, 10, 6)
        for tid in range(3):
            assert lib.im_clip_crossed_tid(ctx.h, tid, *PAR, 4, *args()) == 0 and found.value == 0          # empty arrays, an empty table
        ctx.clip_build(CLENS[1], np.zeros(0, np.int32), np.zeros(0, np.uint8))
        assert lib.im_clip_crossed(ctx.h, 1, *PAR, 4, *args()) == 0 and found.value == 0
        m, T, dmin, dmax, S, mv = PAR
        for bad, word in (((0, T, dmin, dmax, S, mv, 4), b"min_reads 0"), ((m, 65, dmin, dmax, S, mv, 4), b"reach 65"), ((m, -1, dmin, dmax, S, mv, 4), b"reach -1"),
                          ((m, T, 0, dmax, S, mv, 4), b"min_len 0"), ((m, T, dmin, dmin - 1, S, mv, 4), b"max_len 49"), ((m, T, dmin, dmax, 33, mv, 4), b"max_shift 33"),
                          ((m, T, dmin, dmax, -1, mv, 4), b"max_shift -1"), ((m, T, dmin, dmax, S, 0, 4), b"min_verified 0"), ((m, T, dmin, dmax, S, mv, -1), b"cap -1")):
            assert lib.im_clip_crossed_tid(ctx.h, 0, *bad, *args()) != 0 and word in lib.im_last_error(ctx.h), bad
            assert lib.im_clip_crossed(ctx.h, 1, *bad, *args()) != 0 and word in lib.im_last_error(ctx.h), bad
        assert lib.im_clip_crossed_tid(ctx.h, 3, *PAR, 4, *args()) != 0 and lib.im_clip_crossed_tid(ctx.h, -1, *PAR, 4, *args()) != 0
        assert lib.im_clip_crossed_tid(ctx.h, 0, *PAR, 4, *[ptr(o) for o in out], None) != 0
        for k in range(9):
            holed = [ptr(o) for o in out]; holed[k] = None
            assert lib.im_clip_crossed_tid(ctx.h, 0, *PAR, 4, *holed, C.byref(found)) != 0, k
        assert lib.im_clip_crossed_tid(ctx.h, 0, m, T, dmin, dmin, 0, 1, 0, *[None] * 9, C.byref(found)) == 0 and found.value == 0
    finally:
        ctx.close()


# ------------------------------------------------------------------------------------------ the soak

def soak_records(refs, seed, n_records=20_000, n_hot=300):
    """records with clips at 300 hot positions: 150 duplications [pl, pr) of 50 .. 3 000 bases on two contigs, some sharing a breakpoint's
    neighbourhood, up to 15 reads a side whose clipped bases continue at the other breakpoint at the site's shift (or now and then at
    another), with flipped bases, Ns and low mapping qualities; clipped reads of random bases at random places and at the piles; and the
    many reads that do not clip"""
    from tests.test_gpu_cliptail import M, S, tail_read, with_bases
    rng = np.random.default_rng(seed)
    recs = []
    sites = [(0, int(a), int(w)) for a, w in zip(range(4_000, 146_000, 1_000), rng.integers(50, 3_000, 142))]
    sites += [(1, int(a), int(w)) for a, w in zip(range(300, 4_300, 500), rng.integers(50, 600, 8))]
    assert 2 * len(sites) == n_hot
    for tid, pl, w in sites:
        pr = min(pl + w, CLENS[tid])
        s = int(rng.choice([0, 0, 0, 1, 3, 7, 32, 33]))
        for side in (RIGHT, LEFT):
            for _ in range(int(rng.integers(0, 16))):
                Lc = int(rng.integers(15, 71))
                m = int(rng.integers(10, 81))
                k = int(rng.choice([0, 0, 0, 1, 2, 3]))
                n_at = [int(rng.integers(0, Lc))] if rng.random() < 0.05 else []
                jitter = int(rng.choice([0, 0, 0, 0, 0, 1, 2, 31]))         # a few reads clip beside the pile
                recs.append(tail_read(refs[tid], tid, side, pr + (jitter if side == RIGHT else 0), pl + (jitter if side == LEFT else 0),
                                      s if rng.random() < 0.9 else int(rng.integers(0, 40)), Lc, m,
                                      flips=[int(x) for x in rng.integers(0, min(Lc, 32), k)], n_at=n_at, mapq=int(rng.choice([60, 60, 60, 9, 10]))))
    noise = []
    for _ in range(2_000):
        tid = int(rng.random() < 0.1)
        Lc, m = int(rng.integers(1, 80)), int(rng.integers(1, 90))
        pos = int(rng.integers(0, CLENS[tid] - 100)) if rng.random() < 0.7 else sites[int(rng.integers(0, len(sites)))][1]
        noise.append((tid if pos < CLENS[tid] - 100 else 0, pos, 60, int(rng.choice([0, 0, 0, 0x10, 0x400])), [[(M, m), (S, Lc)], [(S, Lc), (M, m)], [(S, Lc), (M, m), (S, Lc)]][int(rng.integers(0, 3))]))
    recs += with_bases(noise, seed + 1)
    plain = [(int(rng.random() < 0.03), int(rng.integers(0, 4_800)), 60, 0, [(M, 100)]) for _ in range(n_records - len(recs))]
    recs += with_bases(plain, seed + 2)
    order = rng.permutation(len(recs))
    return [recs[int(k)] for k in order]


def test_crossed_seeded_soak_scatter_against_add_and_the_build_form():
    """20 000 records through im_dev_clip_scatter and im_dev_cliptail_scatter in three launches, both record forms, against the same
    events through im_clip_build and im_cliptail_add"""
    c, q = 20, 10
    refs = contigs()
    recs = soak_records(refs, 11)
    assert len(recs) == 20_000
    cuts = [0, 7_000, 13_001, len(recs)]
    parsed = []
    pars = ((3, 30, 50, 3_000, 32, 2), (2, 5, 50, 1_500, 32, 1), (3, 30, 300, 100_000, 8, 3))
    answers = []
    dev = Device(c, q, log2_slots=14, refs=refs)
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
        assert 1_500 < sum(len(v) for v in table.values()) < 8_192 and max(len(v) for v in table.values()) >= 10
        assert check_crossed(dev, R, L, table, pars[0], at_least=40) > check_crossed(dev, R, L, table, pars[2], at_least=15)
        check_crossed(dev, R, L, table, pars[1], at_least=30)
        want = cp.crossed(R[0], L[0], table, refs[0], 0, *pars[0])[0]
        assert sum(1 for w in want if w[6] > 0) >= 5 and sum(1 for w in want if w[4] < w[7] or w[5] < w[8]) >= 10       # shifts, and piles that verify in part
        answers.append([crossed_of(dev, tid, par) for par in pars for tid in range(3)])
    finally:
        dev.close()
    dev = Device(c, q, log2_slots=14, refs=refs)
    try:
        dev.add(table)
        got = []
        for par in pars:
            for tid in range(3):
                pos = np.concatenate([np.repeat(np.arange(CLENS[tid] + 1), R[tid]), np.repeat(np.arange(CLENS[tid] + 1), L[tid])])
                side = np.concatenate([np.zeros(int(R[tid].sum()), np.uint8), np.ones(int(L[tid].sum()), np.uint8)])
                dev.ctx.clip_build(CLENS[tid], pos, side)
                got.append([tuple(int(x) for x in row) for row in zip(*dev.ctx.clip_crossed(tid, *par))])
        answers.append(got)
    finally:
        dev.close()
    assert answers[0] == answers[1] and sum(len(x) for x in answers[0]) > 90


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
    from tests.test_gpu_depth_evidence import depth_of_bam
    refs, rd = cp.planted_reads()
    d = cp.write_planted(str(tmp_path_factory.mktemp("crossed_planted")), refs, rd)
    text, recs, n_cand, n_peaks = cp.render_of_bam(d + "/aln.bam", d + "/ref.fa", 10)
    names, depth = depth_of_bam(d + "/aln.bam")
    text_d = cp.render_of_bam(d + "/aln.bam", d + "/ref.fa", 10, depth)[0]
    return d, text, text_d, recs, n_cand, n_peaks


BASE = ["-i", "cfg.txt", "-s", "100"]


def test_product_tandem_duplications(planted, tmp_path):
    d, text, text_d, recs, n_cand, n_peaks = planted
    prod = _product()
    # the figures of the planted data set, from the restatement (tests/test_crossed_host.py has them without a GPU)
    assert len(cp.SITES) >= 8 and n_peaks == (19, 19) and n_cand == 182 and [(r[2], r[1] - r[2]) for r in recs] == cp.SITES
    f = str(tmp_path / "dup.vcf")
    gcv = _ok(_run(prod, BASE + ["-G", "-C", "-V"], d))
    gcvu = _ok(_run(prod, BASE + ["-G", "-C", "-V", "-U", f], d))
    got = open(f, "rb").read()
    assert got == text                                              # FILE is the restatement's rendering, byte for byte
    assert gcvu.stdout == gcv.stdout and gcvu.stderr == gcv.stderr and len(gcv.stdout) > 1000       # stdout and stderr do not know about -U
    for pl, n in cp.SITES:                                          # every planted site is in FILE
        assert sum(1 for ln in got.decode().split("\n") if ln.startswith("ctg0\t%d\t" % pl) and ";END=%d;SVLEN=%d;" % (pl + n, n) in ln) == 1, (pl, n)
    # the record-at-a-time path and three walkers on small pieces write the same bytes
    envs = ({"INDELMINER_PIPELINE": "host"}, {"INDELMINER_PIECE_BYTES": "60000", "INDELMINER_WALKERS": "3"})
    for k, env in enumerate(envs):
        fk = str(tmp_path / ("dup%d.vcf" % k))
        r = _ok(_run(prod, BASE + ["-G", "-C", "-V", "-U", fk], d, env=env))
        assert open(fk, "rb").read() == text and r.stdout == gcv.stdout, env
    # with -D every record gains DM and DFC, on all three paths; stdout is that of -G -D -C -V
    gdcv = _ok(_run(prod, BASE + ["-G", "-D", "-C", "-V"], d))
    assert text_d != text and text_d.count(b";DM=") == len(recs) and text_d.count(b";DFC=") == len(recs)
    for k, env in enumerate(({},) + envs):
        fk = str(tmp_path / ("dupd%d.vcf" % k))
        r = _ok(_run(prod, BASE + ["-G", "-D", "-C", "-V", "-U", fk], d, env=env))
        assert open(fk, "rb").read() == text_d and r.stdout == gdcv.stdout, env
    # with -I beside it: both files are what they are alone
    fi, fi2, fu2 = str(tmp_path / "ins.vcf"), str(tmp_path / "ins2.vcf"), str(tmp_path / "dup2.vcf")
    _ok(_run(prod, BASE + ["-G", "-C", "-V", "-I", fi], d))
    for env in ({},) + envs[:1]:
        r = _ok(_run(prod, BASE + ["-G", "-C", "-V", "-I", fi2, "-U", fu2], d, env=env))
        assert open(fu2, "rb").read() == text and open(fi2, "rb").read() == open(fi, "rb").read() and r.stdout == gcv.stdout, env
    # -o detailed ignores -U and writes no FILE; without -V it is refused
    fd = str(tmp_path / "none.vcf")
    d0 = _ok(_run(prod, BASE + ["-o", "detailed"], d))
    d1 = _ok(_run(prod, BASE + ["-o", "detailed", "-G", "-C", "-V", "-U", fd], d))
    assert d1.stdout == d0.stdout and d1.stderr == d0.stderr and len(d0.stdout) > 0 and not os.path.exists(fd)
    r = _run(prod, BASE + ["-G", "-C", "-U", fd], d)
    assert r.returncode != 0 and r.stdout == b"" and b"indelminer: -U needs -V" in r.stderr and not os.path.exists(fd)


def test_product_mapping_quality_gates_the_piles(tmp_path):
    """every second clipped read gets mapping quality 20: at -q 30 the piles are half as high, and fewer pairs qualify"""
    refs, rd = cp.planted_reads()
    d = cp.write_planted(str(tmp_path), refs, rd, lower_mapq_of_every_second_clipped_read=True)
    prod = _product()
    n = {}
    for q in (10, 30):
        text, recs, _, _ = cp.render_of_bam(d + "/aln.bam", d + "/ref.fa", q)
        f = str(tmp_path / ("dup_q%d.vcf" % q))
        _ok(_run(prod, BASE + ["-q", str(q), "-G", "-C", "-V", "-U", f], d))
        assert open(f, "rb").read() == text, q
        n[q] = len(recs)
    assert n[10] == len(cp.SITES) and 0 < n[30] < n[10], n
