"""Large insertions from facing clip piles (-I): the chip-wide search of im_span.hip's clip_facing_kernel, the per-base consensus of
im_cliptail.hip's cliptail_consensus_kernel, and what the host driver makes of them (-I FILE).

The yardstick is the plain restatement in tests/support/facingpiles.py, written from the definitions in include/indelminer_amd.h (seam 5,
"Facing piles" and "The consensus of a pile"), not from the code under test; tests/test_facing_host.py pins it to cases worked by hand.
Every answer is compared exactly.
"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests.support import clipcounts as cc
from tests.support import cliptails as ct
from tests.support import facingpiles as fp
from tests.support.clipcounts import LEFT, RIGHT
from tests.support.spanarrays import _product

pytestmark = pytest.mark.gpu

M, S = 0, 4
CLENS = [150_000, 5_000, 70]
NONE = 0xFFFFFFFF
# the shape of clip_facing_kernel: a lane takes 4 positions, a wave 256, a workgroup 1 024 per load and 4 loads, 4 096 in all
LANE, WAVE, SWEEP, TILE = 4, 256, 1_024, 4_096


def contigs(seed=3):
    rng = np.random.default_rng(seed)
    return [bytes(rng.choice(np.frombuffer(b"ACGT", np.uint8), n)) for n in CLENS]


class Device:
    """one context over three contigs with the clip arrays enabled, and the clip-tail table where log2_slots is given"""

    def __init__(self, c=20, q=10, log2_slots=None, refs=None):
        from indelminer_amd import capi
        self.capi = capi
        self.refs = refs or contigs()
        self.ctx = capi.Context(0)
        self.ctx.set_reference(self.refs)
        self.ctx.clip_enable(c, q)
        if log2_slots is not None:
            self.ctx.cliptail_enable(c, q, log2_slots)
        self.keep = []

    def records(self, raw, off):
        capi = self.capi
        d_raw = capi.DevBuf(self.ctx, len(raw) + 64).upload(raw)
        d_off = capi.DevBuf(self.ctx, 4 * len(off)).upload(off)
        self.keep += [d_raw, d_off]
        return capi.DevRecords(len(off) - 1, d_raw.ptr, d_off.ptr, 0)

    def sync(self):
        self.ctx._check(self.capi.lib().im_stream_sync(self.ctx.h, self.ctx.stream))

    def counts(self, right, left):
        """the two arrays of every contig through im_dev_clip_scatter, as hand-made records: R[p] right clips that end in front of p,
        L[p] left clips that start at p"""
        recs = []
        for tid in range(len(CLENS)):
            for p in np.nonzero(right[tid])[0]:
                recs += [(tid, int(p) - 50, 60, 0, [(M, 50), (S, 30)])] * int(right[tid][p])      # a negative pos is legal: refend counts
            for p in np.nonzero(left[tid])[0]:
                recs += [(tid, int(p), 60, 0, [(S, 30), (M, 50)])] * int(left[tid][p])
        from tests.test_gpu_clip import raw_records
        for tid in range(len(CLENS)):
            self.ctx.clip_reset(tid)
        if recs:
            self.ctx.clip_scatter(self.records(*raw_records(recs, qual=False)))
        self.sync()
        assert cc.arrays_of(recs, CLENS, 20, 10)[0][0].sum() == right[0].sum()

    def facing(self, tid, m, T, cap=65536):
        return [tuple(int(x) for x in row) for row in zip(*self.ctx.clip_facing_tid(tid, m, T, cap))]

    def check_facing(self, right, left, m, T, at_least=0):
        n = 0
        for tid in range(len(CLENS)):
            want = fp.facing_many(right[tid], left[tid], m, T)
            if len(right[tid]) <= 5_001:
                assert fp.facing(right[tid], left[tid], m, T) == want           # the fast form against the plain one
            got = self.facing(tid, m, T)
            assert got == want, (tid, m, T, [x for x in got if x not in want][:8], [x for x in want if x not in got][:8])
            n += len(want)
        assert n >= at_least, n
        return n

    def add(self, table):
        """a restatement table {(tid, side, position): [bases]} through im_cliptail_add, one call per contig"""
        for tid in range(len(self.refs)):
            ent = [(p, side, b) for (t, side, p), lst in table.items() if t == tid for b in lst]
            self.ctx.cliptail_add(tid, [e[0] for e in ent], [e[1] for e in ent], [len(e[2]) for e in ent],
                                  np.array([ct.planes_of(e[2]) for e in ent], np.uint32).reshape(-1, 2))

    def consensus(self, tid, pos, side, c):
        self.sync()
        return [tuple(int(x) for x in row) for row in zip(*self.ctx.cliptail_consensus(tid, pos, side, c))]

    def check_consensus(self, table, queries, covers=(1, 2, 3)):
        """queries: [(tid, side, position)]; every answer against the restatement, for every min_cover"""
        for tid in range(len(self.refs)):
            qs = [(side, p) for t, side, p in queries if t == tid]
            if not qs:
                continue
            for c in covers:
                want = [fp.answer(table, tid, p, side, c, CLENS[tid]) for side, p in qs]
                got = self.consensus(tid, [p for _, p in qs], [side for side, _ in qs], c)
                bad = [k for k in range(len(qs)) if got[k] != want[k]]
                assert not bad, (tid, c, [(qs[k], got[k], want[k]) for k in bad[:8]])

    def close(self):
        for b in self.keep:
            b.free()
        self.ctx.close()


def empty_arrays():
    return [np.zeros(n + 1, np.int64) for n in CLENS], [np.zeros(n + 1, np.int64) for n in CLENS]


# ------------------------------------------------------------------------------------------ facing piles

def named_cases(T, m=3):
    """(right, left, what some positions must answer whatever the restatement says) for max_overlap T"""
    R, L = empty_arrays()
    c0, c1, c2 = CLENS
    known = {}
    at = iter(range(2_000, 140_000, 700))
    # equal peaks at distance T (the left one wins) and at distance T + 1 (both are piles)
    a = next(at); R[0][a] = R[0][a + T] = 4; L[0][a] = L[0][a + T] = m; known[(0, a)] = (a, 4, m); known[(0, a + T)] = None if T else (a, 4, m)
    a = next(at); R[0][a] = R[0][a + T + 1] = 4; L[0][a] = L[0][a + T + 1] = m; known[(0, a)] = (a, 4, m); known[(0, a + T + 1)] = (a + T + 1, 4, m)
    # a higher peak T to the right, and one T + 1 to the right
    if T:
        a = next(at); R[0][a] = 4; R[0][a + T] = 5; L[0][a] = m; known[(0, a)] = None; known[(0, a + T)] = (a, 5, m)
    a = next(at); R[0][a] = 4; R[0][a + T + 1] = 5; L[0][a] = m; known[(0, a)] = (a, 4, m); known[(0, a + T + 1)] = None
    # a partner at exactly p - T and one at p - T - 1
    a = next(at); R[0][a] = m; L[0][a - T] = m; known[(0, a)] = (a - T, m, m)
    a = next(at); R[0][a] = m; L[0][a - T - 1] = m; known[(0, a)] = None
    # two equal partners (the larger x wins), a larger one further away, pl = pr
    if T >= 2:
        a = next(at); R[0][a] = m; L[0][a - 2] = L[0][a - 1] = m + 1; known[(0, a)] = (a - 1, m, m + 1)
        a = next(at); R[0][a] = m; L[0][a - 2] = m + 2; L[0][a - 1] = m + 1; known[(0, a)] = (a - 2, m, m + 2)
    a = next(at); R[0][a] = m; L[0][a] = m; known[(0, a)] = (a, m, m)
    # counts of m and m - 1 on either side; a left pile behind the right pile (a deletion's) is no partner
    a = next(at); R[0][a] = m - 1; L[0][a] = m; known[(0, a)] = None
    a = next(at); R[0][a] = m; L[0][a] = m - 1; known[(0, a)] = None
    a = next(at); R[0][a] = m; L[0][a + 1] = m + 5; known[(0, a)] = None
    # piles at 0 and at clen
    R[0][0] = m; L[0][0] = m; known[(0, 0)] = (0, m, m)
    R[1][0] = m + 1; L[1][0] = m; known[(1, 0)] = (0, m + 1, m)
    # a pile on the last entry of contig 0 with a larger pile on the first entries of contig 1: nothing leaks across the boundary
    R[0][c0] = m; L[0][c0] = m; known[(0, c0)] = (c0, m, m)
    R[1][1] = m + 6; L[1][1] = m + 6
    known[(1, 1)] = (1, m + 6, m + 6)
    if T:
        known[(1, 0)] = None                                        # hidden by its own contig's larger pile, not by contig 0's
    # ... and the reverse: the larger pile at the end of contig 1, a pile on the first entry of contig 2
    R[1][c1] = m + 7; L[1][c1 - 1] = m if T else 0; L[1][c1] = 0 if T else m; known[(1, c1)] = (c1 - 1 if T else c1, m + 7, m)
    R[2][0] = m; L[2][0] = m + 1; known[(2, 0)] = (0, m, m + 1)
    # the 70-base contig, whose whole run is shorter than one window
    R[2][40] = m + 1; L[2][40 - min(T, 35)] = m
    known[(2, 40)] = (40 - min(T, 35), m + 1, m)
    if T >= 40:
        known[(2, 0)] = None                                        # the larger pile at 40 is within reach and hides position 0 ...
        known[(2, 40)] = (0, m + 1, m + 1)                          # ... and its partner is the larger left pile there
    return R, L, known


@pytest.mark.parametrize("T", [30, 0, 64, 1])
def test_facing_piles_and_partners(T):
    R, L, known = named_cases(T)
    dev = Device()
    try:
        dev.counts(R, L)
        for m in (3, 1, 4):
            dev.check_facing(R, L, m, T, at_least=6 if m <= 3 else 1)
        for tid in range(3):
            got = {pr: (pl, cr, cl) for pr, pl, cr, cl in dev.facing(tid, 3, T)}
            for (t, p), want in known.items():
                if t == tid:
                    assert got.get(p) == want, (T, t, p, got.get(p), want)
    finally:
        dev.close()


def boundary_cases(T, delta):
    """piles whose four-position group and whose windows straddle the kernel's lane, wave, load and workgroup boundaries, at delta"""
    R, L = empty_arrays()
    for b in (LANE * 25, WAVE, SWEEP, SWEEP + WAVE * 3, TILE, TILE + SWEEP, 2 * TILE, 17 * TILE + 3 * SWEEP, 36 * TILE, 146 * SWEEP):
        p = b + delta
        R[0][p] = 4; L[0][p - T] = 3                                # the partner window reaches back across the boundary
        R[0][p + T] = 4                                             # an equal peak T behind: hidden, its own window reaches back across
        R[0][p - T - 1] = 6; L[0][p - T - 1] = 4                    # a pile just out of reach in front
        R[0][p + 2 * T + 1] = 3; L[0][p + 2 * T + 1 - (T // 2)] = 5
    for b in (SWEEP, TILE):                                         # contig 1 has one workgroup boundary, and ends inside a four-position group
        p = b + delta
        R[1][p] = 3; L[1][p - T] = 3; R[1][p - 1] = 2; R[1][p + 1] = 3
    R[1][CLENS[1]] = 5; L[1][CLENS[1] - T] = 3; R[1][CLENS[1] - 1] = 5
    return R, L


@pytest.mark.parametrize("T", [30, 64, 0])
def test_facing_kernel_boundaries(T):
    dev = Device()
    try:
        for delta in (-1, 0, 1, 3):
            R, L = boundary_cases(T, delta)
            dev.counts(R, L)
            dev.check_facing(R, L, 3, T, at_least=20)
    finally:
        dev.close()


def hot_arrays(seed, n_records=20_000, n_hot=300):
    """the two arrays of clipped records concentrated on hot positions of all three contigs, neighbours and equal counts included"""
    rng = np.random.default_rng(seed)
    R, L = empty_arrays()
    hot = [(0, int(p)) for p in rng.integers(0, CLENS[0] + 1, n_hot - 60)] + [(1, int(p)) for p in rng.integers(0, CLENS[1] + 1, 50)] + \
          [(2, int(p)) for p in rng.integers(0, CLENS[2] + 1, 10)] + [(0, 0), (0, CLENS[0]), (1, CLENS[1]), (2, CLENS[2]), (0, TILE), (0, TILE - 1)]
    weight = rng.integers(1, 12, len(hot)).astype(np.float64)
    pick = rng.choice(len(hot), n_records, p=weight / weight.sum())
    jitter = rng.choice([0, 0, 0, 0, 1, 2, 7, 29, 30, 31, 63, 64, 65], n_records)
    side = rng.integers(0, 2, n_records)
    for k, j, s in zip(pick, jitter, side):
        tid, p = hot[int(k)]
        p = p - int(j) if s == LEFT else p + int(j) % 3             # left clips stand up to 65 in front, right clips beside the hot position
        (L if s == LEFT else R)[tid][min(max(p, 0), CLENS[tid])] += 1
    return R, L


def test_facing_seeded_soak_cap_and_the_build_form():
    R, L = hot_arrays(23)
    assert sum(int(a.sum()) for a in R + L) == 20_000
    dev = Device()
    try:
        dev.counts(R, L)
        n = dev.check_facing(R, L, 3, 30, at_least=150)
        dev.check_facing(R, L, 3, 64, at_least=100)
        dev.check_facing(R, L, 1, 0, at_least=n)
        dev.check_facing(R, L, 20, 30)
        # cap smaller than the total: n_found is exact, the call succeeds; a second call with enough room answers
        lib, ptr = dev.capi.lib(), lambda a: a.ctypes.data_as(C.c_void_p)
        want = fp.facing_many(R[0], L[0], 3, 30)
        assert len(want) > 100
        out, found = [np.zeros(len(want), np.int32 if k < 2 else np.uint32) for k in range(4)], C.c_int32(-1)
        for cap in (0, 1, len(want) - 1):
            assert lib.im_clip_facing_tid(dev.ctx.h, 0, 3, 30, cap, *[ptr(o) for o in out], C.byref(found)) == 0 and found.value == len(want), cap
        assert lib.im_clip_facing_tid(dev.ctx.h, 0, 3, 30, 0, None, None, None, None, C.byref(found)) == 0 and found.value == len(want)
        assert lib.im_clip_facing_tid(dev.ctx.h, 0, 3, 30, len(want), *[ptr(o) for o in out], C.byref(found)) == 0 and found.value == len(want)
        assert [tuple(int(x) for x in row) for row in zip(*out)] == want
        assert dev.facing(0, 3, 30, cap=7) == want                  # the binding asks again by itself
        # im_clip_build + im_clip_facing: the record-at-a-time form, contig by contig
        for tid in (1, 0, 2):
            pos = np.concatenate([np.repeat(np.arange(CLENS[tid] + 1), R[tid]), np.repeat(np.arange(CLENS[tid] + 1), L[tid])])
            side = np.concatenate([np.zeros(int(R[tid].sum()), np.uint8), np.ones(int(L[tid].sum()), np.uint8)])
            dev.ctx.clip_build(CLENS[tid], pos, side)
            for m, T in ((3, 30), (1, 0), (3, 64)):
                got = [tuple(int(x) for x in row) for row in zip(*dev.ctx.clip_facing(m, T))]
                assert got == dev.facing(tid, m, T) == fp.facing_many(R[tid], L[tid], m, T), (tid, m, T)
    finally:
        dev.close()


def test_facing_empty_arrays_and_arguments():
    from indelminer_amd import capi
    lib, ptr = capi.lib(), lambda a: a.ctypes.data_as(C.c_void_p)
    out, found = [np.zeros(4, np.int32 if k < 2 else np.uint32) for k in range(4)], C.c_int32(-1)
    args = lambda: [ptr(o) for o in out] + [C.byref(found)]
    ctx = capi.Context(0)
    try:
        ctx.set_reference(contigs())
        assert lib.im_clip_facing_tid(ctx.h, 0, 3, 30, 4, *args()) != 0         # before im_clip_enable
        assert lib.im_clip_facing(ctx.h, 3, 30, 4, *args()) != 0 and lib.im_last_error(ctx.h) == b"im_clip_build has not been called"
        ctx.clip_enable(20, 10)
        for tid in range(3):
            for m, T in ((1, 0), (3, 30), (3, 64)):
                assert lib.im_clip_facing_tid(ctx.h, tid, m, T, 4, *args()) == 0 and found.value == 0, (tid, m, T)
        ctx.clip_build(1_000, np.zeros(0, np.int32), np.zeros(0, np.uint8))
        assert lib.im_clip_facing(ctx.h, 1, 0, 4, *args()) == 0 and found.value == 0
        for bad, word in (((0, 0, 30, 4), b"min_reads 0"), ((0, 3, 65, 4), b"max_overlap 65"), ((0, 3, -1, 4), b"max_overlap -1"), ((0, 3, 30, -1), b"cap -1")):
            assert lib.im_clip_facing_tid(ctx.h, *bad, *args()) != 0 and word in lib.im_last_error(ctx.h), bad
            assert lib.im_clip_facing(ctx.h, *bad[1:], *args()) != 0 and word in lib.im_last_error(ctx.h), bad
        assert lib.im_clip_facing_tid(ctx.h, 3, 3, 30, 4, *args()) != 0 and lib.im_clip_facing_tid(ctx.h, -1, 3, 30, 4, *args()) != 0
        assert lib.im_clip_facing_tid(ctx.h, 0, 3, 30, 4, *[ptr(o) for o in out], None) != 0
        assert lib.im_clip_facing_tid(ctx.h, 0, 3, 30, 4, None, *[ptr(o) for o in out[1:]], C.byref(found)) != 0
        one, side = np.zeros(1, np.int32), np.zeros(1, np.uint8)
        res = [np.zeros(2, np.uint32) for _ in range(4)]
        assert lib.im_cliptail_consensus(ctx.h, 0, 1, ptr(one), ptr(side), 2, *[ptr(o) for o in res]) != 0
        assert lib.im_last_error(ctx.h) == b"im_cliptail_enable has not been called"
        ctx.cliptail_enable(20, 10, 6)
        assert lib.im_cliptail_consensus(ctx.h, 0, 1, ptr(one), ptr(side), 0, *[ptr(o) for o in res]) != 0 and b"min_cover 0" in lib.im_last_error(ctx.h)
        assert lib.im_cliptail_consensus(ctx.h, 3, 1, ptr(one), ptr(side), 2, *[ptr(o) for o in res]) != 0
        assert lib.im_cliptail_consensus(ctx.h, 0, 1, None, ptr(side), 2, *[ptr(o) for o in res]) != 0
        assert lib.im_cliptail_consensus(ctx.h, 0, 1, ptr(one), ptr(np.full(1, 2, np.uint8)), 2, *[ptr(o) for o in res]) != 0 and b"side 2" in lib.im_last_error(ctx.h)
        assert lib.im_cliptail_consensus(ctx.h, 0, 0, None, None, 2, None, None, None, None) == 0
        assert lib.im_cliptail_consensus(ctx.h, 0, 1, ptr(one), ptr(side), 2, *[ptr(o) for o in res]) == 0 and [int(o[0]) for o in res] == [0, 0, 0, 0]
    finally:
        ctx.close()


# ------------------------------------------------------------------------------------------ the consensus

def random_entries(rng, n, lo=1, hi=32, base=None, flips=(0, 0, 0, 1, 2, 3)):
    """n entries of lo .. hi bases: `base` with a few bases changed, or random ones"""
    out = []
    for _ in range(n):
        k = int(rng.integers(lo, hi + 1))
        e = list(base[:k]) if base is not None else [int(x) for x in rng.integers(0, 4, k)]
        for i in rng.integers(0, k, int(rng.choice(flips))):
            e[int(i)] = (e[int(i)] + 1 + int(rng.integers(0, 3))) % 4
        out.append(tuple(e))
    return out


def queries_of(table):
    """every key of the table, the other side at the same position, and a neighbour nobody clips at"""
    qs = set()
    for tid, side, p in table:
        qs |= {(tid, side, p), (tid, 1 - side, p), (tid, side, p + 1)}
    return sorted(qs)


def test_consensus_table_at_its_smallest_and_overflow():
    rng = np.random.default_rng(51)
    # 64 slots: 5 keys whose home slots are the last four and the first, 6 entries each: collisions, and runs that wrap past slot 63
    homes = {}
    for p in range(1_000, 140_000):
        for side in (RIGHT, LEFT):
            homes.setdefault(ct.home_slot(0, side, p, 6), []).append((side, p))
    picked = [homes[h][k] for h, k in ((63, 0), (62, 0), (63, 1), (61, 0), (0, 0))]
    table = {}
    for side, p in picked:
        base = [int(x) for x in rng.integers(0, 4, 32)]
        table[(0, side, p)] = random_entries(rng, 6, 20, 32, base)
    dev = Device(log2_slots=6)
    try:
        dev.add(table)
        assert dev.ctx.cliptail_stats() == (30, 0)
        dev.check_consensus(table, queries_of(table), covers=(1, 2, 6, 7))
        # 10 more make 40: 32 stored, 8 dropped; every output is the no-answer value, and the call returns
        dev.add({(1, LEFT, 2_000): random_entries(rng, 10)})
        assert dev.ctx.cliptail_stats() == (32, 8)
        qs = [(side, p) for _, side, p in table]
        assert dev.consensus(0, [p for _, p in qs], [s for s, _ in qs], 2) == [(NONE,) * 5] * len(qs)
        assert dev.consensus(1, [2_000, -4], [LEFT, LEFT], 1) == [(NONE,) * 5] * 2
        dev.ctx.cliptail_reset()
        dev.add(table)
        dev.check_consensus(table, queries_of(table))
    finally:
        dev.close()


def test_consensus_pile_sizes_cover_ties_and_tolerance():
    rng = np.random.default_rng(52)
    A, C_, G, T = 0, 1, 2, 3
    table, at = {}, iter(range(3_000, 140_000, 911))
    # piles of 1, 2, 63, 64, 65 and 130 entries: the batch edges of the 64-slot walk; mixed n from 20 to 32, cover falls inside the bases
    for n in (1, 2, 63, 64, 65, 130):
        base = [int(x) for x in rng.integers(0, 4, 32)]
        table[(0, RIGHT if n % 2 else LEFT, next(at))] = random_entries(rng, n, 20, 32, base)
    # short entries only: len stays below 32 whatever min_cover; entries of 1 .. 32 random bases: majorities of 2 or 3 and many ties
    table[(0, RIGHT, next(at))] = random_entries(rng, 9, 1, 12)
    table[(1, LEFT, 77)] = random_entries(rng, 40, 1, 32)
    # a 2 : 2 tie on every base, for every pair of codes: the smaller code
    p = next(at)
    pairs = [(a, b) for a in range(4) for b in range(4) if a < b]
    table[(0, RIGHT, p)] = [tuple(a for a, _ in pairs)] * 2 + [tuple(b for _, b in pairs)] * 2
    known = {(0, RIGHT, p): (4, 6, ct.planes_of([a for a, _ in pairs]), 2)}
    # the other side at the same position holds something else
    table[(0, LEFT, p)] = [(T, T, T, G)] * 3
    known[(0, LEFT, p)] = (3, 4, ct.planes_of((T, T, T, G)), 3)
    # an entry exactly at the tolerance and one beyond it: 2 and 3 of 32, 1 and 2 of 20, 0 and 1 of 15
    base = tuple(int(x) for x in rng.integers(0, 4, 32))
    flip = lambda t, where: tuple((b + 1) % 4 if i in where else b for i, b in enumerate(t))
    p = next(at)
    table[(0, LEFT, p)] = [base] * 5 + [flip(base, (0, 31)), flip(base, (0, 15, 31)), flip(base[:20], (19,)), flip(base[:20], (0, 19)), base[:15], flip(base[:15], (14,))]
    known[(0, LEFT, p)] = (11, 32, ct.planes_of(base), 5 + 1 + 0 + 1 + 0 + 1 + 0)
    # a foreign key interleaved in the same probe run: its home slot lies three behind, and the entries of the two arrive in turns
    log2 = 10
    h = ct.home_slot(0, RIGHT, 60_000, log2)
    foreign = next((side, q) for q in range(1_000, 140_000) for side in (RIGHT, LEFT) if ct.home_slot(0, side, q, log2) == (h + 3) % 1024)
    mine, theirs = random_entries(rng, 12, 20, 32, [int(x) for x in rng.integers(0, 4, 32)]), random_entries(rng, 12, 20, 32, [int(x) for x in rng.integers(0, 4, 32)])
    dev = Device(log2_slots=log2)
    try:
        for k in range(0, 12, 3):
            dev.add({(0, RIGHT, 60_000): mine[k:k + 3]})
            dev.add({(0, foreign[0], foreign[1]): theirs[k:k + 3]})
        dev.add(table)
        table[(0, RIGHT, 60_000)] = mine
        table[(0, foreign[0], foreign[1])] = theirs
        assert dev.ctx.cliptail_stats() == (sum(len(v) for v in table.values()), 0)
        for key, (n, ln, (lo, hi), agree) in known.items():
            assert fp.answer(table, *key[:1], key[2], key[1], 2, CLENS[key[0]]) == (n, ln, lo, hi, agree), key
        # c = 1, c = 2, c inside the piles, c above |E| (len 0, agree 0); a key with no entries; positions outside the contig
        dev.check_consensus(table, queries_of(table) + [(0, RIGHT, 5), (0, LEFT, CLENS[0]), (0, RIGHT, CLENS[0] + 1), (0, LEFT, -1), (2, RIGHT, 70), (2, LEFT, 71)],
                            covers=(1, 2, 3, 5, 12, 64, 65, 131))
        assert dev.consensus(0, [p], [LEFT], 12) == [(11, 0, 0, 0, 0)]
    finally:
        dev.close()


def test_consensus_seeded_soak_and_add_gives_the_answers_of_the_scatter():
    """20 000 records with random clips through im_dev_cliptail_scatter in three launches, both record forms; every pile of either side is
    queried.  Then the same entries through im_cliptail_add."""
    from tests.test_gpu_cliptail import soak_records
    c, q = 20, 10
    refs = contigs()
    recs, _ = soak_records(refs, 7)
    assert len(recs) == 20_000
    cuts = [0, 7_000, 13_001, len(recs)]
    parsed, answers = [], []
    dev = Device(c, q, log2_slots=14, refs=refs)
    try:
        for k in range(3):
            raw, off = ct.pack_records(recs[cuts[k]:cuts[k + 1]], qual=k != 1)
            parsed += ct.parse_raw(raw, off)
            dev.ctx.cliptail_scatter(dev.records(raw, off))
        table = ct.table_of(parsed, CLENS, c, q)
        assert 1_500 < sum(len(v) for v in table.values()) < 8_192 and max(len(v) for v in table.values()) >= 10
        qs = queries_of(table)
        want = [fp.answer(table, t, p, side, 2, CLENS[t]) for t, side, p in qs]
        assert sum(1 for w in want if w[1] == 32) >= 20 and sum(1 for w in want if 0 < w[1] < 32) >= 20 and sum(1 for w in want if 0 < w[4] < w[0]) >= 10
        answers.append([dev.consensus(t, [p for tt, _, p in qs if tt == t], [s for tt, s, _ in qs if tt == t], 2) for t in range(2)])
        got = answers[0][0] + answers[0][1]                         # qs is sorted by contig, and contig 2 has no records
        bad = [k for k in range(len(qs)) if got[k] != want[k]]
        assert len(got) == len(qs) and not bad, [(qs[k], got[k], want[k]) for k in bad[:8]]
        dev.check_consensus(table, qs[::10], covers=(1, 3))
    finally:
        dev.close()
    dev = Device(c, q, log2_slots=14, refs=refs)
    try:
        dev.add(table)
        answers.append([dev.consensus(t, [p for tt, _, p in qs if tt == t], [s for tt, s, _ in qs if tt == t], 2) for t in range(2)])
    finally:
        dev.close()
    assert answers[0] == answers[1] and sum(len(x) for x in answers[0]) == len(qs) > 300


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
    refs, rd, insertions = fp.planted_reads()
    d = fp.write_planted(str(tmp_path_factory.mktemp("facing_planted")), refs, rd)
    text, recs, table = fp.render_of_bam(d + "/aln.bam", d + "/ref.fa", 10)
    return d, text, recs, table, insertions


BASE = ["-i", "cfg.txt", "-s", "100"]


def test_product_large_insertions(planted, tmp_path):
    d, text, recs, table, insertions = planted
    prod = _product()
    # the figures of the planted data set, from the restatement (tests/test_facing_host.py has them without a GPU)
    sites = dict(fp.SITES)
    assert len(recs) == 18 and [r[1] - r[2] for r in recs if r[1] in sites] == [0, 3, 6, 9, 12, 15, 24, 27]
    assert [r[1] - r[2] for r in recs if r[1] not in sites] == [0] * 10
    assert (sum(len(v) for v in table.values()), len(table)) == (276, 41)
    f = str(tmp_path / "ins.vcf")
    gcv = _ok(_run(prod, BASE + ["-G", "-C", "-V"], d))
    gcvi = _ok(_run(prod, BASE + ["-G", "-C", "-V", "-I", f], d))
    got = open(f, "rb").read()
    assert got == text                                              # FILE is the restatement's rendering, byte for byte
    assert gcvi.stdout == gcv.stdout and gcvi.stderr == gcv.stderr and len(gcv.stdout) > 1000      # stdout and stderr do not know about -I
    # at the site without a duplication LSEQ / RSEQ are the planted insertion's first and last bases
    (line,) = [ln for ln in got.decode().split("\n") if ln.startswith("ctg0\t%d\t" % fp.SITES[0][0])]
    info = dict(kv.split("=") for kv in line.split("\t")[7].split(";"))
    ins = insertions[0].tobytes().decode()
    assert info["END"] == str(fp.SITES[0][0]) and info["HOMLEN"] == "0" and info["SVTYPE"] == "INS"
    assert len(info["LSEQ"]) >= 20 and len(info["RSEQ"]) >= 20 and ins.startswith(info["LSEQ"]) and ins.endswith(info["RSEQ"])
    # the record-at-a-time path and three walkers on small pieces write the same bytes
    for k, env in enumerate(({"INDELMINER_PIPELINE": "host"}, {"INDELMINER_PIECE_BYTES": "60000", "INDELMINER_WALKERS": "3"})):
        fk = str(tmp_path / ("ins%d.vcf" % k))
        r = _ok(_run(prod, BASE + ["-G", "-C", "-V", "-I", fk], d, env=env))
        assert open(fk, "rb").read() == text and r.stdout == gcv.stdout, env
    # -o detailed ignores -I and writes no FILE; without -V it is refused
    fd = str(tmp_path / "none.vcf")
    d0 = _ok(_run(prod, BASE + ["-o", "detailed"], d))
    d1 = _ok(_run(prod, BASE + ["-o", "detailed", "-G", "-C", "-V", "-I", fd], d))
    assert d1.stdout == d0.stdout and d1.stderr == d0.stderr and len(d0.stdout) > 0 and not os.path.exists(fd)
    r = _run(prod, BASE + ["-G", "-C", "-I", fd], d)
    assert r.returncode != 0 and r.stdout == b"" and b"indelminer: -I needs -V" in r.stderr and not os.path.exists(fd)


def test_product_mapping_quality_gates_the_piles(tmp_path):
    """every second clipped read gets mapping quality 20: at -q 30 fewer piles reach three reads"""
    refs, rd, _ = fp.planted_reads()
    d = fp.write_planted(str(tmp_path), refs, rd, lower_mapq_of_every_second_clipped_read=True)
    prod = _product()
    n = {}
    for q in (10, 30):
        text, recs, _ = fp.render_of_bam(d + "/aln.bam", d + "/ref.fa", q)
        f = str(tmp_path / ("ins_q%d.vcf" % q))
        _ok(_run(prod, BASE + ["-q", str(q), "-G", "-C", "-V", "-I", f], d))
        assert open(f, "rb").read() == text, q
        n[q] = len(recs)
    assert n[10] == 18 and 0 < n[30] < n[10], n
