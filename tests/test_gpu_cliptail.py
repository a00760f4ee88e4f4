"""Clipped-read breakpoints verified by the clipped bases (-V): the keyed table of im_cliptail.hip (cliptail_scatter_kernel,
cliptail_add_kernel), the comparison of cliptail_verify_kernel, and what the host driver makes of them (FORMAT CV:CH).

The yardstick is the plain restatement in tests/support/cliptails.py, written from the definition in include/indelminer_amd.h
(seam 5, "Clip tails"), not from the code under test; tests/test_cliptail_host.py pins it to cases worked by hand.
"""
import importlib.util
import os
import subprocess

import numpy as np
import pytest

from tests.support import clipcounts as cc
from tests.support import cliptails as ct
from tests.support.clipcounts import LEFT, MIN_CLIP, MIN_LEN, RIGHT
from tests.support.spanarrays import GOLD, _product

pytestmark = pytest.mark.gpu

M, I, D, N, S, H, EQ, X = 0, 1, 2, 3, 4, 5, 7, 8
CLENS = [150_000, 5_000]
NONE = 0xFFFFFFFF
CODE = {65: 1, 67: 2, 71: 4, 84: 8, 78: 15}           # A C G T N as BAM packs them


def contigs(seed=3, n_at=()):
    """the seeded random reference of tests/test_gpu_clip.py; n_at: (tid, position) that hold an N instead"""
    rng = np.random.default_rng(seed)
    out = [bytearray(bytes(rng.choice(np.frombuffer(b"ACGT", np.uint8), n))) for n in CLENS]
    for tid, p in n_at:
        out[tid][p] = ord("N")
    return [bytes(c) for c in out]


class Device:
    """one context over the reference with the clip-tail table enabled for (min_clip, min_mapq, log2_slots)"""

    def __init__(self, refs, c, q, log2_slots=16):
        from indelminer_amd import capi
        self.capi = capi
        self.refs = refs
        self.ctx = capi.Context(0)
        self.ctx.set_reference(refs)
        self.ctx.cliptail_enable(c, q, log2_slots)
        self.keep = []

    def scatter(self, raw, off):
        capi = self.capi
        d_raw = capi.DevBuf(self.ctx, len(raw) + 64).upload(raw)
        d_off = capi.DevBuf(self.ctx, 4 * len(off)).upload(off)
        self.keep += [d_raw, d_off]
        self.ctx.cliptail_scatter(capi.DevRecords(len(off) - 1, d_raw.ptr, d_off.ptr, 0))

    def add(self, table):
        """a restatement table {(tid, side, position): [bases]} through im_cliptail_add, one call per contig"""
        for tid in range(len(self.refs)):
            ent = [(p, side, b) for (t, side, p), lst in table.items() if t == tid for b in lst]
            self.ctx.cliptail_add(tid, [e[0] for e in ent], [e[1] for e in ent], [len(e[2]) for e in ent],
                                  np.array([ct.planes_of(e[2]) for e in ent], np.uint32).reshape(-1, 2))

    def sync(self):
        self.ctx._check(self.capi.lib().im_stream_sync(self.ctx.h, self.ctx.stream))

    def verify(self, tid, pr, pl, S=32):
        self.sync()
        vr, vl, sh, sr, sl = self.ctx.cliptail_verify(tid, pr, pl, S)
        return [tuple(int(x) for x in row) for row in zip(vr, vl, sh, sr, sl)]

    def check(self, table, queries, S=32):
        """queries: [(tid, pr, pl)]; every answer against the restatement"""
        for tid in range(len(self.refs)):
            qs = [(a, b) for t, a, b in queries if t == tid]
            if not qs:
                continue
            pr, pl = [a for a, _ in qs], [b for _, b in qs]
            want = ct.answer_many(table, self.refs[tid], tid, pr, pl, S)
            got = self.verify(tid, pr, pl, S)
            bad = [k for k in range(len(qs)) if got[k] != want[k]]
            assert not bad, (tid, [(qs[k], got[k], want[k]) for k in bad[:8]])
            for k in range(0, len(qs), max(1, len(qs) // 25)):      # the fast form against the plain one
                assert ct.answer(table, self.refs[tid], tid, pr[k], pl[k], S) == want[k], qs[k]

    def close(self):
        for b in self.keep:
            b.free()
        self.ctx.close()


def every_pile(table, partner=None, gap=300):
    """one query per key of the table: against the partner position it was made for, or one `gap` positions away"""
    partner = partner or {}
    out = []
    for (tid, side, p) in table:
        other = partner.get((tid, side, p), p + gap if side == RIGHT else p - gap)
        out.append((tid, p, other) if side == RIGHT else (tid, other, p))
    return sorted(set(out))


def tail_read(ref, tid, side, a, b, s, L, m, flips=(), n_at=(), flag=0, mapq=60, fill=None):
    """a read clipped at the deletion [a, b) of contig tid whose L clipped bases continue behind the other breakpoint at shift s:
    side RIGHT: m aligned bases in front of a, clipped base i = ref[b + s + i]; side LEFT: aligned from b, clipped base i (counted
    from the junction) = ref[a - 1 - s - i].  Outside the contig the base is `fill`.  flips / n_at: clipped bases (counted from the
    junction) that get another base / an N"""
    def base(p, i):
        c = ref[p] if 0 <= p < len(ref) else (fill or ord("A"))
        c = ord("A") if c == ord("N") else c                        # where the reference has an N the read holds an A
        if i in flips:
            c = b"ACGT"[(b"ACGT".index(bytes([c])) + 1 + i % 3) % 4]
        return CODE[ord("N")] if i in n_at else CODE[c]
    if side == RIGHT:
        codes = [CODE[ref[p]] for p in range(a - m, a)] + [base(b + s + i, i) for i in range(L)]
        return (tid, a - m, mapq, flag, [(M, m), (S, L)], m + L, codes)
    codes = [base(a - 1 - s - i, i) for i in range(L)][::-1] + [CODE[ref[p]] for p in range(b, b + m)]
    return (tid, b, mapq, flag, [(S, L), (M, m)], m + L, codes)


def with_bases(records, seed):
    """(tid, pos, mapq, flag, cigar) of tests/test_gpu_clip.py -> the same records with random read bases, now and then an N"""
    rng = np.random.default_rng(seed)
    out = []
    for tid, pos, mapq, flag, cigar in records:
        l_seq = sum(ln for op, ln in cigar if op in (M, I, S, EQ, X))
        codes = [1 << int(x) for x in rng.integers(0, 4, l_seq)]
        if rng.random() < 0.1 and l_seq:
            codes[int(rng.integers(0, l_seq))] = 15
        out.append((tid, pos, mapq, flag, cigar, l_seq, codes))
    return out


def scenarios(refs, c):
    """[(record, ...)], the queries they were made for, and what some of them must answer whatever the restatement says"""
    r0, r1 = refs
    R, Q, known = [], [], {}
    at = iter(range(20_000, 140_000, 1_500))

    def deletion(tid=0, width=400):
        a = next(at) if tid == 0 else 1_000
        return a, a + width

    # planted shifts 0, 1, 7, 32 and 33 (not found), three reads a side, tails at even and odd read offsets, odd and even l_seq
    for s in (0, 1, 7, 32, 33):
        a, b = deletion()
        R += [tail_read(r0, 0, RIGHT, a, b, s, 40, m) for m in (60, 61, 59)] + [tail_read(r0, 0, LEFT, a, b, s, L, 50) for L in (40, 41, 33)]
        Q.append((0, a, b)); known[(0, a, b)] = (3, 3, s) if s <= 32 else (0, 0, -1)
    # the micro-homology form: the piles stand at a + h and b, the reads match at s = h
    a, b = deletion()
    R += [tail_read(r0, 0, RIGHT, a, b, 0, 35, 60)] * 2 + [tail_read(r0, 0, LEFT, a, b, 0, 35, 60)] * 2
    Q += [(0, a, b), (0, a, b + 5), (0, a - 5, b)]; known[(0, a, b)] = (2, 2, 0)
    # clip lengths c - 1, c, 31, 32, 33, 60 on either side: n = min(L, 32), the first stores nothing
    for L in (c - 1, c, 31, 32, 33, 60):
        a, b = deletion()
        R += [tail_read(r0, 0, RIGHT, a, b, 2, L, 100 - L), tail_read(r0, 0, LEFT, a, b, 2, L, 101 - L)]
        Q.append((0, a, b)); known[(0, a, b)] = (1, 1, 2) if L >= c else (0, 0, -1)
    # 0 .. 3 mismatches at n = 20, 31, 32, the first and the last compared base among them
    for n, allowed in ((20, 1), (31, 1), (32, 2)):
        for k in range(4):
            for where in ([0] + list(range(n - k + 1, n)) if k else [], list(range(k))):
                if len(where) != k:
                    continue
                a, b = deletion()
                R += [tail_read(r0, 0, RIGHT, a, b, 0, n, 50, flips=where), tail_read(r0, 0, LEFT, a, b, 0, n + (28 if n == 32 else 0), 50, flips=where)]
                Q.append((0, a, b)); known[(0, a, b)] = (1, 1, 0) if k <= allowed else (0, 0, -1)
    # an N inside the first n bases: nothing stored; beyond base 32: stored
    a, b = deletion()
    R += [tail_read(r0, 0, RIGHT, a, b, 0, 60, 40, n_at=[31]), tail_read(r0, 0, RIGHT, a, b, 0, 60, 40, n_at=[32]), tail_read(r0, 0, RIGHT, a, b, 0, 25, 40, n_at=[0]),
          tail_read(r0, 0, LEFT, a, b, 0, 60, 40, n_at=[5]), tail_read(r0, 0, LEFT, a, b, 0, 60, 40, n_at=[45]), tail_read(r0, 0, LEFT, a, b, 0, 25, 40, n_at=[24])]
    Q.append((0, a, b)); known[(0, a, b)] = (1, 1, 0, 1, 1)
    # both ends in one record, H outside S: the record clips at a (right) and starts at b2 (left)
    a, b = deletion()
    a2, b2 = a - 40 - 500, a - 40
    left_part = tail_read(r0, 0, LEFT, a2, b2, 0, 30, 40)
    right_part = tail_read(r0, 0, RIGHT, a, b, 0, 30, 40)
    both = (0, b2, 60, 0, [(H, 4), (S, 30), (M, 40), (S, 30), (H, 9)], 100, left_part[6][:70] + right_part[6][40:])
    R += [both, both]
    Q += [(0, a, b), (0, a2, b2)]; known[(0, a, b)] = (2, 0, 0, 2, 0); known[(0, a2, b2)] = (0, 2, 0, 0, 2)
    # partner windows that run off the contig: 2 of 32 bases outside are allowed, 3 are not; at the front, at the end, on contig 1
    for tid, ref in ((0, r0), (1, r1)):
        clen = len(ref)
        for out_of in (2, 3):
            R += [tail_read(ref, tid, RIGHT, 600 + out_of, clen - 32 + out_of, 0, 32, 50), tail_read(ref, tid, LEFT, 32 - out_of, 900 + out_of, 0, 32, 50)]
            Q += [(tid, 600 + out_of, clen - 32 + out_of), (tid, 32 - out_of, 900 + out_of)]
            known[(tid, 600 + out_of, clen - 32 + out_of)] = (1, 0, 0) if out_of == 2 else (0, 0, -1)
            known[(tid, 32 - out_of, 900 + out_of)] = (0, 1, 0) if out_of == 2 else (0, 0, -1)
        R += [tail_read(ref, tid, RIGHT, 700, clen, 0, 20, 50), tail_read(ref, tid, LEFT, 0, 800, 0, 20, 50)]      # wholly outside
        Q += [(tid, 700, clen), (tid, 0, 800), (tid, 700, 2_000_000_000), (tid, -2_000_000_000, 800), (tid, -5, clen + 5)]
    # pl <= pr, and a query nobody clips at
    a, b = Q[0][1], Q[0][2]
    Q += [(0, a, a), (0, b, a), (0, a + 1, b), (0, 77, 99), (1, a, b)]
    known[(0, a, a)] = known[(0, b, a)] = (0, 0, -1)
    # -C's gates: flag, mapq, a contig that does not exist
    a, b = deletion()
    R += [tail_read(r0, 0, RIGHT, a, b, 0, 30, 50, flag=f) for f in (0x4, 0x100, 0x200, 0x400, 0x800 | 0x10)] + \
         [tail_read(r0, 0, RIGHT, a, b, 0, 30, 50, mapq=q) for q in (9, 10)] + [tail_read(r0, 7, RIGHT, a, b, 0, 30, 50), tail_read(r0, -1, LEFT, a, b, 0, 30, 50)]
    Q.append((0, a, b)); known[(0, a, b)] = (2, 0, 0, 2, 0)
    # bases that do not lie inside the record: l_seq claims more than the record carries; a clip longer than l_seq; l_seq = 0
    a, b = deletion()
    good = tail_read(r0, 0, RIGHT, a, b, 0, 30, 50)
    R += [good, good[:5] + (100_000, good[6]), good[:5] + (25, good[6][:25]), good[:5] + (0, [])]
    Q.append((0, a, b)); known[(0, a, b)] = (1, 0, 0, 1, 0)
    return R, Q, known


@pytest.mark.parametrize("qual", [True, False])
def test_cliptail_hand_made_records_with_real_bases(qual):
    """through scatter and verify; with base qualities and, as the product's walkers deliver records, without"""
    from tests.test_gpu_clip import hand_made
    c, q = 20, 10
    n_at = [(0, 30_000 + 5), (0, 30_000 + 40)]
    refs = contigs(n_at=n_at)
    R, Q, known = scenarios(refs, c)
    # a reference N inside the window: the read itself holds an A there; one such base of 20 is allowed, of 15 it is not
    R += [tail_read(refs[0], 0, RIGHT, 29_000, 30_000, 0, 20, 50), tail_read(refs[0], 0, RIGHT, 29_100, 30_000 + 30, 0, 15, 50)]
    Q += [(0, 29_000, 30_000), (0, 29_100, 30_000 + 30)]
    known[(0, 29_000, 30_000)] = (1, 0, 0); known[(0, 29_100, 30_000 + 30)] = (0, 0, -1)
    R += with_bases(hand_made(c, q), 17)                            # tests/test_gpu_clip.py's eligibility list, with random bases
    raw, off = ct.pack_records(R, qual=qual)
    parsed = ct.parse_raw(raw, off)
    assert [p[:6] for p in parsed] == [r[:6] for r in R]            # the packer and the parser agree
    table = ct.table_of(parsed, CLENS, c, q)
    # what the test is about is there: the hand-known answers, 300-entry piles, keys the N kept entries from
    for (tid, a, b), want in known.items():
        assert ct.answer(table, refs[tid], tid, a, b)[:len(want)] == want, ((tid, a, b), want)
    assert len(table[(0, RIGHT, 2040)]) >= 250 and len(table[(0, LEFT, 2000)]) >= 250
    clip_r, clip_l = cc.arrays_of([p[:5] for p in parsed], CLENS, c, q)
    n_entries = sum(len(v) for v in table.values())
    assert n_entries < sum(int(a.sum()) for a in clip_r + clip_l)   # some clipped reads store nothing
    dev = Device(refs, c, q)
    try:
        dev.scatter(raw, off)
        dev.check(table, Q + every_pile(table))
        for S in (0, 6, 7, 31):                                     # a smaller max_shift finds less
            dev.check(table, Q, S)
        dev.sync()
        assert dev.ctx.cliptail_stats() == (n_entries, 0)
    finally:
        dev.close()


def pile_table(refs, keys, per_key, seed):
    """entries for [(tid, side, position, partner)]: per_key each, most of them what the reference holds behind the partner at a
    shift of 0 .. 3, with 0 .. 3 bases changed and 1 .. 32 bases long"""
    rng = np.random.default_rng(seed)
    table, partner = {}, {}
    for tid, side, p, other in keys:
        ref = refs[tid]
        for _ in range(per_key):
            n, s = int(rng.integers(1, 33)), int(rng.integers(0, 4))
            start, step = (other + s, 1) if side == RIGHT else (other - 1 - s, -1)
            bases = [b"ACGT".index(ref[start + step * i:start + step * i + 1]) for i in range(n)]
            for i in rng.integers(0, n, int(rng.integers(0, 4))):
                bases[int(i)] = (bases[int(i)] + 1) % 4
            table.setdefault((tid, side, p), []).append(tuple(bases))
        partner[(tid, side, p)] = other
    return table, partner


def test_cliptail_table_at_its_smallest():
    refs = contigs()
    # 64 slots: 5 keys whose home slots are the last four and the first, 6 entries each: collisions, and runs that wrap past slot 63
    homes = {}
    for p in range(1_000, 140_000):
        for side in (RIGHT, LEFT):
            homes.setdefault(ct.home_slot(0, side, p, 6), []).append((side, p))
    picked = [homes[h][k] for h, k in ((63, 0), (62, 0), (63, 1), (61, 0), (0, 0))]
    keys = [(0, side, p, p + 500 if side == RIGHT else p - 500) for side, p in picked]
    table, partner = pile_table(refs, keys, 6, 41)
    dev = Device(refs, 20, 10, log2_slots=6)
    try:
        dev.add(table)
        assert dev.ctx.cliptail_stats() == (30, 0)
        dev.check(table, every_pile(table, partner))
        # 10 more make 40: 32 stored, 8 dropped; every output of verify is the no-answer value, and the call returns
        more, _ = pile_table(refs, [(1, LEFT, 2_000, 1_500)], 10, 42)
        dev.add(more)
        assert dev.ctx.cliptail_stats() == (32, 8)
        qs = every_pile(table, partner)
        got = dev.verify(0, [a for _, a, _ in qs], [b for _, _, b in qs])
        assert got == [(NONE, NONE, -1, NONE, NONE)] * len(qs)
        assert dev.verify(1, [1_500], [2_000]) == [(NONE, NONE, -1, NONE, NONE)]
        # after reset everything works again
        dev.ctx.cliptail_reset()
        dev.sync()
        assert dev.ctx.cliptail_stats() == (0, 0)
        assert dev.verify(0, [a for _, a, _ in qs], [b for _, _, b in qs]) == [(0, 0, -1, 0, 0)] * len(qs)
        dev.add(more); dev.add(table)
        both = dict(table); both.update(more)
        assert dev.ctx.cliptail_stats() == (32, 8)                  # 40 again, in another order: as many stored, others dropped
        dev.ctx.cliptail_reset()
        dev.add(table)
        assert dev.ctx.cliptail_stats() == (30, 0)
        dev.check(table, every_pile(table, partner))
    finally:
        dev.close()
    # one key with 300 entries in 1 024 slots: a probe run of several 64-slot batches, beside a second key that starts inside it
    dev = Device(refs, 20, 10, log2_slots=10)
    try:
        h = ct.home_slot(0, RIGHT, 50_000, 10)
        inside = next((side, p) for p in range(1_000, 140_000) for side in (RIGHT, LEFT) if ct.home_slot(0, side, p, 10) == (h + 100) % 1024)
        table, partner = pile_table(refs, [(0, RIGHT, 50_000, 50_700)], 300, 43)
        t2, p2 = pile_table(refs, [(0, inside[0], inside[1], inside[1] + (400 if inside[0] == RIGHT else -400))], 12, 44)
        dev.add(table); dev.add(t2)
        table.update(t2); partner.update(p2)
        assert dev.ctx.cliptail_stats() == (312, 0)
        dev.check(table, every_pile(table, partner))
        # and the refusals of the entry points
        import ctypes as C
        L = dev.capi.lib()
        assert L.im_cliptail_enable(dev.ctx.h, 20, 10, 10) == 0
        for args in ((21, 10, 10), (20, 11, 10), (20, 10, 11)):
            assert L.im_cliptail_enable(dev.ctx.h, *args) != 0
            assert L.im_last_error(dev.ctx.h) == b"im_cliptail_enable: already enabled with min_clip 20, min_mapq 10, log2_slots 10"
        one, out = np.zeros(1, np.int32), [np.zeros(1, np.uint32) for _ in range(5)]
        ptr = lambda a: a.ctypes.data_as(C.c_void_p)
        assert L.im_cliptail_verify(dev.ctx.h, 0, 1, ptr(one), ptr(one), 33, *[ptr(o) for o in out]) != 0 and b"max_shift 33" in L.im_last_error(dev.ctx.h)
        assert L.im_cliptail_verify(dev.ctx.h, 2, 1, ptr(one), ptr(one), 32, *[ptr(o) for o in out]) != 0
        assert L.im_cliptail_verify(dev.ctx.h, 0, 1, None, ptr(one), 32, *[ptr(o) for o in out]) != 0
        assert L.im_cliptail_verify(dev.ctx.h, 0, 0, None, None, 32, None, None, None, None, None) == 0
        nb = np.array([33], np.uint8)
        assert L.im_cliptail_add(dev.ctx.h, 0, 1, ptr(one), ptr(np.zeros(1, np.uint8)), ptr(nb), ptr(np.zeros(2, np.uint32))) != 0 and b"33 bases" in L.im_last_error(dev.ctx.h)
    finally:
        dev.close()
    from indelminer_amd import capi
    ctx = capi.Context(0)
    try:
        L = capi.lib()
        assert L.im_cliptail_enable(ctx.h, 20, 10, 10) != 0 and b"im_set_reference" in L.im_last_error(ctx.h)
        ctx.set_reference([b"ACGT" * 100])
        assert L.im_cliptail_reset(ctx.h, ctx.stream) != 0
        for args, word in (((0, 10, 10), b"min_clip 0"), ((20, 10, 5), b"log2_slots 5"), ((20, 10, 31), b"log2_slots 31")):
            assert L.im_cliptail_enable(ctx.h, *args) != 0 and word in L.im_last_error(ctx.h)
        recs = capi.DevRecords(0, None, None, 0)
        import ctypes as C
        assert L.im_dev_cliptail_scatter(ctx.h, C.byref(recs), ctx.stream) != 0 and L.im_last_error(ctx.h) == b"im_cliptail_enable has not been called"
    finally:
        ctx.close()


def soak_records(refs, seed, n_records=20_000):
    rng = np.random.default_rng(seed)
    R, partner = [], {}
    dels = [(0, int(a), int(a) + int(w)) for a, w in zip(range(5_000, 145_000, 2_300), rng.integers(150, 900, 61))]
    dels += [(1, 1_200, 1_900), (1, 2_500, 3_300), (1, 20, 4_970)]
    for tid, a, b in dels:
        s = int(rng.choice([0, 0, 0, 1, 3, 7, 32, 33]))
        for side in (RIGHT, LEFT):
            for _ in range(int(rng.integers(0, 16))):
                L = int(rng.integers(15, 71))
                m = int(rng.integers(10, 19 if min(a, b) < 100 else 81))
                k = int(rng.choice([0, 0, 0, 1, 2, 3]))
                n_at = [int(rng.integers(0, L))] if rng.random() < 0.05 else []
                R.append(tail_read(refs[tid], tid, side, a, b, s if rng.random() < 0.9 else int(rng.integers(0, 40)), L, m,
                                   flips=[int(x) for x in rng.integers(0, min(L, 32), k)], n_at=n_at, mapq=int(rng.choice([60, 60, 60, 9, 10]))))
        partner[(tid, RIGHT, a)] = b; partner[(tid, LEFT, b)] = a
    # clipped reads of random bases at random places, some of them at the piles, and the many reads that do not clip
    noise = []
    for _ in range(3_000):
        tid = int(rng.random() < 0.1)
        L, m = int(rng.integers(1, 80)), int(rng.integers(1, 90))
        pos = int(rng.integers(0, CLENS[tid] - 100)) if rng.random() < 0.8 else dels[int(rng.integers(0, 61))][1 + int(rng.integers(0, 2))]
        cigar = [[(M, m), (S, L)], [(S, L), (M, m)], [(S, L), (M, m), (S, L)], [(H, 3), (S, L), (M, m), (I, 2), (M, 5), (D, 3), (M, 5), (S, L)]][int(rng.integers(0, 4))]
        noise.append((tid, pos, 60, int(rng.choice([0, 0, 0, 0x10, 0x400, 0x800])), cigar))
    R += with_bases(noise, seed + 1)
    plain = [(int(rng.random() < 0.03), int(rng.integers(0, 4_800)), 60, 0, [(M, 100)]) for _ in range(n_records - len(R))]
    R += with_bases(plain, seed + 2)
    order = rng.permutation(len(R))
    return [R[int(k)] for k in order], partner


def test_cliptail_seeded_soak():
    """20 000 records with random clips on two contigs, scattered in three launches, both record forms; every pile of either side
    is queried"""
    c, q = 20, 10
    refs = contigs()
    R, partner = soak_records(refs, 7)
    assert len(R) == 20_000
    cuts = [0, 7_000, 13_001, len(R)]
    parsed = []
    dev = Device(refs, c, q, log2_slots=14)
    try:
        for k in range(3):
            raw, off = ct.pack_records(R[cuts[k]:cuts[k + 1]], qual=k != 1)
            parsed += ct.parse_raw(raw, off)
            dev.scatter(raw, off)
        table = ct.table_of(parsed, CLENS, c, q)
        n_entries = sum(len(v) for v in table.values())
        assert 1_500 < n_entries < 8_192 and max(len(v) for v in table.values()) >= 10
        qs = every_pile(table, partner)
        want = [ct.answer_many(table, refs[t], t, [a], [b])[0] for t, a, b in qs]
        assert sum(1 for w in want if w[2] > 0) >= 10 and sum(1 for w in want if w[2] == 0) >= 10 and sum(1 for w in want if w[0] and w[1]) >= 20
        dev.check(table, qs)
        dev.sync()
        assert dev.ctx.cliptail_stats() == (n_entries, 0)
    finally:
        dev.close()


def test_cliptail_add_gives_the_answers_of_the_scatter():
    """the record-at-a-time path: the restatement's entries through im_cliptail_add"""
    c, q = 20, 10
    refs = contigs()
    R, partner = soak_records(refs, 9, n_records=6_000)
    raw, off = ct.pack_records(R, qual=False)
    table = ct.table_of(ct.parse_raw(raw, off), CLENS, c, q)
    qs = every_pile(table, partner)
    answers = []
    for how in ("scatter", "add"):
        dev = Device(refs, c, q, log2_slots=14)
        try:
            if how == "scatter":
                dev.scatter(raw, off)
            else:
                dev.add(table)
            dev.check(table, qs)
            answers.append([dev.verify(t, [a for tt, a, _ in qs if tt == t], [b for tt, _, b in qs if tt == t]) for t in range(2)])
            dev.sync()
            assert dev.ctx.cliptail_stats() == (sum(len(v) for v in table.values()), 0)
        finally:
            dev.close()
    assert answers[0] == answers[1] and sum(len(x) for x in answers[0]) == len(qs) > 100


# ------------------------------------------------------------------------------------------ the product

ADDED_HEADER = ("##FORMAT=<ID=CV,", "##FORMAT=<ID=CH,", "##clipVerification=")


def _run(binary, flags, cwd, env=None):
    e = dict(os.environ)
    e.update(env or {})
    return subprocess.run([binary] + flags + ["ref.fa", "sample=aln.bam"], cwd=cwd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=e)


def _ok(r):
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    assert b"overflowed" not in r.stderr
    return r.stdout


def records_of(out):
    return [ln.split("\t") for ln in out.decode().split("\n") if ln and not ln.startswith("#")]


def strip_verification(out):
    """a -V VCF without what -V adds: its three header lines, the two keys and the two values of the records that carry them"""
    lines = []
    for ln in out.decode().split("\n"):
        if ln.startswith(ADDED_HEADER):
            continue
        if ln and not ln.startswith("#"):
            cols = ln.split("\t")
            if cols[8].endswith(":CV:CH"):
                cols[8] = cols[8][:-len(":CV:CH")]
                cols[9] = ":".join(cols[9].split(":")[:-2])
            ln = "\t".join(cols)
        lines.append(ln)
    return "\n".join(lines).encode()


def check_header(out):
    text = out.decode().split("\n")
    fmt = [i for i, ln in enumerate(text) if ln.startswith("##FORMAT=")]
    assert fmt == list(range(fmt[0], fmt[0] + len(fmt)))
    assert [text[i][:16] for i in fmt[-4:]] == ["##FORMAT=<ID=CB,", "##FORMAT=<ID=CS,", "##FORMAT=<ID=CV,", "##FORMAT=<ID=CH,"]
    assert text[fmt[-2]].startswith("##FORMAT=<ID=CV,Number=2,Type=Integer,") and text[fmt[-1]].startswith("##FORMAT=<ID=CH,Number=1,Type=Integer,")
    chrom = [i for i, ln in enumerate(text) if ln.startswith("#CHROM")][0]
    assert text[chrom - 1].startswith("##clipVerification=\"") and text[chrom - 2].startswith("##clipEvidence=\"")
    assert sum(1 for ln in text if ln.startswith(ADDED_HEADER)) == 3
    for word in ("32 clipped bases", "n >> 4", "s = 0 .. 32", "smallest s", "overflowed", "stderr"):
        assert word in text[chrom - 1], word


def check_records(out, names, fasta, table, right, left, more="", min_plain=100):
    """every record against the restatement from BAM + FASTA; returns [(CS, CV, CH)] of the records with both sides found"""
    both, plain = [], 0
    for cols in records_of(out):
        tags = cols[7].split(";")
        info = dict(kv.split("=") for kv in tags if "=" in kv)
        pos, end, bp_end = int(cols[1]), int(info["END"]), int(info["BP_END"])
        keys, vals = cols[8].split(":"), cols[9].split(":")
        if tags[0] == "DELETION" and end - pos >= MIN_LEN:
            assert cols[8] == "GT:AD:GQ" + more + ":CB:CS:CV:CH", cols
            t = names.index(cols[0])
            cv, ch = ct.verification_of(table, fasta[cols[0]], t, right[t], left[t], tags[1], pos, end, bp_end)
            assert vals[-2:] == [cv, ch], (cols, cv, ch)
            if cv != ".,.":
                both.append((vals[-3], cv, ch))
        else:
            assert "CV" not in keys and "CH" not in keys, cols
            plain += 1
    assert plain > min_plain
    return both


@pytest.fixture(scope="module")
def composite(tmp_path_factory):
    spec = importlib.util.spec_from_file_location("make_golden", os.path.join(GOLD, "make_golden.py"))
    mg = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mg)
    d = str(tmp_path_factory.mktemp("cliptail_composite"))
    mg.write_dataset(d, mg.SYNTH_E2E["synth_2ctg_composite"])
    bam = os.path.join(d, "aln.bam")
    fasta = ct.read_fasta(os.path.join(d, "ref.fa"))
    yard = {}
    for q in (10, 30):
        names, right, left = cc.arrays_of_bam(bam, MIN_CLIP, q)
        yard[q] = (names, fasta, ct.table_of_bam(bam, MIN_CLIP, q)[1], right, left)
    return d, yard


BASE = ["-i", "cfg.txt", "-s", "100"]


def test_product_clip_verification(composite):
    d, yard = composite
    prod = _product()
    gc = _ok(_run(prod, BASE + ["-G", "-C"], d))
    gcv = _ok(_run(prod, BASE + ["-G", "-C", "-V"], d))
    check_header(gcv)
    assert strip_verification(gcv) == gc                            # byte for byte what it printed without -V
    assert not any(ln.startswith(ADDED_HEADER) for ln in gc.decode().split("\n")) and b":CV" not in gc
    both = check_records(gcv, *yard[10])
    assert len(both) >= 20, len(both)
    # the planted deletions verify (tests/test_cliptail_host.py has the figures of the piles themselves): nearly every clipped read
    # continues across its deletion, and none needs a shift
    cs = sum(int(x) for s in both for x in s[0].split(","))
    cv = sum(int(x) for s in both for x in s[1].split(","))
    print("records with both sides: %d, sum CS %d, sum CV %d, CV == CS on %d" % (len(both), cs, cv, sum(1 for s in both if s[0] == s[1])))
    assert cv >= 0.95 * cs, (cv, cs)
    assert sum(1 for s in both if s[0] == s[1]) >= 0.75 * len(both)
    assert all(s[2] == "0" for s in both if s[1] != "0,0") and all(s[2] == "." for s in both if s[1] == "0,0")
    # the record-at-a-time path and three walkers on small pieces print the same bytes
    for env in ({"INDELMINER_PIPELINE": "host"}, {"INDELMINER_PIECE_BYTES": "60000", "INDELMINER_WALKERS": "3"}):
        assert _ok(_run(prod, BASE + ["-G", "-C", "-V"], d, env=env)) == gcv, env


def test_product_clip_verification_beside_depth_evidence_and_the_gate(composite):
    d, yard = composite
    prod = _product()
    gdc = _ok(_run(prod, BASE + ["-G", "-D", "-C"], d))
    gdcv = _ok(_run(prod, BASE + ["-G", "-D", "-C", "-V"], d))
    check_header(gdcv)
    assert strip_verification(gdcv) == gdc
    assert len(check_records(gdcv, *yard[10], more=":DM:DFC")) >= 20
    gcv = _ok(_run(prod, BASE + ["-G", "-C", "-V"], d))
    assert [r[9].split(":")[-2:] for r in records_of(gdcv)] == [r[9].split(":")[-2:] for r in records_of(gcv)]
    # -o detailed ignores -V as it ignores -G and -C; without -C it is refused
    d0 = _ok(_run(prod, BASE + ["-o", "detailed"], d))
    assert _ok(_run(prod, BASE + ["-o", "detailed", "-G", "-C", "-V"], d)) == d0 and len(d0) > 0
    r = _run(prod, BASE + ["-G", "-V"], d)
    assert r.returncode != 0 and r.stdout == b"" and b"indelminer: -V needs -C" in r.stderr
    # -q moves the gate of the clip tails too
    q30 = _ok(_run(prod, BASE + ["-q", "30", "-G", "-C", "-V"], d))
    assert strip_verification(q30) == _ok(_run(prod, BASE + ["-q", "30", "-G", "-C"], d))
    assert len(check_records(q30, *yard[30])) >= 20


@pytest.fixture(scope="module")
def gated(tmp_path_factory):
    """a smaller data set of the same kind in which every second clipped read has mapping quality 20: between -q 10 and -q 30"""
    from indelminer_amd import bamwrite, synth
    refs, rd = synth.simulate(seed=21, ref_len=100_000, coverage=30, n_contigs=1, big_every=3)
    last = np.maximum(rd.ncig.astype(np.int64) - 1, 0)
    clipped = np.nonzero((rd.ncig > 1) & ((rd.cig_op[:, 0] == S) | (rd.cig_op[np.arange(rd.n), last] == S)))[0]
    rd.overrides = {int(i): {"mapq": 20} for i in clipped[::2]}
    d = str(tmp_path_factory.mktemp("cliptail_gated"))
    contigs_ = [("ctg0", len(refs[0]))]
    bamwrite.write_fasta(d + "/ref.fa", contigs_, refs)
    bamwrite.write_bam(d + "/aln.bam", contigs_, rd)
    open(d + "/cfg.txt", "w").write("IL generic 300 700\n")
    return d, len(clipped)


def test_product_mapping_quality_gates_the_clip_tails(gated):
    """-q moves the gate: the reads of mapping quality 20 are in the table at -q 10 and not at -q 30, and CV shows it"""
    d, n_clipped = gated
    prod = _product()
    bam = os.path.join(d, "aln.bam")
    fasta = ct.read_fasta(os.path.join(d, "ref.fa"))
    outs, sizes = {}, {}
    for q in (10, 30):
        names, right, left = cc.arrays_of_bam(bam, MIN_CLIP, q)
        table = ct.table_of_bam(bam, MIN_CLIP, q)[1]
        sizes[q] = sum(len(v) for v in table.values())
        out = _ok(_run(prod, BASE + ["-q", str(q), "-G", "-C", "-V"], d))
        both = check_records(out, names, fasta, table, right, left, min_plain=10)
        assert len(both) >= 3, (q, both)
        outs[q] = both
    assert n_clipped >= 100 and 0 < sizes[30] < sizes[10]
    cv = {q: sum(int(x) for s in outs[q] for x in s[1].split(",")) for q in outs}
    assert 0 < cv[30] < cv[10], cv
