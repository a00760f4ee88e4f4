"""Clipped-read breakpoint evidence for large deletions (-C): the point counts of im_span.hip's clip_scatter_kernel, the arg-max
of clip_argmax_kernel, and what the host driver makes of them (FORMAT CB:CS).

The yardstick is the plain restatement in tests/support/clipcounts.py, written from the definition in include/indelminer_amd.h
(seam 5, "Clipped reads"), not from the code under test; tests/test_clip_host.py pins it to cases worked by hand, and
clip_brute below restates the definition once more, position by position, where that is affordable.
"""
import importlib.util
import os
import struct
import subprocess

import numpy as np
import pytest

from tests.support import clipcounts as cc
from tests.support.clipcounts import LEFT, MIN_CLIP, MIN_LEN, RIGHT
from tests.support.spanarrays import GOLD, _product

pytestmark = pytest.mark.gpu

M, I, D, N, S, H, EQ, X = 0, 1, 2, 3, 4, 5, 7, 8
CLENS = [150_000, 5_000]


# ------------------------------------------------------------------------------------------ records

def rec(tid, pos, cigar, flag=0, mapq=60):
    return (tid, pos, mapq, flag, cigar)


def raw_records(records, qual=True):
    """[(tid, pos, mapq, flag, cigar)] -> the device layout (raw uint8, rec_off uint32[n + 1]): core, qname, CIGAR, packed bases,
    qualities (qual=False: without them and with bin = 0xFFFF, as the product's walkers deliver records), one aux tag"""
    blob, off = bytearray(), [0]
    for i, (tid, pos, mapq, flag, cigar) in enumerate(records):
        qname = b"c%d\0" % i
        l_seq = sum(ln for op, ln in cigar if op in (M, I, S, EQ, X))
        core = struct.pack("<iiBBHHHiiii", tid, pos, len(qname), mapq, 4680 if qual else 0xFFFF, len(cigar), flag, l_seq, -1, -1, 0)
        body = (core + qname + b"".join(struct.pack("<I", (ln << 4) | op) for op, ln in cigar) + b"\x11" * ((l_seq + 1) // 2) +
                (b"\x28" * l_seq if qual else b"") + b"NMC\x01")
        blob += body + b"\0" * (-len(body) % 4)
        off.append(len(blob))
    return np.frombuffer(bytes(blob), np.uint8).copy(), np.array(off, np.uint32)


def parse_raw(raw, off):
    b = raw.tobytes()
    return [cc.parse_record(b, int(off[i]), int(off[i + 1])) for i in range(len(off) - 1)]


def hand_made(c, q=10):
    """c: min_clip.  The first record with a clip opens the workgroup's LDS window at position 1000: it holds 1000 .. 5095."""
    c0, c1 = CLENS
    both = [(S, 30), (M, 40), (S, 30)]
    R = [
        rec(0, 1000, [(S, c), (M, 80)]),                            # a left clip of exactly min_clip, on the window's first position
        rec(0, 1010, [(S, c - 1), (M, 80)]),                        # one base short
        rec(0, 1020, [(M, 80), (S, c)]), rec(0, 1030, [(M, 80), (S, c - 1)]),      # the same at the right end
        rec(0, 1040, both),                                         # both ends in one record
        rec(0, 1050, [(H, 5), (S, 30), (M, 40), (S, 30), (H, 7)]),  # H in front of the leading S and behind the trailing one
        rec(0, 1055, [(H, 1), (H, 2), (S, 30), (M, 40), (S, 30), (H, 2), (H, 1)]),      # and more than one of them
        rec(0, 1060, [(H, 30), (M, 70)]), rec(0, 1061, [(M, 70), (H, 30)]),        # H alone is no clip
        rec(0, 1070, [(M, 10), (I, 1), (M, 10), (D, 1), (M, 10), (I, 2), (M, 10), (D, 3), (M, 17), (S, 40)]),     # more operations than registers
        rec(0, 1080, [(M, 30), (D, 7), (M, 20), (N, 500), (M, 10), (S, 40)]),     # D and N move refend
        rec(0, 1085, [(EQ, 30), (X, 1), (EQ, 39), (S, 30)]),        # = and X consume reference
        rec(0, 1090, [(S, 100)]), rec(0, 1091, [(H, 10), (S, 90)]),     # 100S alone consumes no reference
        rec(0, 1092, [(S, 30), (I, 40), (S, 30)]),                  # nor does this one
        rec(0, 1095, [(M, 20), (S, 25), (M, 55)]),                  # an S inside the CIGAR is not looked at
        rec(0, 1096, [(S, 30), (M, 20), (S, 25), (M, 25)]),         # ... the leading one still counts
    ]
    R += [rec(0, 1100 + k, both, flag=bit) for k, bit in enumerate((0x4, 0x100, 0x200, 0x400))]
    R += [
        rec(0, 1110, [(H, 40), (M, 30), (S, 30)], flag=0x800),      # a supplementary alignment counts
        rec(0, 1120, both, mapq=q - 1), rec(0, 1121, both, mapq=q),
        rec(-1, 1130, both), rec(7, 1131, both),                    # no contig, a contig that does not exist
        rec(0, c0 - 80, [(M, 80), (S, 30)]),                        # refend == clen counts ...
        rec(0, c0 - 79, [(M, 80), (S, 30)]),                        # ... clen + 1 does not
        rec(0, 0, [(S, 30), (M, 70)]),                              # pos = 0 with a left clip (in front of the window)
        rec(0, -5, [(M, 70), (S, 30)]), rec(0, -1, [(S, 30), (M, 70)]),     # a negative pos: only refend can lie on the contig
        rec(0, 101_000, both),                                      # 100 kb from the workgroup's first record: outside the window
        rec(0, 5095 - 70, [(M, 70), (S, 30)]), rec(0, 5096 - 70, [(M, 70), (S, 30)]),      # refend on the window's last position, and behind it
        rec(0, 5095, [(S, 30), (M, 70)]), rec(0, 5096, [(S, 30), (M, 70)]),                # pos on the window's last position, and behind it
        rec(1, 200, [(S, 30), (M, 70)]),                            # a second contig inside the same workgroup
        rec(1, c1 - 70, [(M, 70), (S, 30)]), rec(1, c1 - 69, [(M, 70), (S, 30)]), rec(1, c1, [(S, 30), (M, 1)]), rec(1, c1 + 1, [(S, 30), (M, 1)]),
    ]
    assert len(R) <= 100
    R += [rec(0, 2000, both)] * 300                                 # one position, more than one workgroup: the packed halves meet the memory atomics
    R += [rec(0, 1200, [(M, 50), (S, 50)]), rec(1, 100, both)]      # and back again (unsorted input is legal for the scatter)
    return R


def clip_brute(records, tid_want, clen, n_contigs, c, q):
    """the definition itself, position by position (a small contig): checks the restatement"""
    facts = []
    for tid, pos, mapq, flag, cigar in records:
        if tid != tid_want or not 0 <= tid < n_contigs or flag & 0x4 or flag & 0x100 or flag & 0x200 or flag & 0x400 or mapq < q:
            continue
        refend, consumes = pos, False
        for op, ln in cigar:
            if op in (M, EQ, X, D, N):
                refend += ln; consumes = True
        k0 = 0
        while k0 < len(cigar) and cigar[k0][0] == H:
            k0 += 1
        k1 = len(cigar) - 1
        while k1 >= 0 and cigar[k1][0] == H:
            k1 -= 1
        if not consumes:
            continue
        facts.append((cigar[k1][0] == S and cigar[k1][1] >= c, refend, cigar[k0][0] == S and cigar[k0][1] >= c, pos))
    right, left = np.zeros(clen + 1, np.int64), np.zeros(clen + 1, np.int64)
    for p in range(clen + 1):
        for r_clip, refend, l_clip, pos in facts:
            right[p] += r_clip and refend == p
            left[p] += l_clip and pos == p
    return right, left


# ------------------------------------------------------------------------------------------ device level

class Device:
    """one context with the clip arrays enabled for (min_clip, min_mapq) over contigs of the given lengths"""

    def __init__(self, clens, c, q, seed=3):
        from indelminer_amd import capi
        self.capi = capi
        rng = np.random.default_rng(seed)
        self.clens = list(clens)
        self.ctx = capi.Context(0)
        self.ctx.set_reference([bytes(rng.choice(np.frombuffer(b"ACGT", np.uint8), n)) for n in clens])
        self.ctx.clip_enable(c, q)
        self.keep = []

    def scatter(self, raw, off):
        capi = self.capi
        d_raw = capi.DevBuf(self.ctx, len(raw) + 64).upload(raw)
        d_off = capi.DevBuf(self.ctx, 4 * len(off)).upload(off)
        self.keep += [d_raw, d_off]
        recs = capi.DevRecords(len(off) - 1, d_raw.ptr, d_off.ptr, 0)
        self.ctx.clip_scatter(recs)
        return recs

    def sync(self):
        self.ctx._check(self.capi.lib().im_stream_sync(self.ctx.h, self.ctx.stream))

    def every_position(self, tid):
        """(clipR, clipL) of contig tid through windows of one position, both sides in one call"""
        self.sync()
        n = self.clens[tid] + 1
        p = np.tile(np.arange(n, dtype=np.int32), 2)
        cnt, pos = self.ctx.clip_query_tid(tid, np.repeat(np.array([RIGHT, LEFT], np.uint8), n), p, p)
        assert np.array_equal(pos, p)
        return cnt[:n].astype(np.int64), cnt[n:].astype(np.int64)

    def check(self, want_right, want_left):
        for tid in range(len(self.clens)):
            for name, got, want in zip(("clipR", "clipL"), self.every_position(tid), (want_right[tid], want_left[tid])):
                bad = np.nonzero(got != want)[0]
                assert len(bad) == 0, (name, tid, bad[:10], got[bad[:10]], want[bad[:10]])

    def close(self):
        for b in self.keep:
            b.free()
        self.ctx.close()


@pytest.mark.parametrize("c", [20, 1])
def test_clip_hand_made_records_every_position(c):
    recs = hand_made(c)
    right, left = cc.arrays_of(recs, CLENS, c, 10)
    # the restatement against the definition, where that is affordable, and on the cases that name a position
    br, bl = clip_brute(recs, 1, CLENS[1], len(CLENS), c, 10)
    assert np.array_equal(right[1], br) and np.array_equal(left[1], bl) and br.sum() >= 2 and bl.sum() >= 3
    assert left[0][1000] == 1 and left[0][1010] == 0 and right[0][1100] == 1 and right[0][1110] == 0
    assert right[0][1647] == 1 and right[0][1131] == 1 and right[0][1155] == 1 and left[0][1050] == left[0][1055] == right[0][1090] == right[0][1095] == 1
    assert right[0][CLENS[0]] == 1 and right[1][CLENS[1]] == 1 and left[1][CLENS[1]] == 1 and left[0][0] == 1 and right[0][65] == 1
    assert right[0][5095] == right[0][5096] == left[0][5095] == left[0][5096] == 1
    assert left[0][2000] == 300 and right[0][2040] == 300 and left[0][1096] == 1 and right[0][1250] == 1
    assert left[0][1100:1104].sum() == 0 and left[0][1120] == 0 and left[0][1121] == 1
    dev = Device(CLENS, c, 10)
    try:
        raw, off = raw_records(recs)
        assert parse_raw(raw, off) == recs                          # the packer and the parser agree
        dev.scatter(raw, off)
        dev.check(right, left)
    finally:
        dev.close()


def test_clip_synthetic_chunk_every_position():
    """a chunk at the density of the 30x benchmark input (two contigs, so that workgroups straddle the contig boundary), scattered
    in two calls, with the hand-made records on top"""
    from indelminer_amd import rawrec, synth
    refs, rd = synth.simulate(seed=11, ref_len=150_000, coverage=30, n_contigs=2, big_every=9)
    clens = [len(r) for r in refs]
    raw, off = rawrec.records(rd)
    half = rd.n // 2
    c, q = 20, 10
    dev = Device(clens, c, q)
    try:
        for lo, hi in ((0, half), (half, rd.n)):
            dev.scatter(*rawrec.records(rd, lo, hi))
        extra = [x for x in hand_made(c) if x[0] != 1 or x[1] < 1000]
        dev.scatter(*raw_records(extra))
        recs = parse_raw(raw, off) + extra
        assert len(recs) == rd.n + len(extra)
        right, left = cc.arrays_of(recs, clens, c, q)
        # the reads the simulator clips at its large deletions pile up: an all-zero answer cannot pass
        synth_right, synth_left = cc.arrays_of(recs[:rd.n], clens, c, q)
        assert sum(int((a >= 4).sum()) for a in synth_right) >= 10 and sum(int((a >= 4).sum()) for a in synth_left) >= 10
        dev.check(right, left)
    finally:
        dev.close()


def test_clip_records_without_qualities_and_reset():
    """the layout the product's walkers deliver (no base qualities); im_clip_reset + a second pass gives the same arrays, and a
    reset of contig 0 leaves contig 1 alone"""
    from indelminer_amd import rawrec, synth
    refs, rd = synth.simulate(seed=12, ref_len=60_000, coverage=20, n_contigs=2, big_every=5)
    clens = [len(r) for r in refs]
    raw, off = rawrec.records(rd, qual=False)
    full_raw, full_off = rawrec.records(rd)
    assert len(raw) < len(full_raw)
    extra = hand_made(20)[:40]
    right, left = cc.arrays_of(parse_raw(full_raw, full_off) + extra, clens, 20, 10)
    assert all(a.max() >= 3 for a in right + left)
    dev = Device(clens, 20, 10)
    try:
        hr, ho = raw_records(extra, qual=False)
        assert parse_raw(hr, ho) == extra
        dev.scatter(raw, off); dev.scatter(hr, ho)
        dev.check(right, left)
        dev.ctx.clip_reset(0)
        r0, l0 = dev.every_position(0)
        assert not r0.any() and not l0.any()
        zeros = np.zeros(clens[0] + 1, np.int64)
        dev.check([zeros, right[1]], [zeros, left[1]])
        dev.ctx.clip_reset(1)
        dev.scatter(raw, off); dev.scatter(hr, ho)
        dev.check(right, left)
    finally:
        dev.close()


def test_clip_argmax_query():
    """the arg-max on arrays built through im_clip_build: ties, the maximum on a window's first and last position, windows of
    1, 63, 64, 65 and 5000 positions, across position 8192, clipped at 0 and at clen, empty after the clip, both sides mixed"""
    from indelminer_amd import capi
    rng = np.random.default_rng(31)
    clen = 20_000
    pos = np.concatenate([rng.integers(0, clen + 1, 6000), rng.integers(8100, 8300, 600), [0, 0, 0, clen, clen, clen, -1, clen + 1, -7]])
    side = rng.integers(0, 2, len(pos)).astype(np.uint8)
    ok = (pos >= 0) & (pos <= clen)
    right, left = np.zeros(clen + 1, np.int64), np.zeros(clen + 1, np.int64)
    np.add.at(right, pos[ok & (side == 0)], 1); np.add.at(left, pos[ok & (side == 1)], 1)
    assert right.max() >= 4 and left.max() >= 4
    fixed = []                                                      # (side, beg, end)
    top = int(np.argmax(right))
    fixed += [(RIGHT, top, top + 40), (RIGHT, top - 40, top), (RIGHT, top, top)]                   # the maximum on the first and on the last position
    for width in (1, 63, 64, 65, 5000):
        fixed += [(s, a, a + width - 1) for s in (RIGHT, LEFT) for a in (0, 777, 8192 - width // 2, clen - width + 1)]
    fixed += [(LEFT, 8100, 8300), (RIGHT, 8191, 8192), (LEFT, 8192, 8192)]                         # across position 8192
    fixed += [(RIGHT, -500, 30), (LEFT, -1, 0), (RIGHT, clen - 30, clen + 900), (LEFT, clen, clen + 1), (RIGHT, -10**9, 10**9)]
    fixed += [(RIGHT, -50, -1), (LEFT, clen + 1, clen + 50), (RIGHT, 300, 299), (LEFT, 5000, 100)]      # empty after the clip
    rb = rng.integers(-100, clen + 100, 2000); rw = rng.choice([0, 1, 5, 20, 64, 200, 3000], 2000)
    qs = np.concatenate([[f[0] for f in fixed], rng.integers(0, 2, 2000)]).astype(np.uint8)
    qb = np.concatenate([[f[1] for f in fixed], rb]).astype(np.int32)
    qe = np.concatenate([[f[2] for f in fixed], rb + rw]).astype(np.int32)
    want_c, want_p = cc.argmax_many(right, left, qs, qb, qe)
    for k in list(range(len(fixed))) + list(range(len(fixed), len(qs), 50)):                       # the fast form against the plain one
        assert cc.argmax(left if qs[k] else right, qb[k], qe[k]) == (want_c[k], want_p[k]), k
    # ties exist among the windows asked, and the smallest position wins them
    tied = [k for k in range(len(qs)) if want_c[k] > 0 and ((left if qs[k] else right)[max(qb[k], 0):qe[k] + 1] == want_c[k]).sum() > 1]
    assert len(tied) >= 50 and list(want_c[-4 + len(fixed):len(fixed)]) == [0] * 4 and list(want_p[-4 + len(fixed):len(fixed)]) == [-1] * 4
    ctx = capi.Context(0)
    try:
        ctx.clip_build(clen, pos, side)
        for _ in range(2):                                          # the same call twice
            cnt, at = ctx.clip_query(qs, qb, qe)
            bad = np.nonzero((cnt != want_c) | (at != want_p))[0]
            assert len(bad) == 0, (bad[:10], qs[bad[:10]], qb[bad[:10]], qe[bad[:10]], cnt[bad[:10]], at[bad[:10]], want_c[bad[:10]], want_p[bad[:10]])
        p = np.arange(clen + 1, dtype=np.int32)
        assert np.array_equal(ctx.clip_query(np.zeros(clen + 1, np.uint8), p, p)[0], right)
        assert np.array_equal(ctx.clip_query(np.ones(clen + 1, np.uint8), p, p)[0], left)
        ctx.clip_build(100, np.zeros(0, np.int32), np.zeros(0, np.uint8))       # an empty build answers zeros
        cnt, at = ctx.clip_query([0, 1, 0], [0, 0, 101], [100, 100, 300])
        assert list(cnt) == [0, 0, 0] and list(at) == [0, 0, -1]
    finally:
        ctx.close()


def test_clip_build_beside_the_other_builds_and_the_refusals():
    """-G -P -C on the record-at-a-time path holds span, pair-span and clip arrays of one contig: each query answers its own.
    The enable refuses other parameters under its own name; a null pointer with n = 1 is an argument error, not a fault."""
    import ctypes as C
    from indelminer_amd import capi
    rng = np.random.default_rng(33)
    clen = 30_000
    rs = rng.integers(0, clen, 6000).astype(np.int32); rl = rng.choice([40, 100], 6000).astype(np.int32)
    fs = rng.integers(0, clen, 3000).astype(np.int32); fl = rng.choice([300, 500, 650], 3000).astype(np.int32)
    cp = rng.integers(0, clen + 1, 4000).astype(np.int32); cs = rng.integers(0, 2, 4000).astype(np.uint8)
    right, left = np.zeros(clen + 1, np.int64), np.zeros(clen + 1, np.int64)
    np.add.at(right, cp[cs == 0], 1); np.add.at(left, cp[cs == 1], 1)
    p = np.arange(clen + 1, dtype=np.int32)
    ctx = capi.Context(0)
    L = capi.lib()
    try:
        one, out, sd, at = np.zeros(1, np.int32), np.zeros(1, np.uint32), np.zeros(1, np.uint8), np.zeros(1, np.int32)
        ptr = lambda a: a.ctypes.data_as(C.c_void_p)
        assert L.im_clip_query(ctx.h, 1, ptr(sd), ptr(one), ptr(one), ptr(out), ptr(at)) != 0
        assert L.im_last_error(ctx.h) == b"im_clip_build has not been called"
        ctx.span_build(clen, rs, rl, 10)
        span = ctx.span_query(p, p).copy()
        ctx.clip_build(clen, cp, cs)
        ctx.pairspan_build(clen, fs, fl, 10)
        pspan = ctx.pairspan_query(p, p).copy()
        assert span.max() > 5 and pspan.max() > 5 and not np.array_equal(span, pspan)
        assert np.array_equal(ctx.clip_query(np.zeros(clen + 1, np.uint8), p, p)[0], right)
        assert np.array_equal(ctx.clip_query(np.ones(clen + 1, np.uint8), p, p)[0], left)
        ctx.clip_build(clen // 2, cp, cs)                           # another length: the other two arrays stay
        assert np.array_equal(ctx.span_query(p, p), span) and np.array_equal(ctx.pairspan_query(p, p), pspan)
        half = p[:clen // 2 + 1]
        assert np.array_equal(ctx.clip_query(np.zeros(len(half), np.uint8), half, half)[0], right[:clen // 2 + 1])
        # null pointers with n = 1, and a side that is neither 0 nor 1
        for args in ((None, ptr(one), ptr(one), ptr(out), ptr(at)), (ptr(sd), None, ptr(one), ptr(out), ptr(at)), (ptr(sd), ptr(one), None, ptr(out), ptr(at)),
                     (ptr(sd), ptr(one), ptr(one), None, ptr(at)), (ptr(sd), ptr(one), ptr(one), ptr(out), None)):
            assert L.im_clip_query(ctx.h, 1, *args) != 0
        assert L.im_clip_build(ctx.h, 100, 1, None, ptr(sd)) != 0 and L.im_clip_build(ctx.h, 100, 1, ptr(one), None) != 0
        sd[0] = 2
        assert L.im_clip_query(ctx.h, 1, ptr(sd), ptr(one), ptr(one), ptr(out), ptr(at)) != 0 and b"side 2" in L.im_last_error(ctx.h)
        assert L.im_clip_build(ctx.h, 100, 1, ptr(one), ptr(sd)) != 0 and b"side 2" in L.im_last_error(ctx.h)
        sd[0] = 0
        assert L.im_clip_query(ctx.h, 0, None, None, None, None, None) == 0
        # the genome-wide form: before the reference, before the enable, and the enable's own refusals
        recs = capi.DevRecords(0, None, None, 0)
        assert L.im_clip_enable(ctx.h, 20, 10) != 0 and b"im_set_reference" in L.im_last_error(ctx.h)
        ctx.set_reference([b"ACGT" * 100, b"AC" * 30])
        assert L.im_dev_clip_scatter(ctx.h, C.byref(recs), ctx.stream) != 0 and L.im_last_error(ctx.h) == b"im_clip_enable has not been called"
        assert L.im_clip_query_tid(ctx.h, 0, 1, ptr(sd), ptr(one), ptr(one), ptr(out), ptr(at)) != 0 and L.im_clip_reset(ctx.h, 0, ctx.stream) != 0
        assert L.im_clip_enable(ctx.h, 0, 10) != 0
        assert L.im_last_error(ctx.h) == b"im_clip_enable: min_clip 0, must be >= 1"
        ctx.span_enable(10, 10)
        ctx.clip_enable(20, 10)
        assert L.im_clip_enable(ctx.h, 21, 10) != 0
        assert L.im_last_error(ctx.h) == b"im_clip_enable: already enabled with min_clip 20, min_mapq 10"
        assert L.im_clip_enable(ctx.h, 20, 11) != 0
        assert L.im_last_error(ctx.h) == b"im_clip_enable: already enabled with min_clip 20, min_mapq 10"
        assert L.im_span_enable(ctx.h, 11, 10) != 0
        assert L.im_last_error(ctx.h) == b"im_span_enable: already enabled with flank 10, min_mapq 10"
        assert L.im_clip_enable(ctx.h, 20, 10) == 0
        assert L.im_clip_query_tid(ctx.h, 0, 1, None, ptr(one), ptr(one), ptr(out), ptr(at)) != 0
        assert L.im_clip_query_tid(ctx.h, 2, 1, ptr(sd), ptr(one), ptr(one), ptr(out), ptr(at)) != 0 and L.im_clip_reset(ctx.h, 2, ctx.stream) != 0
        cnt, at2 = ctx.clip_query_tid(1, [0, 1, 1], [0, -5, 61], [60, 900, 70])
        assert list(cnt) == [0, 0, 0] and list(at2) == [0, 0, -1]
    finally:
        ctx.close()


# ------------------------------------------------------------------------------------------ the product

ADDED_HEADER = ("##FORMAT=<ID=CB,", "##FORMAT=<ID=CS,", "##clipEvidence=")


def _run(binary, flags, cwd, env=None):
    e = dict(os.environ)
    e.update(env or {})
    return subprocess.run([binary] + flags + ["ref.fa", "sample=aln.bam"], cwd=cwd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=e)


def _ok(r):
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    return r.stdout


def records_of(out):
    return [ln.split("\t") for ln in out.decode().split("\n") if ln and not ln.startswith("#")]


def strip_clip(out):
    """a -C VCF without what -C adds: its three header lines, the two keys and the two values of the records that carry them"""
    lines = []
    for ln in out.decode().split("\n"):
        if ln.startswith(ADDED_HEADER):
            continue
        if ln and not ln.startswith("#"):
            cols = ln.split("\t")
            if cols[8].endswith(":CB:CS"):
                cols[8] = cols[8][:-len(":CB:CS")]
                cols[9] = ":".join(cols[9].split(":")[:-2])
            ln = "\t".join(cols)
        lines.append(ln)
    return "\n".join(lines).encode()


def check_header(out):
    text = out.decode().split("\n")
    fmt = [i for i, ln in enumerate(text) if ln.startswith("##FORMAT=")]
    assert fmt == list(range(fmt[0], fmt[0] + len(fmt)))
    assert text[fmt[-2]].startswith("##FORMAT=<ID=CB,Number=2,") and text[fmt[-1]].startswith("##FORMAT=<ID=CS,Number=2,")     # behind the last FORMAT line
    chrom = [i for i, ln in enumerate(text) if ln.startswith("#CHROM")][0]
    assert text[chrom - 1].startswith("##clipEvidence=\"") and sum(1 for ln in text if ln.startswith(ADDED_HEADER)) == 3
    for word in ("soft clip", "at least %d bases" % MIN_CLIP, "%d positions" % cc.SLACK, "END-POS >= %d" % MIN_LEN, "smaller"):
        assert word in text[chrom - 1], word


def check_records(out, names, right, left, more=""):
    """every record against the restatement; returns [(kind, POS, END, BP_END, CB, CS)] of the records that carry the fields"""
    seen, plain = [], 0
    for cols in records_of(out):
        tags = cols[7].split(";")
        info = dict(kv.split("=") for kv in tags if "=" in kv)
        pos, end, bp_end = int(cols[1]), int(info["END"]), int(info["BP_END"])
        if tags[0] == "DELETION" and end - pos >= MIN_LEN:
            assert cols[8] == "GT:AD:GQ" + more + ":CB:CS", cols
            t = names.index(cols[0])
            cb, cs, _ = cc.evidence_of(right[t], left[t], tags[1], pos, end, bp_end)
            assert cols[9].split(":")[-2:] == [cb, cs], (cols, cb, cs)
            seen.append((tags[1], pos, end, bp_end, cb, cs))
        else:
            assert "CB" not in cols[8].split(":") and "CS" not in cols[8].split(":"), cols
            plain += 1
    assert plain > 100
    return seen


@pytest.fixture(scope="module")
def composite(tmp_path_factory):
    spec = importlib.util.spec_from_file_location("make_golden", os.path.join(GOLD, "make_golden.py"))
    mg = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mg)
    d = str(tmp_path_factory.mktemp("clip_composite"))
    mg.write_dataset(d, mg.SYNTH_E2E["synth_2ctg_composite"])
    return d, os.path.join(d, "aln.bam")


BASE = ["-i", "cfg.txt", "-s", "100"]


def test_product_clip_evidence(composite):
    d, bam = composite
    prod = _product()
    names, right, left = cc.arrays_of_bam(bam, MIN_CLIP, 10)
    g = _ok(_run(prod, BASE + ["-G"], d))
    gc = _ok(_run(prod, BASE + ["-G", "-C"], d))
    check_header(gc)
    assert strip_clip(gc) == g                                      # byte for byte what it printed without -C
    assert not any(ln.startswith(ADDED_HEADER) for ln in g.decode().split("\n")) and b":CB" not in g
    seen = check_records(gc, names, right, left)
    both = [s for s in seen if "." not in s[4]]
    assert len(both) >= 20, (len(both), len(seen))
    assert all("." not in s[4] for s in seen if s[0] == "PAIRED_READ") and sum(1 for s in seen if s[0] == "PAIRED_READ") >= 5
    for kind, pos, end, bp_end, cb, cs in both:
        a, b = (int(x) for x in cb.split(","))
        assert pos <= a <= pos + max(0, bp_end - end) and end <= b <= max(end, bp_end), (kind, pos, end, bp_end, cb)
        assert all(int(x) > 0 for x in cs.split(","))
    assert {"SPLIT_READ", "COMPOSITE", "PAIRED_READ"} <= {s[0] for s in seen}
    # the record-at-a-time path and three walkers on small pieces print the same bytes
    for env in ({"INDELMINER_PIPELINE": "host"}, {"INDELMINER_PIECE_BYTES": "60000", "INDELMINER_WALKERS": "3"}):
        assert _ok(_run(prod, BASE + ["-G", "-C"], d, env=env)) == gc, env


def test_product_clip_evidence_beside_depth_evidence_and_the_gate(composite):
    d, bam = composite
    prod = _product()
    names, right, left = cc.arrays_of_bam(bam, MIN_CLIP, 10)
    gd = _ok(_run(prod, BASE + ["-G", "-D"], d))
    gdc = _ok(_run(prod, BASE + ["-G", "-D", "-C"], d))
    check_header(gdc)
    assert strip_clip(gdc) == gd
    assert len(check_records(gdc, names, right, left, more=":DM:DFC")) >= 20
    # -o detailed ignores -C as it ignores -G; -c is refused
    d0 = _ok(_run(prod, BASE + ["-o", "detailed"], d))
    assert _ok(_run(prod, BASE + ["-o", "detailed", "-G", "-C"], d)) == d0 and len(d0) > 0
    r = _run(prod, BASE + ["-G", "-C", "-c", "ctg0:1-30000"], d)
    assert r.returncode != 0 and r.stdout == b"" and b"indelminer: -C is not available with -c" in r.stderr
    # -q moves the gate of the clipped reads too
    names30, right30, left30 = cc.arrays_of_bam(bam, MIN_CLIP, 30)
    q30 = _ok(_run(prod, BASE + ["-q", "30", "-G", "-C"], d))
    assert strip_clip(q30) == _ok(_run(prod, BASE + ["-q", "30", "-G"], d))
    assert len(check_records(q30, names30, right30, left30)) >= 20
