"""Pair links (-M): the scatter, add and count kernels of im_links.hip behind the six im_pairlink_* entries, and what the host driver
makes of them (PE= in -U's and -N's FILE).

The yardstick is the plain restatement in tests/support/pairlinks.py, written from the definition in include/indelminer_amd.h (seam 5,
"Pair links"), not from the code under test; tests/test_pairlink_host.py pins it to cases worked by hand.  Every answer is compared
exactly.
"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests.support import pairlinks as pk
from tests.support.pairlinks import EVERTED, FORWARD, NONE, REVERSE, Rec
from tests.support.spanarrays import _product

pytestmark = pytest.mark.gpu

CLENS = [150_000, 5_000, 70]
HASH_MUL = 0x9E3779B97F4A7C15


def contigs(seed=3):
    rng = np.random.default_rng(seed)
    return [bytes(rng.choice(np.frombuffer(b"ACGT", np.uint8), n)) for n in CLENS]


def home_slot(tid, bucket, kind, log2_slots):
    """the first slot a link of this key probes (the header states the hash)"""
    key = (1 << 63) | (tid << 26) | (bucket << 2) | kind
    return ((key * HASH_MUL) & (2**64 - 1)) >> (64 - log2_slots)


class Device:
    """one context over three contigs with the pair-link table enabled"""

    def __init__(self, q=10, log2_slots=12):
        from indelminer_amd import capi
        self.capi = capi
        self.ctx = capi.Context(0)
        self.ctx.set_reference(contigs())
        self.ctx.pairlink_enable(q, log2_slots)
        self.q = q
        self.keep = []

    def records(self, raw, off):
        capi = self.capi
        d_raw = capi.DevBuf(self.ctx, len(raw) + 64).upload(raw)
        d_off = capi.DevBuf(self.ctx, 4 * len(off)).upload(off)
        self.keep += [d_raw, d_off]
        return capi.DevRecords(len(off) - 1, d_raw.ptr, d_off.ptr, 0)

    def scatter(self, recs, qual=True):
        self.ctx.pairlink_scatter(self.records(*pk.pack_records(recs, qual)))

    def sync(self):
        self.ctx._check(self.capi.lib().im_stream_sync(self.ctx.h, self.ctx.stream))

    def add(self, links):
        for tid in range(len(CLENS)):
            mine = [x for x in links if x[0] == tid]
            self.ctx.pairlink_add(tid, [p for _, _, p, _ in mine], [m for _, _, _, m in mine], [k for _, k, _, _ in mine])

    def count(self, tid, queries, min_sep=0):
        """queries: [(kind, a0, a1, b0, b1)]"""
        return [int(x) for x in self.ctx.pairlink_count(tid, *[[q[k] for q in queries] for k in range(5)], min_sep)]

    def close(self):
        for b in self.keep:
            b.free()
        self.ctx.close()


def check(dev, links, rng, n_random=60, min_seps=(0, 50)):
    """the table holds exactly `links`: the stored count, every link where it is, and windows of every width against the restatement"""
    assert dev.ctx.pairlink_stats() == (len(links), 0)
    for tid in range(len(CLENS)):
        clen = CLENS[tid]
        queries = [(k, p, p, m, m) for t, k, p, m in set(links) if t == tid]
        queries += [(k, -5, 65_530, -5, clen + 5) for k in range(3)] + [(k, 65_531, 131_066, 0, clen) for k in range(3)] + [(k, 131_067, clen + 9, 0, clen) for k in range(3)]
        for _ in range(n_random):
            a0, b0 = int(rng.integers(-300, clen + 300)), int(rng.integers(-300, clen + 300))
            queries.append((int(rng.integers(0, 3)), a0, a0 + int(rng.choice([0, 1, 255, 256, 700, 1_032, 65_535])), b0, b0 + int(rng.choice([0, 1, 300, 1_032, 200_000]))))
        for sep in min_seps:
            want = [pk.count(links, CLENS, tid, *q, sep) for q in queries]
            got = dev.count(tid, queries, sep)
            assert got == want, (tid, sep, [(q, g, w) for q, g, w in zip(queries, got, want) if g != w][:6])


# ------------------------------------------------------------------------------------------ the scatter

def rule_edges():
    """one record per edge of the record rule (tests/test_pairlink_host.py works the same ones by hand)"""
    r = lambda **kw: Rec(**dict(dict(tid=0, pos=100, mapq=60, flag=0x1 | 0x10 | 0x40, mtid=0, mpos=400), **kw))
    out = [r()]
    out += [r(flag=0x1 | 0x10 | 0x40 | bit) for bit in (0x4, 0x8, 0x100, 0x200, 0x400, 0x800)] + [r(flag=0x10 | 0x40), r(flag=0x1 | 0x2 | 0x10 | 0x80)]
    out += [r(flag=0x1 | 0x10), r(flag=0x1), r(flag=0x1 | 0x10 | 0x20), r(flag=0x1 | 0x20), r(flag=0x1 | 0x20, mpos=90_000)]
    out += [r(pos=400, mpos=100), r(pos=300, mpos=300, flag=0x1 | 0x40), r(pos=300, mpos=300, flag=0x1 | 0x80)]
    out += [r(mapq=9), r(mapq=10), r(mtid=1), r(mtid=-1), r(tid=1, mtid=1), r(tid=3, mtid=3), r(tid=-1, mtid=-1)]
    out += [r(pos=0), r(pos=-1), r(mpos=150_000), r(mpos=150_001), r(pos=150_000, mpos=150_000), r(pos=150_001, mpos=150_001)]
    out += [r(tid=1, mtid=1, mpos=5_000), r(tid=1, mtid=1, mpos=5_001), r(tid=2, mtid=2, pos=0, mpos=70), r(tid=2, mtid=2, pos=70, mpos=71)]
    out += [r(pos=255, mpos=600), r(pos=256, mpos=600), r(pos=257, mpos=600)]
    return out


def random_records(rng, n):
    """records around every edge of the rule: mostly pairs in the normal orientation, as in a real chunk"""
    out = []
    for _ in range(n):
        tid = int(rng.choice([0, 0, 0, 0, 1, 1, 2, 3, -1]))
        clen = CLENS[tid] if 0 <= tid < 3 else 1_000
        pos, mpos = (int(rng.choice([rng.integers(0, clen + 1), 0, clen, clen + 1, -1], p=[0.9, 0.03, 0.03, 0.02, 0.02])) for _ in range(2))
        if rng.random() < 0.05:
            mpos = pos
        flag = 0x1 | int(rng.choice([0x40, 0x80]))
        flag |= int(rng.choice([0x20, 0x20, 0x20, 0, 0x10, 0x30]))
        if rng.random() < 0.12:
            flag |= int(rng.choice([0x4, 0x8, 0x100, 0x200, 0x400, 0x800, 0x2]))
        if rng.random() < 0.03:
            flag &= ~0x1
        out.append(Rec(tid, pos, int(rng.choice([60, 60, 60, 10, 9, 0])), flag, tid if rng.random() < 0.93 else int(rng.integers(-1, 3)), mpos))
    return out


def test_scatter_against_the_restatement_at_every_chunk_size_and_in_both_record_forms():
    rng = np.random.default_rng(5)
    dev = Device(q=10, log2_slots=12)
    try:
        edges = rule_edges()
        assert len(pk.links_of(edges, CLENS, 10)) == 16
        for n in (1, 63, 64, 65, 1_023, 1_024, 1_025, 2_049):
            for qual in (True, False):
                recs = (edges + random_records(rng, n))[-n:] if n < len(edges) else edges + random_records(rng, n - len(edges))
                if n == 1:
                    recs = [edges[0]]
                assert len(recs) == n
                links = pk.links_of(recs, CLENS, 10)
                assert n < 64 or len(links) >= n // 16
                dev.ctx.pairlink_reset()
                dev.scatter(recs, qual)
                dev.sync()
                check(dev, links, rng, n_random=25)
        # a chunk without a link stores nothing and draws no ticket; a second chunk adds to what the first left
        plain = [Rec(0, 100 + i, 60, 0x1 | 0x20 | 0x40, 0, 400 + i) for i in range(1_500)]
        assert pk.links_of(plain, CLENS, 10) == []
        dev.ctx.pairlink_reset()
        dev.scatter(plain)
        dev.sync()
        assert dev.ctx.pairlink_stats() == (0, 0)
        dev.scatter(edges); dev.scatter(plain, qual=False); dev.scatter(edges, qual=False)
        dev.sync()
        check(dev, 2 * pk.links_of(edges, CLENS, 10), rng, n_random=25)
    finally:
        dev.close()
    dev = Device(q=61, log2_slots=6)         # mapq is the enable's: at q = 61 nothing is a link
    try:
        dev.scatter(edges)
        dev.sync()
        assert dev.ctx.pairlink_stats() == (0, 0) and pk.links_of(edges, CLENS, 61) == []
    finally:
        dev.close()


# ------------------------------------------------------------------------------------------ count queries

def test_count_buckets_windows_and_clipping():
    rng = np.random.default_rng(8)
    dev = Device(log2_slots=12)
    try:
        links = []
        # buckets with 1, 63, 64, 65 and 130 links: a probe run of one batch, of exactly one, of two and of three
        for k, n in enumerate((1, 63, 64, 65, 130)):
            base = 256 * (4 + 10 * k)
            links += [(0, EVERTED, base + int(p), base + 2_000 + i) for i, p in enumerate(rng.integers(0, 256, n))]
        # the bucket boundary
        links += [(0, FORWARD, 255, 900), (0, FORWARD, 256, 900), (0, FORWARD, 257, 900)]
        # the first and the last bucket of a window of 257, and the positions just outside it
        links += [(0, REVERSE, 256, 70_000), (0, REVERSE, 257, 70_000), (0, REVERSE, 65_792, 70_000), (0, REVERSE, 65_793, 70_000)]
        # the contig's ends, and a pair on contig 1 over contig 0's links
        links += [(0, EVERTED, 0, 0), (0, EVERTED, 0, 150_000), (0, EVERTED, 150_000, 150_000), (1, EVERTED, 0, 5_000), (2, FORWARD, 0, 70), (2, FORWARD, 70, 70)]
        links += [(1, FORWARD, 255, 900), (1, EVERTED, 256 * 4 + 7, 256 * 4 + 2_007)]
        dev.add(links)
        check(dev, links, rng)
        q = lambda tid, *a, sep=0: dev.count(tid, [a], sep)[0]
        for k, n in enumerate((1, 63, 64, 65, 130)):
            base = 256 * (4 + 10 * k)
            assert q(0, EVERTED, base, base + 255, 0, 150_000) == n
            assert q(0, EVERTED, base - 256, base - 1, 0, 150_000) == 0 and q(0, FORWARD, base, base + 255, 0, 150_000) == 0
        assert q(1, EVERTED, 256 * 4, 256 * 4 + 255, 0, 5_000) == 1                    # contig 1's own, not contig 0's
        assert [q(0, FORWARD, a0, a1, 900, 900) for a0, a1 in ((255, 255), (256, 256), (257, 257), (255, 256), (256, 257), (0, 255), (256, 511), (0, 511))] == [1, 1, 1, 2, 2, 1, 2, 3]
        # windows over 1, 2 and 257 buckets; a1 - a0 = 65 535 is the widest
        assert q(0, REVERSE, 256, 511, 0, 150_000) == 2 and q(0, REVERSE, 255, 256, 0, 150_000) == 1
        assert q(0, REVERSE, 257, 65_792, 0, 150_000) == 2 and q(0, REVERSE, 256, 65_791, 0, 150_000) == 2 and q(0, REVERSE, 258, 65_793, 0, 150_000) == 2
        assert (257 >> 8, 65_792 >> 8) == (1, 257)
        # clipped at 0 and at length; empty after the clip
        assert q(0, EVERTED, -100, 0, -100, 0) == 1 and q(0, EVERTED, -100, 0, 149_999, 200_000) == 1 and q(0, EVERTED, 149_999, 200_000, 150_000, 2_000_000_000) == 1
        assert q(0, EVERTED, -2_000_000_000, -2_000_000_000 + 65_535, 0, 150_000) == 0
        assert q(0, EVERTED, -100, -1, 0, 150_000) == 0 and q(0, EVERTED, 150_001, 150_100, 0, 150_000) == 0
        assert q(0, EVERTED, 0, 0, -7, -1) == 0 and q(0, EVERTED, 0, 0, 150_001, 150_002) == 0 and q(0, EVERTED, 5, 4, 0, 150_000) == 0 and q(0, EVERTED, 0, 5, 9, 8) == 0
        assert q(2, FORWARD, -5, 80, -5, 80) == 2 and q(2, FORWARD, 0, 69, 0, 70) == 1 and q(2, FORWARD, 0, 70, 0, 70, sep=1) == 1
        # min_sep at its edge
        assert q(0, FORWARD, 255, 257, 0, 1_000, sep=643) == 3 and q(0, FORWARD, 255, 257, 0, 1_000, sep=644) == 2 and q(0, FORWARD, 255, 257, 0, 1_000, sep=646) == 0
        assert dev.count(0, []) == []
    finally:
        dev.close()


def test_count_table_at_its_smallest_foreign_keys_wrap_around_overflow_and_reset():
    """64 slots: links of another contig, another kind and another bucket on the probe run of the bucket asked for, a run that starts on
    the table's last slots and goes on at its first; then more links than the table keeps"""
    homes = {}
    for tid in (0, 1):
        for bucket in range(0, CLENS[tid] // 256):
            for kind in range(3):
                homes.setdefault(home_slot(tid, bucket, kind, 6), []).append((tid, bucket, kind))
    run = homes[62]
    mine = next(k for k in run if k[0] == 0)
    other_tid = next(k for k in run + homes[63] if k[0] == 1)
    other_kind = next(k for k in run + homes[63] + homes[0] if k[0] == 0 and k[2] != mine[2] and k != mine)
    other_bucket = next(k for k in run + homes[63] if k[0] == 0 and k[1] != mine[1] and k not in (mine, other_kind))
    at = lambda key, i: (key[0], key[2], 256 * key[1] + i, 256 * key[1] + 300 + i)
    # interleaved, so that the run of `mine` has the others in between and passes the last slot
    links = []
    for i in range(5):
        links += [at(mine, i), at(other_tid, i), at(other_kind, i), at(other_bucket, i)]
    rng = np.random.default_rng(2)
    dev = Device(log2_slots=6)
    try:
        dev.add(links)
        check(dev, links, rng)
        for key in (mine, other_tid, other_kind, other_bucket):
            assert dev.count(key[0], [(key[2], 256 * key[1], 256 * key[1] + 255, 0, CLENS[key[0]])]) == [5], key
        # 17 more make 37: 32 stored, 5 dropped; no answer from then on
        more = [(0, FORWARD, 2_000 + 300 * i, 9_000) for i in range(12)]
        dev.add(more)
        check(dev, links + more, rng, n_random=10)
        assert dev.ctx.pairlink_stats() == (32, 0)
        dev.add([(1, REVERSE, 100 + i, 200 + i) for i in range(5)])
        assert dev.ctx.pairlink_stats() == (32, 5)
        assert dev.count(0, [(mine[2], 0, 65_535, 0, 150_000), (FORWARD, 2_000, 2_000, 9_000, 9_000), (EVERTED, -9, -1, 0, 0)]) == [NONE] * 3
        assert dev.count(1, [(REVERSE, 0, 5_000, 0, 5_000)]) == [NONE] and dev.count(2, [(REVERSE, 0, 70, 0, 70)]) == [NONE]
        dev.ctx.pairlink_reset()
        assert dev.ctx.pairlink_stats() == (0, 0) and dev.count(0, [(mine[2], 0, 65_535, 0, 150_000)]) == [0]
        dev.add(links)
        check(dev, links, rng, n_random=10)
    finally:
        dev.close()


def test_pairlink_arguments():
    from indelminer_amd import capi
    lib, ptr = capi.lib(), lambda a: a.ctypes.data_as(C.c_void_p)
    kind, out = np.zeros(2, np.uint8), np.full(2, 77, np.uint32)
    a0, a1, b0, b1 = (np.array(v, np.int32) for v in ([0, 10], [65_535, 20], [0, 0], [100, 100]))
    count = lambda h, tid, nq, k, w, x, y, z, sep, o: lib.im_pairlink_count(h, tid, nq, *[None if v is None else ptr(v) for v in (k, w, x, y, z)], sep, None if o is None else ptr(o))
    recs = capi.DevRecords(0, None, None, 0)
    ctx = capi.Context(0)
    try:
        assert lib.im_pairlink_enable(ctx.h, 10, 8) != 0 and lib.im_last_error(ctx.h) == b"im_set_reference has not been called"
        ctx.set_reference(contigs())
        # every entry before the enable
        assert lib.im_dev_pairlink_scatter(ctx.h, C.byref(recs), None) != 0 and lib.im_last_error(ctx.h) == b"im_pairlink_enable has not been called"
        assert count(ctx.h, 0, 2, kind, a0, a1, b0, b1, 0, out) != 0 and lib.im_last_error(ctx.h) == b"im_pairlink_enable has not been called"
        assert lib.im_pairlink_add(ctx.h, 0, 0, None, None, None) != 0 and lib.im_pairlink_reset(ctx.h, None) != 0
        stored, dropped = C.c_uint64(0), C.c_uint64(0)
        assert lib.im_pairlink_stats(ctx.h, C.byref(stored), C.byref(dropped)) != 0
        for k in (5, 31, -1):
            assert lib.im_pairlink_enable(ctx.h, 10, k) != 0 and b"log2_slots" in lib.im_last_error(ctx.h)
        assert lib.im_pairlink_enable(None, 10, 8) != 0
        ctx.pairlink_enable(10, 8)
        ctx.pairlink_enable(10, 8)                                  # the same values again: fine
        assert lib.im_pairlink_enable(ctx.h, 11, 8) != 0 and b"already enabled with min_mapq 10, log2_slots 8" in lib.im_last_error(ctx.h)
        assert lib.im_pairlink_enable(ctx.h, 10, 9) != 0
        # count
        assert count(ctx.h, 0, 2, kind, a0, a1, b0, b1, 0, out) == 0 and list(out) == [0, 0]
        wide = a1.copy(); wide[0] = 65_536
        assert count(ctx.h, 0, 2, kind, a0, wide, b0, b1, 0, out) != 0 and b"query 0: a1 - a0 = 65536" in lib.im_last_error(ctx.h)
        low = a0.copy(); low[1] = -2_000_000_000; high = a1.copy(); high[1] = 2_000_000_000
        assert count(ctx.h, 0, 2, kind, low, high, b0, b1, 0, out) != 0 and b"query 1: a1 - a0 = 4000000000" in lib.im_last_error(ctx.h)
        bad = kind.copy(); bad[1] = 3
        assert count(ctx.h, 0, 2, bad, a0, a1, b0, b1, 0, out) != 0 and b"query 1: kind 3" in lib.im_last_error(ctx.h)
        assert count(ctx.h, 0, 2, kind, a0, a1, b0, b1, -1, out) != 0 and b"min_sep -1" in lib.im_last_error(ctx.h)
        assert count(ctx.h, 3, 2, kind, a0, a1, b0, b1, 0, out) != 0 and count(ctx.h, -1, 2, kind, a0, a1, b0, b1, 0, out) != 0
        assert count(ctx.h, 0, -1, kind, a0, a1, b0, b1, 0, out) != 0 and count(None, 0, 2, kind, a0, a1, b0, b1, 0, out) != 0
        for k in range(6):
            args = [kind, a0, a1, b0, b1, out]; args[k] = None
            assert count(ctx.h, 0, 2, *args[:5], 0, args[5]) != 0, k
        assert count(ctx.h, 0, 0, None, None, None, None, None, 0, None) == 0
        # add
        pos = np.array([5, 6], np.int32)
        assert lib.im_pairlink_add(ctx.h, 0, 2, ptr(pos), ptr(pos), ptr(bad)) != 0 and b"link 1: kind 3" in lib.im_last_error(ctx.h)
        assert lib.im_pairlink_add(ctx.h, 3, 2, ptr(pos), ptr(pos), ptr(kind)) != 0 and lib.im_pairlink_add(ctx.h, -1, 2, ptr(pos), ptr(pos), ptr(kind)) != 0
        assert lib.im_pairlink_add(ctx.h, 0, -1, ptr(pos), ptr(pos), ptr(kind)) != 0 and lib.im_pairlink_add(None, 0, 2, ptr(pos), ptr(pos), ptr(kind)) != 0
        for k in range(3):
            args = [ptr(pos), ptr(pos), ptr(kind)]; args[k] = None
            assert lib.im_pairlink_add(ctx.h, 0, 2, *args) != 0, k
        assert lib.im_pairlink_add(ctx.h, 0, 0, None, None, None) == 0 and ctx.pairlink_stats() == (0, 0)
        # positions outside [0, length] are dropped without a ticket
        ctx.pairlink_add(2, [0, -1, 5, 5, 71], [70, 5, 71, -1, 71], [0, 0, 0, 0, 0])
        assert ctx.pairlink_stats() == (1, 0) and list(ctx.pairlink_count(2, [0], [0], [70], [0], [70])) == [1]
        # scatter, reset, stats
        assert lib.im_dev_pairlink_scatter(ctx.h, None, None) != 0 and lib.im_dev_pairlink_scatter(None, C.byref(recs), None) != 0
        neg = capi.DevRecords(-1, None, None, 0)
        assert lib.im_dev_pairlink_scatter(ctx.h, C.byref(neg), None) != 0 and lib.im_last_error(ctx.h) == b"negative record count"
        assert lib.im_dev_pairlink_scatter(ctx.h, C.byref(recs), None) == 0              # no record: no launch
        assert lib.im_pairlink_reset(None, None) != 0 and lib.im_pairlink_stats(None, C.byref(stored), C.byref(dropped)) != 0
        assert lib.im_pairlink_stats(ctx.h, None, C.byref(dropped)) != 0 and lib.im_pairlink_stats(ctx.h, C.byref(stored), None) != 0
        # a new reference takes the table with it
        ctx.set_reference(contigs())
        assert lib.im_pairlink_reset(ctx.h, None) != 0
        ctx.pairlink_enable(11, 9)
    finally:
        ctx.close()


# ------------------------------------------------------------------------------------------ the soak

def soak_records(seed, n_records=20_000, n_hot=300):
    """records whose positions are drawn from 300 hot positions (and their neighbours), so that buckets hold tens of links of every kind
    on two contigs and four of them more than a hundred, among pairs in the normal orientation and records the rule excludes"""
    rng = np.random.default_rng(seed)
    hot = [(0, int(p)) for p in rng.integers(0, 150_000, n_hot - 30)] + [(1, int(p)) for p in rng.integers(0, 5_000, 30)]
    out = []
    for _ in range(n_records):
        tid, p = hot[int(rng.integers(0, 4))] if rng.random() < 0.2 else hot[int(rng.integers(0, n_hot))]     # four of them hotter than a batch of the walk
        _, m = hot[int(rng.integers(0, n_hot - 30))] if tid == 0 else hot[n_hot - 30 + int(rng.integers(0, 30))]
        p += int(rng.choice([0, 0, 0, 1, -1, 7, 255, 256])); m += int(rng.choice([0, 0, 1, 40]))
        flag = 0x1 | int(rng.choice([0x40, 0x80])) | int(rng.choice([0x20, 0x20, 0, 0x10, 0x30]))
        if rng.random() < 0.05:
            flag |= int(rng.choice([0x4, 0x8, 0x100, 0x400, 0x800]))
        out.append(Rec(tid, p, int(rng.choice([60, 60, 10, 9])), flag, tid if rng.random() < 0.97 else 1 - tid, m))
    return out


def test_seeded_soak_scatter_against_add():
    """20 000 records through im_dev_pairlink_scatter in three launches, both record forms, against the same links through im_pairlink_add"""
    recs = soak_records(17)
    links = pk.links_of(recs, CLENS, 10)
    assert len(recs) == 20_000 and 4_000 < len(links) < 8_192
    buckets = {}
    for t, k, p, m in links:
        buckets[(t, k, p >> 8)] = buckets.get((t, k, p >> 8), 0) + 1
    assert max(buckets.values()) > 64                               # some probe run of one key is longer than a batch
    rng = np.random.default_rng(18)
    queries = {tid: [(int(rng.integers(0, 3)), a0, a0 + int(rng.choice([0, 300, 1_032, 65_535])), b0, b0 + int(rng.choice([0, 1_032, 150_000])))
                     for a0, b0 in zip(rng.integers(-500, CLENS[tid], 400), rng.integers(-500, CLENS[tid], 400))] for tid in (0, 1)}
    answers = []
    for how in ("scatter", "add"):
        dev = Device(log2_slots=14)
        try:
            if how == "scatter":
                cuts = [0, 7_000, 13_001, len(recs)]
                for k in range(3):
                    dev.scatter(recs[cuts[k]:cuts[k + 1]], qual=k != 1)
                dev.sync()
            else:
                dev.add(links)
            assert dev.ctx.pairlink_stats() == (len(links), 0)
            answers.append({(tid, sep): dev.count(tid, queries[tid], sep) for tid in (0, 1) for sep in (0, 50)})
        finally:
            dev.close()
    assert answers[0] == answers[1]
    for (tid, sep), got in answers[0].items():
        assert got == [pk.count(links, CLENS, tid, *q, sep) for q in queries[tid]], (tid, sep)
    assert sum(sum(v) for v in answers[0].values()) > 10_000


# ------------------------------------------------------------------------------------------ the product

def _run(binary, flags, cwd, env=None):
    e = dict(os.environ)
    e.update(env or {})
    return subprocess.run([binary] + flags + ["ref.fa", "sample=aln.bam"], cwd=cwd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=e)


def _ok(r):
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    assert b"overflowed" not in r.stderr
    return r


BASE = ["-i", "cfg.txt", "-s", "100"]
ENVS = ({"INDELMINER_PIPELINE": "host"}, {"INDELMINER_PIECE_BYTES": "60000", "INDELMINER_WALKERS": "3"})


@pytest.mark.parametrize("svtype", ["DUP", "INV"])
def test_product_pe_in_both_files(svtype, tmp_path):
    """the planted duplications (svtype DUP) or inversions (INV) with their planted pairs: the FILE of the option that finds them, and
    the other option's, which holds the header alone there or whatever chance gives it -- both byte for byte the restatement's"""
    from tests.test_gpu_depth_evidence import depth_of_bam
    refs, rd, planted = pk.planted_dup_reads() if svtype == "DUP" else pk.planted_inv_reads()
    d = pk.write_planted(str(tmp_path), refs, rd)
    bam, fa = d + "/aln.bam", d + "/ref.fa"
    dup_plain, dup_pe, dup_found = pk.render_of_bam("DUP", bam, fa, 10)
    inv_plain, inv_pe, inv_found = pk.render_of_bam("INV", bam, fa, 10)
    dup_plain_d, dup_pe_d, _ = pk.render_of_bam("DUP", bam, fa, 10, depth_of_bam(bam)[1])
    # the figures of tests/test_pairlink_host.py
    found = dup_found if svtype == "DUP" else inv_found
    assert len(found) == (9 if svtype == "DUP" else 18) and [f[4] for f in found] == [0] * (len(found) * 5 // 9) + [3] * (len(found) * 4 // 9)
    assert len(dup_found if svtype == "INV" else inv_found) == 0
    prod = _product()
    path = lambda name: str(tmp_path / name)
    read = lambda name: open(path(name), "rb").read()
    # without -M both files are what they are today; with it stdout, stderr and -I's FILE do not change
    r0 = _ok(_run(prod, BASE + ["-G", "-C", "-V", "-I", path("i0"), "-U", path("u0"), "-N", path("n0")], d))
    r1 = _ok(_run(prod, BASE + ["-G", "-C", "-V", "-I", path("i1"), "-U", path("u1"), "-N", path("n1"), "-M"], d))
    assert read("u0") == dup_plain and read("n0") == inv_plain
    assert read("u1") == dup_pe and read("n1") == inv_pe
    assert r1.stdout == r0.stdout and r1.stderr == r0.stderr and read("i1") == read("i0") and len(r0.stdout) > 1000
    assert read("u1" if svtype == "DUP" else "n1").count(b";PE=3\n") == len(found) * 4 // 9
    # -U alone and -N alone
    _ok(_run(prod, BASE + ["-G", "-C", "-V", "-M", "-U", path("u2")], d))
    _ok(_run(prod, BASE + ["-G", "-C", "-V", "-N", path("n2"), "-M"], d))
    assert read("u2") == dup_pe and read("n2") == inv_pe
    # the record-at-a-time path and three walkers on small pieces write the same bytes
    for k, env in enumerate(ENVS):
        r = _ok(_run(prod, BASE + ["-G", "-C", "-V", "-U", path("u3%d" % k), "-N", path("n3%d" % k), "-M"], d, env=env))
        assert read("u3%d" % k) == dup_pe and read("n3%d" % k) == inv_pe and r.stdout == r0.stdout, env
    # with -D: PE stands behind -U's depth fields, -N's FILE has none
    rd0 = _ok(_run(prod, BASE + ["-G", "-D", "-C", "-V", "-U", path("u4"), "-N", path("n4")], d))
    rd1 = _ok(_run(prod, BASE + ["-G", "-D", "-C", "-V", "-U", path("u5"), "-N", path("n5"), "-M"], d))
    assert read("u4") == dup_plain_d and read("u5") == dup_pe_d and read("n4") == inv_plain and read("n5") == inv_pe
    assert rd1.stdout == rd0.stdout and rd1.stderr == rd0.stderr
    if svtype == "DUP":
        assert b";DFC=" in dup_pe_d and all(ln.split(b";")[-2].startswith(b"DFC=") for ln in dup_pe_d.split(b"\n") if b"<DUP:TANDEM>" in ln)


def test_product_detailed_output_ignores_the_option_and_it_is_refused_alone(tmp_path):
    refs, rd, _ = pk.planted_dup_reads()
    d = pk.write_planted(str(tmp_path), refs, rd)
    prod = _product()
    fo = str(tmp_path / "none.vcf")
    d0 = _ok(_run(prod, BASE + ["-o", "detailed"], d))
    d1 = _ok(_run(prod, BASE + ["-o", "detailed", "-G", "-C", "-V", "-U", fo, "-M"], d))
    assert d1.stdout == d0.stdout and d1.stderr == d0.stderr and len(d0.stdout) > 0 and not os.path.exists(fo)
    r = _run(prod, BASE + ["-G", "-C", "-V", "-M"], d)
    assert r.returncode != 0 and r.stdout == b"" and r.stderr == b"indelminer: -M needs -U or -N\n"
    r = _run(prod, BASE + ["-G", "-C", "-V", "-I", fo, "-M"], d)
    assert r.returncode != 0 and r.stdout == b"" and r.stderr == b"indelminer: -M needs -U or -N\n" and not os.path.exists(fo)


def test_product_after_an_overflow_of_the_link_table(tmp_path):
    """2 100 everted pairs against the 2 048 links the table of a small BAM keeps: the records are still printed, every PE is ., and
    stderr says so once, at the end"""
    refs, rd = pk.planted_overflow_reads()
    d = pk.write_planted(str(tmp_path), refs, rd)
    names, clens, links = pk.links_of_bam(d + "/aln.bam", 10)
    assert len(links) == 2_100 and os.path.getsize(d + "/aln.bam") < 64 << 16
    plain = pk.render_of_bam("DUP", d + "/aln.bam", d + "/ref.fa", 10)[0]
    want = pk.with_pe(plain, "DUP", names, clens, links, overflowed=True)[0]
    assert want.count(b";PE=.\n") == 9
    prod = _product()
    f0, f1 = str(tmp_path / "u0"), str(tmp_path / "u1")
    r0 = _ok(_run(prod, BASE + ["-G", "-C", "-V", "-U", f0], d))
    r1 = _run(prod, BASE + ["-G", "-C", "-V", "-U", f1, "-M"], d)
    assert r1.returncode == 0 and open(f0, "rb").read() == plain and open(f1, "rb").read() == want
    line = b"indelminer: -M: the pair-link table overflowed (2048 links stored, 52 dropped): PE is . in the files of -U and -N\n"
    assert r1.stdout == r0.stdout and r1.stderr == r0.stderr + line


def test_product_record_at_a_time_chunk_edges(tmp_path):
    """The record-at-a-time path hands its records to the scatters in chunks (run_contig).  The planted duplications, 18 000 records,
    with every evidence option on, at caps of records per chunk that cut inside every launch shape: one record per launch, the
    one-wave scatters' workgroup (64), the 256-record scatter workgroup with its LDS window, one past it, and the default (one chunk).
    stdout, stderr and the three FILEs are the same bytes in all five runs, the default pipelined run's, and the restatement's."""
    from tests.test_gpu_depth_evidence import depth_of_bam
    refs, rd, _ = pk.planted_dup_reads()
    assert rd.n <= 20_000
    d = pk.write_planted(str(tmp_path), refs, rd)
    bam, fa = d + "/aln.bam", d + "/ref.fa"
    dup_pe_d = pk.render_of_bam("DUP", bam, fa, 10, depth_of_bam(bam)[1])[1]
    inv_pe = pk.render_of_bam("INV", bam, fa, 10)[1]
    prod = _product()

    def leg(k, env):
        files = [str(tmp_path / ("%s%d" % (f, k))) for f in "iun"]
        flags = BASE + ["-G", "-P", "-D", "-C", "-V", "-I", files[0], "-U", files[1], "-N", files[2], "-M"]
        r = subprocess.run([prod] + flags + ["ref.fa", "sample=aln.bam"], cwd=d, stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                           env=dict(os.environ, **env), timeout=120)
        _ok(r)
        return [r.stdout, r.stderr] + [open(f, "rb").read() for f in files]

    want = leg(0, {})
    assert want[3] == dup_pe_d and want[4] == inv_pe and want[3].count(b";PE=3\n") == 4 and len(want[0]) > 1000
    for k, cap in enumerate(("1", "64", "256", "257", None), 1):
        env = {"INDELMINER_PIPELINE": "host"}
        if cap is not None:
            env["INDELMINER_HOST_CHUNK_RECS"] = cap
        assert leg(k, env) == want, cap
