"""Breakpoints between contigs (-T): the scatter, add and partner kernels of im_links.hip behind the six im_matelink_* entries, the
junction kernel of im_cliptail.hip behind im_cliptail_junction, and what the host driver makes of them (-T's FILE).

The yardstick is the plain restatement in tests/support/intercontig.py, written from the definitions in include/indelminer_amd.h (seam 5,
"Mate links" and "Junctions"), not from the code under test; tests/test_intercontig_host.py pins it to cases worked by hand.  Every answer
is compared exactly.
"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests.support import cliptails as ct
from tests.support import intercontig as ic
from tests.support.intercontig import NONE, Rec
from tests.support.spanarrays import _product

pytestmark = pytest.mark.gpu

CLENS = [150_000, 300_000, 70, 5_000]


def contigs(seed=3):
    rng = np.random.default_rng(seed)
    return [bytes(rng.choice(np.frombuffer(b"ACGT", np.uint8), n)) for n in CLENS]


class Device:
    """one context over four contigs with the mate-link table enabled"""

    def __init__(self, q=10, log2_slots=12):
        from indelminer_amd import capi
        self.capi = capi
        self.ctx = capi.Context(0)
        self.ctx.set_reference(contigs())
        self.ctx.matelink_enable(q, log2_slots)
        self.keep = []

    def records(self, raw, off):
        capi = self.capi
        d_raw = capi.DevBuf(self.ctx, len(raw) + 64).upload(raw)
        d_off = capi.DevBuf(self.ctx, 4 * len(off)).upload(off)
        self.keep += [d_raw, d_off]
        return capi.DevRecords(len(off) - 1, d_raw.ptr, d_off.ptr, 0)

    def scatter(self, recs, qual=True):
        self.ctx.matelink_scatter(self.records(*ic.pack_records(recs, qual)))

    def sync(self):
        self.ctx._check(self.capi.lib().im_stream_sync(self.ctx.h, self.ctx.stream))

    def add(self, links):
        for tid in range(len(CLENS)):
            mine = [x for x in links if x[0] == tid]
            self.ctx.matelink_add(tid, [x[2] for x in mine], [x[3] for x in mine], [x[4] for x in mine], [x[1] for x in mine])

    def partner(self, tid, queries):
        """queries: [(kind, a0, a1)] -> [(n_links, mtid, n_partner, lo, hi)]"""
        out = self.ctx.matelink_partner(tid, *[[q[k] for q in queries] for k in range(3)])
        return [tuple(int(o[i]) for o in out) for i in range(len(queries))]

    def close(self):
        for b in self.keep:
            b.free()
        self.ctx.close()


def check(dev, links, rng, n_random=40):
    """the table holds exactly `links`: the stored count, and windows of every width on every contig against the restatement"""
    assert dev.ctx.matelink_stats() == (len(links), 0)
    for tid in range(len(CLENS)):
        clen = CLENS[tid]
        queries = [(k, p, p) for t, k, p, _, _ in set(links) if t == tid][:60]
        queries += [(k, a0, a0 + 65_535) for k in range(4) for a0 in range(-5, clen + 10, 65_536)]        # the whole contig, in the widest windows
        for _ in range(n_random):
            a0 = int(rng.integers(-300, clen + 300))
            queries.append((int(rng.integers(0, 4)), a0, a0 + int(rng.choice([0, 1, 255, 256, 700, 1_032, 65_535]))))
        want = [ic.partner(links, CLENS, tid, *q) for q in queries]
        got = dev.partner(tid, queries)
        assert got == want, (tid, [(q, g, w) for q, g, w in zip(queries, got, want) if g != w][:6])


# ------------------------------------------------------------------------------------------ the scatter

def rule_edges():
    """one record per edge of the record rule (tests/test_intercontig_host.py works the same ones by hand)"""
    r = lambda **kw: Rec(**dict(dict(tid=0, pos=100, mapq=60, flag=0x1 | 0x40, mtid=1, mpos=400), **kw))
    out = [r()] + [r(flag=0x1 | f) for f in (0x10, 0x20, 0x30, 0x80, 0x2 | 0x40)]
    out += [r(flag=0x1 | 0x40 | bit) for bit in (0x4, 0x8, 0x100, 0x200, 0x400, 0x800)] + [r(flag=0x40)]
    out += [r(mtid=0), r(tid=1, mtid=1), r(mtid=-1), r(mtid=4), r(tid=-1), r(tid=4), r(mtid=3, mpos=5_000), r(mtid=3, mpos=5_001)]
    out += [r(mapq=9), r(mapq=10)]
    out += [r(pos=0), r(pos=-1), r(pos=150_000), r(pos=150_001), r(mpos=0), r(mpos=-1), r(mpos=300_000), r(mpos=300_001)]
    out += [r(mtid=2, mpos=70), r(mtid=2, mpos=71), r(tid=2, pos=70, mtid=0, mpos=150_000), r(tid=2, pos=71, mtid=0)]
    out += [r(tid=1, pos=400, mtid=0, mpos=100, flag=0x1 | 0x80 | 0x30)]
    out += [r(pos=255, mpos=1_023), r(pos=256, mpos=1_024), r(pos=257, mpos=2_047)]
    return out


def random_records(rng, n):
    """records around every edge of the rule: one in three with its mate on another contig"""
    out = []
    for _ in range(n):
        tid = int(rng.choice([0, 0, 0, 1, 1, 2, 3, 4, -1]))
        mtid = tid if rng.random() < 0.65 else int(rng.choice([0, 0, 1, 1, 2, 3, 4, -1]))
        length = lambda t: CLENS[t] if 0 <= t < 4 else 1_000
        pos, mpos = (int(rng.choice([rng.integers(0, length(t) + 1), 0, length(t), length(t) + 1, -1], p=[0.9, 0.03, 0.03, 0.02, 0.02])) for t in (tid, mtid))
        flag = 0x1 | int(rng.choice([0x40, 0x80])) | int(rng.choice([0x20, 0, 0x10, 0x30]))
        if rng.random() < 0.12:
            flag |= int(rng.choice([0x4, 0x8, 0x100, 0x200, 0x400, 0x800, 0x2]))
        if rng.random() < 0.03:
            flag &= ~0x1
        out.append(Rec(tid, pos, int(rng.choice([60, 60, 60, 10, 9, 0])), flag, mtid, mpos))
    return out


def test_scatter_against_the_restatement_at_every_chunk_size_and_in_both_record_forms():
    rng = np.random.default_rng(5)
    dev = Device(q=10, log2_slots=12)
    try:
        edges = rule_edges()
        assert len(ic.links_of(edges, CLENS, 10)) == 18
        for n in (1, 63, 64, 65, 1_023, 1_024, 1_025):
            for qual in (True, False):
                recs = (edges + random_records(rng, n))[-n:] if n < len(edges) else edges + random_records(rng, n - len(edges))
                if n == 1:
                    recs = [edges[0]]
                assert len(recs) == n
                links = ic.links_of(recs, CLENS, 10)
                assert n < 64 or len(links) >= n // 16
                dev.ctx.matelink_reset()
                dev.scatter(recs, qual)
                dev.sync()
                check(dev, links, rng, n_random=15)
        # a chunk without a link stores nothing and draws no ticket; a second chunk adds to what the first left
        plain = [Rec(0, 100 + i, 60, 0x1 | 0x20 | 0x40, 0, 400 + i) for i in range(1_500)]
        assert ic.links_of(plain, CLENS, 10) == []
        dev.ctx.matelink_reset()
        dev.scatter(plain)
        dev.sync()
        assert dev.ctx.matelink_stats() == (0, 0)
        dev.scatter(edges); dev.scatter(plain, qual=False); dev.scatter(edges, qual=False)
        dev.sync()
        check(dev, 2 * ic.links_of(edges, CLENS, 10), rng, n_random=15)
    finally:
        dev.close()
    dev = Device(q=61, log2_slots=6)         # mapq is the enable's: at q = 61 nothing is a link
    try:
        dev.scatter(edges)
        dev.sync()
        assert dev.ctx.matelink_stats() == (0, 0) and ic.links_of(edges, CLENS, 61) == []
    finally:
        dev.close()


def soak_records(seed, n_records=20_000, n_hot=300):
    """records whose positions are drawn from 300 hot positions (and their neighbours) on two contigs, a third of them with the mate on
    another contig, so that buckets hold tens of links of every kind and some more than a batch of the walk"""
    rng = np.random.default_rng(seed)
    hot = [(0, int(p)) for p in rng.integers(0, 150_000, n_hot - 30)] + [(1, int(p)) for p in rng.integers(0, 300_000, 30)]
    out = []
    for _ in range(n_records):
        tid, p = hot[int(rng.integers(0, 4))] if rng.random() < 0.2 else hot[int(rng.integers(0, n_hot))]
        mtid, m = hot[int(rng.integers(0, n_hot))]
        r = rng.random()
        if r < 0.35:                                                # the mate on the other of the two contigs
            mtid, m = hot[n_hot - 30 + int(rng.integers(0, 30))] if tid == 0 else hot[int(rng.integers(0, n_hot - 30))]
        elif r < 0.4:
            mtid, m = 3, int(rng.integers(0, 5_000))
        p += int(rng.choice([0, 0, 0, 1, -1, 7, 255, 256])); m += int(rng.choice([0, 0, 1, 40, 1_024]))
        flag = 0x1 | int(rng.choice([0x40, 0x80])) | int(rng.choice([0x20, 0, 0x10, 0x30]))
        if rng.random() < 0.05:
            flag |= int(rng.choice([0x4, 0x8, 0x100, 0x400, 0x800]))
        out.append(Rec(tid, p, int(rng.choice([60, 60, 10, 9])), flag, mtid, m))
    return out


def test_seeded_soak_scatter_against_add():
    """20 000 records through im_dev_matelink_scatter in three launches, both record forms, against the same links through im_matelink_add"""
    recs = soak_records(17)
    links = ic.links_of(recs, CLENS, 10)
    assert len(recs) == 20_000 and 2_000 < len(links) < 8_192
    buckets = {}
    for t, k, p, _, _ in links:
        buckets[(t, k, p >> 8)] = buckets.get((t, k, p >> 8), 0) + 1
    assert max(buckets.values()) > 64                               # some probe run of one key is longer than a batch
    rng = np.random.default_rng(18)
    queries = {tid: [(int(rng.integers(0, 4)), a0, a0 + int(rng.choice([0, 300, 1_032, 65_535]))) for a0 in rng.integers(-500, CLENS[tid], 300)] for tid in (0, 1)}
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
            assert dev.ctx.matelink_stats() == (len(links), 0)
            answers.append({tid: dev.partner(tid, queries[tid]) for tid in (0, 1)})
        finally:
            dev.close()
    assert answers[0] == answers[1]
    for tid, got in answers[0].items():
        assert got == [ic.partner(links, CLENS, tid, *q) for q in queries[tid]], tid
    assert sum(g[2] for got in answers[0].values() for g in got) > 2_000


# ------------------------------------------------------------------------------------------ partner queries

def test_partner_buckets_windows_cells_and_ties():
    rng = np.random.default_rng(8)
    dev = Device(log2_slots=13)
    try:
        L = lambda pos, mtid, mpos, kind=0, tid=0: (tid, kind, pos, mtid, mpos)
        links = []
        # buckets with 1, 63, 64, 65 and 130 links: a probe run of one batch, of exactly one, of two and of three
        for k, n in enumerate((1, 63, 64, 65, 130)):
            base = 256 * (4 + 10 * k)
            links += [L(base + int(p), 1, 50_000 * (k + 1) + i) for i, p in enumerate(rng.integers(0, 256, n))]
        # the bucket border 255 | 256, the first and the last bucket of a window of 257, the contig's ends
        links += [L(255, 1, 900, 1), L(256, 1, 901, 1), L(257, 1, 902, 1)]
        links += [L(256, 1, 70_000, 2), L(257, 1, 70_001, 2), L(65_792, 1, 70_002, 2), L(65_793, 1, 70_003, 2)]
        links += [L(0, 1, 0, 3), L(0, 1, 300_000, 3), L(150_000, 1, 5, 3), L(0, 0, 150_000, 3, tid=2), L(70, 3, 5_000, 3, tid=2)]
        # mates at 1 023, 1 024, 2 047 and 2 048; equal scores on two contigs and on two cells
        links += [L(100_000, 1, m, 1) for m in (1_023, 1_024, 2_047, 2_048)]
        links += [L(110_000, 3, 100, 1), L(110_001, 3, 101, 1), L(110_002, 1, 9_000, 1), L(110_003, 1, 9_001, 1)]
        links += [L(120_000, 1, 20_000, 1), L(120_001, 1, 20_001, 1), L(120_002, 1, 9_000, 1), L(120_003, 1, 9_001, 1)]
        links += [L(7, 0, 100, 0, tid=3), L(8, 1, 100, 0, tid=3)]
        dev.add(links)
        check(dev, links, rng)
        q = lambda tid, *a: dev.partner(tid, [a])[0]
        for k, n in enumerate((1, 63, 64, 65, 130)):
            base = 256 * (4 + 10 * k)
            assert q(0, 0, base, base + 255) == (n, 1, n, 50_000 * (k + 1), 50_000 * (k + 1) + n - 1)
            assert q(0, 0, base - 256, base - 1) == (0, -1, 0, 0, 0) and q(0, 1, base, base + 255) == (0, -1, 0, 0, 0)
        assert [q(0, 1, a0, a1)[0] for a0, a1 in ((255, 255), (256, 256), (257, 257), (255, 256), (256, 257), (0, 255), (256, 511), (0, 511))] == [1, 1, 1, 2, 2, 1, 2, 3]
        assert q(0, 1, 255, 256) == (2, 1, 2, 900, 901)
        # windows over 257 buckets; a1 - a0 = 65 535 is the widest
        assert q(0, 2, 257, 65_792) == (2, 1, 2, 70_001, 70_002) and q(0, 2, 256, 65_791)[0] == 2 and q(0, 2, 258, 65_793)[0] == 2
        # clipped at 0 and at length; empty after the clip
        assert q(0, 3, -100, 0) == (2, 1, 1, 0, 0) and q(0, 3, 149_999, 200_000) == (1, 1, 1, 5, 5)
        assert q(0, 3, -2_000_000_000, -2_000_000_000 + 65_535) == (0, -1, 0, 0, 0) and q(0, 3, 150_001, 150_100) == (0, -1, 0, 0, 0) and q(0, 3, 5, 4) == (0, -1, 0, 0, 0)
        assert q(2, 3, -5, 80) == (2, 0, 1, 150_000, 150_000) and q(2, 3, 1, 70) == (1, 3, 1, 5_000, 5_000)
        # two neighbouring cells count together; ties: the smaller contig, then the smaller cell
        assert q(0, 1, 100_000, 100_000) == (4, 1, 3, 1_023, 2_047)
        assert q(0, 1, 110_000, 110_003) == (4, 1, 2, 9_000, 9_001) and q(0, 1, 110_000, 110_002) == (3, 3, 2, 100, 101)
        assert q(0, 1, 120_000, 120_003) == (4, 1, 2, 9_000, 9_001) and q(0, 1, 120_000, 120_002) == (3, 1, 2, 20_000, 20_001)
        assert q(3, 0, 0, 100) == (2, 0, 1, 100, 100)
        assert dev.partner(0, []) == []
    finally:
        dev.close()


def test_partner_255_256_and_257_cells():
    dev = Device(log2_slots=12)
    try:
        cell = lambda c, pos: (0, 0, pos, 1, 1_024 * c + 7)
        links = [cell(c, 1_000 + c) for c in range(257)] + [(0, 0, 1_000, 1, 5)]
        links += [(0, 2, 2_000 + (c % 50), 1 + 2 * (c % 2), 1_024 * (c % 4) + c) for c in range(300)]       # 300 links in 8 cells
        dev.add(links)
        q = lambda *a: dev.partner(0, [a])[0]
        assert q(0, 1_000, 1_254) == ic.partner(links, CLENS, 0, 0, 1_000, 1_254) == (256, 1, 3, 5, 1_031)
        assert q(0, 1_000, 1_255) == ic.partner(links, CLENS, 0, 0, 1_000, 1_255) == (257, 1, 3, 5, 1_031)
        assert q(0, 1_000, 1_256) == ic.partner(links, CLENS, 0, 0, 1_000, 1_256) == (258, -2, 0, 0, 0)
        assert q(0, 1_001, 1_256) == ic.partner(links, CLENS, 0, 0, 1_001, 1_256) == (256, 1, 2, 1_031, 2_055)
        assert q(2, 2_000, 2_049) == ic.partner(links, CLENS, 0, 2, 2_000, 2_049) and q(2, 2_000, 2_049)[0] == 300
        # the order of arrival does not matter: the same links the other way round
        dev.ctx.matelink_reset()
        dev.add(links[::-1])
        assert q(0, 1_000, 1_255) == (257, 1, 3, 5, 1_031) and q(0, 1_000, 1_256) == (258, -2, 0, 0, 0)
        # several queries of one launch, capped and not, do not see each other's cells
        got = dev.partner(0, [(0, 1_000, 1_256), (0, 1_000, 1_010), (0, 1_000, 1_256), (2, 2_000, 2_049), (0, 1_100, 1_101)] * 3)
        assert got == [ic.partner(links, CLENS, 0, *x) for x in [(0, 1_000, 1_256), (0, 1_000, 1_010), (0, 1_000, 1_256), (2, 2_000, 2_049), (0, 1_100, 1_101)] * 3]
    finally:
        dev.close()


def test_partner_table_at_its_smallest_foreign_keys_wrap_around_overflow_and_reset():
    """64 slots: links of another contig, another kind and another bucket on the probe run of the bucket asked for, a run that starts on
    the table's last slots and goes on at its first; then more links than the table keeps"""
    homes = {}
    for tid in (0, 1):
        for bucket in range(0, 150_000 // 256):
            for kind in range(4):
                homes.setdefault(ic.home_slot(tid, bucket, kind, 6), []).append((tid, bucket, kind))
    run = homes[62]
    mine = next(k for k in run if k[0] == 0)
    other_tid = next(k for k in run + homes[63] if k[0] == 1)
    other_kind = next(k for k in run + homes[63] + homes[0] if k[0] == 0 and k[2] != mine[2] and k != mine)
    other_bucket = next(k for k in run + homes[63] if k[0] == 0 and k[1] != mine[1] and k not in (mine, other_kind))
    at = lambda key, i: (key[0], key[2], 256 * key[1] + i, 1 - key[0], 3_000 + i)
    links = []
    for i in range(5):
        links += [at(mine, i), at(other_tid, i), at(other_kind, i), at(other_bucket, i)]
    rng = np.random.default_rng(2)
    dev = Device(log2_slots=6)
    try:
        dev.add(links)
        check(dev, links, rng)
        for key in (mine, other_tid, other_kind, other_bucket):
            assert dev.partner(key[0], [(key[2], 256 * key[1], 256 * key[1] + 255)]) == [(5, 1 - key[0], 5, 3_000, 3_004)], key
        more = [(0, 1, 2_000 + 300 * i, 1, 9_000) for i in range(12)]
        dev.add(more)
        check(dev, links + more, rng, n_random=10)
        assert dev.ctx.matelink_stats() == (32, 0)
        dev.add([(1, 2, 100 + i, 0, 200 + i) for i in range(5)])
        assert dev.ctx.matelink_stats() == (32, 5)
        assert dev.partner(0, [(mine[2], 0, 65_535), (1, 2_000, 2_000), (0, -9, -1)]) == [(NONE, -1, NONE, -1, -1)] * 3
        assert dev.partner(1, [(2, 0, 5_000)]) == [(NONE, -1, NONE, -1, -1)] and dev.partner(2, [(0, 0, 70)]) == [(NONE, -1, NONE, -1, -1)]
        dev.ctx.matelink_reset()
        assert dev.ctx.matelink_stats() == (0, 0) and dev.partner(0, [(mine[2], 0, 65_535)]) == [(0, -1, 0, 0, 0)]
        dev.add(links)
        check(dev, links, rng, n_random=10)
    finally:
        dev.close()


# ------------------------------------------------------------------------------------------ the junction verify

class TailDevice:
    """one context over the given contigs with the clip-tail table enabled, entries named by the test"""

    def __init__(self, refs, log2_slots=12):
        from indelminer_amd import capi
        self.ctx = capi.Context(0)
        self.ctx.set_reference(refs)
        self.ctx.cliptail_enable(20, 10, log2_slots)

    def add(self, table):
        for tid in sorted({k[0] for k in table}):
            rows = [(p, s, b) for (t, s, p), bs in table.items() if t == tid for b in bs]
            self.ctx.cliptail_add(tid, [r[0] for r in rows], [r[1] for r in rows], [len(r[2]) for r in rows], [ct.planes_of(r[2]) for r in rows])

    def junction(self, queries, S=32):
        out = self.ctx.cliptail_junction(*[[q[k] for q in queries] for k in range(6)], S)
        return [tuple(int(o[i]) for o in out) for i in range(len(queries))]


def _codes(ref, start, n, step=1, comp=False):
    out = tuple(b"ACGT".index(ref[start + step * i]) for i in range(n))
    return tuple(3 - c for c in out) if comp else out


def test_junction_four_cases_shifts_tolerance_ends_and_other_bytes():
    refs = contigs()
    refs[3] = refs[3][:2_000] + b"N" + refs[3][2_001:]
    A, B = refs[0], refs[1]
    table, queries = {}, []
    put = lambda tid, side, p, bases: table.setdefault((tid, side, p), []).append(bases)
    # the four cases x shifts {0, 5, 32}, every pair of positions its own; entries of 16, 31 and 32 bases at their tolerance and one beyond
    at = 1_000
    for s1, s2 in ((0, 1), (1, 0), (0, 0), (1, 1)):
        for s in (0, 5, 32):
            p1, p2 = at, 200_000 - at
            at += 500
            for n, bad in ((16, 0), (16, 1), (16, 2), (31, 1), (31, 2), (32, 2), (32, 3), (20, 0)):
                for (tid, side, p), (oref, op, oside) in (((0, s1, p1), (B, p2, s2)), ((1, s2, p2), (A, p1, s1))):
                    bases = list(_codes(oref, op + s if oside == 1 else op - 1 - s, n, 1 if oside == 1 else -1, comp=s1 == s2))
                    for k in range(bad):
                        bases[n - 1 - 3 * k] ^= 1
                    put(tid, side, p, tuple(bases))
            queries.append((0, p1, s1, 1, p2, s2))
            queries.append((1, p2, s2, 0, p1, s1))
    # positions that run off either contig's end: a pile 10 bases in front of contig 1's end and at contig 2's (70 bases) ends
    put(0, 0, 50_000, _codes(B, 299_990, 10) + (0,) * 10); put(1, 1, 299_990, _codes(A, 49_999, 20, -1))
    queries += [(0, 50_000, 0, 1, 299_990, 1), (0, 50_000, 0, 1, 299_999, 1), (0, 50_000, 0, 1, 300_000, 1), (0, 50_000, 0, 1, 300_001, 1), (0, 50_000, 0, 1, -1, 1)]
    put(2, 0, 70, _codes(A, 60_000, 20)); put(0, 1, 60_000, _codes(refs[2], 69, 20, -1)); put(2, 1, 0, _codes(A, 60_999, 20, -1))
    queries += [(2, 70, 0, 0, 60_000, 1), (0, 60_000, 1, 2, 70, 0), (2, 0, 1, 0, 61_000, 0), (2, 71, 0, 0, 60_000, 1), (0, 10, 1, 2, 5, 0)]
    put(0, 1, 10, _codes(refs[2], 4, 5, -1) + (1,) * 15)
    # a reference byte that is no base: contig 3 has an N at 2 000
    put(0, 0, 70_000, _codes(refs[3], 1_990, 10) + (0,) + _codes(refs[3], 2_001, 5)); put(0, 0, 70_100, _codes(refs[3], 1_990, 10) + (0,) + _codes(refs[3], 2_001, 4))
    queries += [(0, 70_000, 0, 3, 1_990, 1), (0, 70_100, 0, 3, 1_990, 1), (0, 70_000, 0, 3, 1_958, 1), (0, 70_100, 0, 3, 1_958, 1)]
    dev = TailDevice(refs)
    try:
        dev.add(table)
        for S in (32, 5, 4, 0):
            want = [ic.junction(table, refs, *q, S) for q in queries]
            assert dev.junction(queries, S) == want, (S, [(q, g, w) for q, g, w in zip(queries, dev.junction(queries, S), want) if g != w][:5])
        want = [ic.junction(table, refs, *q) for q in queries]
        # the planted figures: per case and shift 5 of 8 entries at either end are within the tolerance, at the planted shift
        assert want[:24] == [(5, 5, s, 8, 8) for _ in range(4) for s in (0, 0, 5, 5, 32, 32)]
        assert want[24:29] == [(0, 1, 0, 1, 1), (0, 0, -1, 1, 0), (0, 0, -1, 1, 0), (0, 0, -1, 1, 0), (0, 0, -1, 1, 0)]
        assert want[29:31] == [(1, 1, 0, 1, 1), (1, 1, 0, 1, 1)] and want[32][3:] == (0, 1)
        assert want[34:] == [(1, 0, 0, 1, 0), (0, 0, -1, 1, 0), (1, 0, 32, 1, 0), (0, 0, -1, 1, 0)]
        assert dev.junction([]) == []
    finally:
        dev.ctx.close()


def test_junction_on_one_contig_is_verify_crossed_and_inverted():
    """tid1 == tid2: im_cliptail_verify where pl > pr, and the v / s columns of im_clip_crossed_tid and im_clip_inverted_tid on their
    planted tables"""
    from indelminer_amd import capi, rawrec
    from tests.support import crossedpiles as cp, invertedpiles as ip
    for mod in (cp, ip):
        refs, rd = mod.planted_reads()
        raw, off = rawrec.records(rd)
        ctx = capi.Context(0)
        try:
            ctx.set_reference([r.tobytes() for r in refs])
            ctx.clip_enable(20, 10)
            ctx.cliptail_enable(20, 10, 14)
            d_raw = capi.DevBuf(ctx, len(raw) + 64).upload(raw)
            d_off = capi.DevBuf(ctx, 4 * len(off)).upload(off)
            recs = capi.DevRecords(len(off) - 1, d_raw.ptr, d_off.ptr, 0)
            ctx.clip_scatter(recs); ctx.cliptail_scatter(recs)
            ctx._check(capi.lib().im_stream_sync(ctx.h, ctx.stream))
            zeros = lambda n: np.zeros(n, np.int32)
            if mod is cp:
                pr, pl, _cr, _cl, vr, vl, s, nr, nl = ctx.clip_crossed_tid(0, 3, 30, 50, 100_000, 32, 1)
                assert len(pr) >= 9
                got = ctx.cliptail_junction(zeros(len(pr)), pr, zeros(len(pr)), zeros(len(pr)), pl, zeros(len(pr)) + 1)
                assert [list(map(int, g)) for g in got] == [list(map(int, w)) for w in (vr, vl, s, nr, nl)]
                # and verify itself, on the peaks in the order it accepts
                rp, lp = ctx.clip_peaks_tid(0, 0, 3, 30)[0][:40], ctx.clip_peaks_tid(0, 1, 3, 30)[0]
                a = np.repeat(rp, 3); b = np.concatenate([lp[np.searchsorted(lp, p + 1):][:3] for p in rp])
                a = a[:len(b)] if len(b) < len(a) else a
                b = b[:len(a)]
                keep = b > a
                a, b = a[keep], b[keep]
                want = ctx.cliptail_verify(0, a, b)
                got = ctx.cliptail_junction(zeros(len(a)), a, zeros(len(a)), zeros(len(a)), b, zeros(len(a)) + 1)
                assert len(a) >= 20 and [list(map(int, g)) for g in got] == [list(map(int, w)) for w in want]
            else:
                side, x, y, _c1, _c2, v1, v2, s, n1, n2 = ctx.clip_inverted_tid(0, 3, 30, 50, 1_000_000, 32, 1)
                assert len(x) >= 18
                got = ctx.cliptail_junction(zeros(len(x)), x, side, zeros(len(x)), y, side)
                assert [list(map(int, g)) for g in got] == [list(map(int, w)) for w in (v1, v2, s, n1, n2)]
            d_raw.free(); d_off.free()
        finally:
            ctx.close()


# ------------------------------------------------------------------------------------------ argument errors

def test_arguments_of_all_seven_entries():
    from indelminer_amd import capi
    lib, ptr = capi.lib(), lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    kind, a0, a1 = np.zeros(2, np.uint8), np.array([0, 10], np.int32), np.array([65_535, 20], np.int32)
    outs = lambda: [np.full(2, 77, np.uint32 if k in (0, 2) else np.int32) for k in range(5)]
    partner = lambda h, tid, nq, k, x, y, o: lib.im_matelink_partner(h, tid, nq, ptr(k), ptr(x), ptr(y), *[ptr(v) for v in o])
    tids, ps, sides = np.zeros(2, np.int32), np.array([5, 6], np.int32), np.zeros(2, np.uint8)
    jouts = lambda: [np.full(2, 77, np.int32 if k == 2 else np.uint32) for k in range(5)]
    junction = lambda h, nq, cols, S, o: lib.im_cliptail_junction(h, nq, *[ptr(c) for c in cols], S, *[ptr(v) for v in o])
    jcols = [tids, ps, sides, tids, ps, sides]
    recs = capi.DevRecords(0, None, None, 0)
    stored, dropped = C.c_uint64(0), C.c_uint64(0)
    ctx = capi.Context(0)
    try:
        # the reference is not set
        assert lib.im_matelink_enable(ctx.h, 10, 8) != 0 and lib.im_last_error(ctx.h) == b"im_set_reference has not been called"
        assert junction(ctx.h, 2, jcols, 32, jouts()) != 0
        ctx.set_reference(contigs())
        # every entry before the enable
        assert lib.im_dev_matelink_scatter(ctx.h, C.byref(recs), None) != 0 and lib.im_last_error(ctx.h) == b"im_matelink_enable has not been called"
        assert partner(ctx.h, 0, 2, kind, a0, a1, outs()) != 0 and lib.im_last_error(ctx.h) == b"im_matelink_enable has not been called"
        assert lib.im_matelink_add(ctx.h, 0, 0, None, None, None, None) != 0 and lib.im_matelink_reset(ctx.h, None) != 0
        assert lib.im_matelink_stats(ctx.h, C.byref(stored), C.byref(dropped)) != 0
        assert junction(ctx.h, 2, jcols, 32, jouts()) != 0 and lib.im_last_error(ctx.h) == b"im_cliptail_enable has not been called"
        for k in (5, 31, -1):
            assert lib.im_matelink_enable(ctx.h, 10, k) != 0 and b"log2_slots" in lib.im_last_error(ctx.h)
        assert lib.im_matelink_enable(None, 10, 8) != 0
        ctx.matelink_enable(10, 8)
        ctx.matelink_enable(10, 8)                                  # the same values again: fine
        assert lib.im_matelink_enable(ctx.h, 11, 8) != 0 and b"already enabled with min_mapq 10, log2_slots 8" in lib.im_last_error(ctx.h)
        assert lib.im_matelink_enable(ctx.h, 10, 9) != 0
        # partner
        o = outs()
        assert partner(ctx.h, 0, 2, kind, a0, a1, o) == 0 and [list(v) for v in o] == [[0, 0], [-1, -1], [0, 0], [0, 0], [0, 0]]
        wide = a1.copy(); wide[0] = 65_536
        assert partner(ctx.h, 0, 2, kind, a0, wide, outs()) != 0 and b"query 0: a1 - a0 = 65536" in lib.im_last_error(ctx.h)
        bad = kind.copy(); bad[1] = 4
        assert partner(ctx.h, 0, 2, bad, a0, a1, outs()) != 0 and b"query 1: kind 4" in lib.im_last_error(ctx.h)
        bad[1] = 3
        assert partner(ctx.h, 0, 2, bad, a0, a1, outs()) == 0
        assert partner(ctx.h, 4, 2, kind, a0, a1, outs()) != 0 and partner(ctx.h, -1, 2, kind, a0, a1, outs()) != 0
        assert partner(ctx.h, 0, -1, kind, a0, a1, outs()) != 0 and partner(None, 0, 2, kind, a0, a1, outs()) != 0
        for k in range(8):
            args = [kind, a0, a1] + outs(); args[k] = None
            assert partner(ctx.h, 0, 2, *args[:3], args[3:]) != 0, k
        assert partner(ctx.h, 0, 0, None, None, None, [None] * 5) == 0
        # add: kind 4 is an error; what fails the rule's range checks is dropped without a ticket
        pos = np.array([5, 6], np.int32); one = np.ones(2, np.int32); bad[1] = 4
        assert lib.im_matelink_add(ctx.h, 0, 2, ptr(pos), ptr(one), ptr(pos), ptr(bad)) != 0 and b"link 1: kind 4" in lib.im_last_error(ctx.h)
        assert lib.im_matelink_add(ctx.h, 4, 2, ptr(pos), ptr(one), ptr(pos), ptr(kind)) != 0 and lib.im_matelink_add(ctx.h, -1, 2, ptr(pos), ptr(one), ptr(pos), ptr(kind)) != 0
        assert lib.im_matelink_add(ctx.h, 0, -1, ptr(pos), ptr(one), ptr(pos), ptr(kind)) != 0 and lib.im_matelink_add(None, 0, 2, ptr(pos), ptr(one), ptr(pos), ptr(kind)) != 0
        for k in range(4):
            args = [ptr(pos), ptr(one), ptr(pos), ptr(kind)]; args[k] = None
            assert lib.im_matelink_add(ctx.h, 0, 2, *args) != 0, k
        assert lib.im_matelink_add(ctx.h, 0, 0, None, None, None, None) == 0 and ctx.matelink_stats() == (0, 0)
        ctx.matelink_add(2, [0, -1, 5, 5, 71, 5, 5, 5, 70], [0, 0, 0, 0, 0, 2, 4, -1, 3], [150_000, 5, 150_001, -1, 5, 5, 5, 5, 5_000], [0] * 9)
        assert ctx.matelink_stats() == (2, 0) and [int(o[0]) for o in ctx.matelink_partner(2, [0], [0], [70])] == [2, 0, 1, 150_000, 150_000]
        # scatter, reset, stats
        assert lib.im_dev_matelink_scatter(ctx.h, None, None) != 0 and lib.im_dev_matelink_scatter(None, C.byref(recs), None) != 0
        neg = capi.DevRecords(-1, None, None, 0)
        assert lib.im_dev_matelink_scatter(ctx.h, C.byref(neg), None) != 0 and lib.im_last_error(ctx.h) == b"negative record count"
        assert lib.im_dev_matelink_scatter(ctx.h, C.byref(recs), None) == 0              # no record: no launch
        assert lib.im_matelink_reset(None, None) != 0 and lib.im_matelink_stats(None, C.byref(stored), C.byref(dropped)) != 0
        assert lib.im_matelink_stats(ctx.h, None, C.byref(dropped)) != 0 and lib.im_matelink_stats(ctx.h, C.byref(stored), None) != 0
        # the junction verify
        ctx.cliptail_enable(20, 10, 8)
        o = jouts()
        assert junction(ctx.h, 2, jcols, 32, o) == 0 and [list(v) for v in o] == [[0, 0], [0, 0], [-1, -1], [0, 0], [0, 0]]
        assert junction(ctx.h, 2, jcols, 33, jouts()) != 0 and b"max_shift 33" in lib.im_last_error(ctx.h)
        assert junction(ctx.h, 2, jcols, -1, jouts()) != 0
        two = sides.copy(); two[1] = 2
        assert junction(ctx.h, 2, jcols[:2] + [two] + jcols[3:], 32, jouts()) != 0 and b"query 1: sides 2 and 0" in lib.im_last_error(ctx.h)
        assert junction(ctx.h, 2, jcols[:5] + [two], 32, jouts()) != 0 and b"query 1: sides 0 and 2" in lib.im_last_error(ctx.h)
        for t in (4, -1):
            off = tids.copy(); off[0] = t
            assert junction(ctx.h, 2, [off] + jcols[1:], 32, jouts()) != 0 and b"query 0: contigs" in lib.im_last_error(ctx.h)
            assert junction(ctx.h, 2, jcols[:3] + [off] + jcols[4:], 32, jouts()) != 0
        assert junction(ctx.h, -1, jcols, 32, jouts()) != 0 and junction(None, 2, jcols, 32, jouts()) != 0
        for k in range(11):
            args = jcols + jouts(); args[k] = None
            assert junction(ctx.h, 2, args[:6], 32, args[6:]) != 0, k
        assert junction(ctx.h, 0, [None] * 6, 32, [None] * 5) == 0
        # after an overflow of the clip-tail table: no answer
        ctx.cliptail_add(0, list(range(100, 230)), [0] * 130, [20] * 130, [(0, 0)] * 130)
        assert ctx.cliptail_stats() == (128, 2)
        o = jouts()
        assert junction(ctx.h, 2, jcols, 32, o) == 0 and [list(v) for v in o] == [[NONE] * 2, [NONE] * 2, [-1, -1], [NONE] * 2, [NONE] * 2]
        # a new reference takes the table with it
        ctx.set_reference(contigs())
        assert lib.im_matelink_reset(ctx.h, None) != 0
        ctx.matelink_enable(11, 9)
    finally:
        ctx.close()


# ------------------------------------------------------------------------------------------ the product

def _run(binary, flags, cwd, env=None):
    e = dict(os.environ)
    e.update(env or {})
    return subprocess.run([binary] + flags + ["ref.fa", "sample=aln.bam"], cwd=cwd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=e, timeout=120)


def _ok(r):
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    assert b"overflowed" not in r.stderr
    return r


BASE = ["-i", "cfg.txt", "-s", "100"]


@pytest.fixture(scope="module")
def planted(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("intercontig"))
    refs, rd = ic.planted_reads()
    ic.write_planted(d, refs, rd)
    text, records = ic.render_of_bam(d + "/aln.bam", d + "/ref.fa", 10)
    return d, text, records


def test_product_file_in_the_pipelined_path_and_record_at_a_time(planted, tmp_path):
    """the planted junctions: FILE byte for byte the restatement's, in the pipelined path, with three walkers on small pieces, and in the
    record-at-a-time path at 1 000 records per chunk, which cuts inside the planted bundles"""
    d, text, records = planted
    assert len(records) == 9 and text.count(b";PE=3,3\n") == 9
    prod = _product()
    path = lambda name: str(tmp_path / name)
    read = lambda name: open(path(name), "rb").read()
    _ok(_run(prod, BASE + ["-G", "-C", "-V", "-T", path("t0")], d))
    assert read("t0") == text
    envs = ({"INDELMINER_PIPELINE": "host", "INDELMINER_HOST_CHUNK_RECS": "1000"}, {"INDELMINER_PIECE_BYTES": "60000", "INDELMINER_WALKERS": "3"})
    for k, env in enumerate(envs, 1):
        _ok(_run(prod, BASE + ["-G", "-C", "-V", "-T", path("t%d" % k)], d, env=env))
        assert read("t%d" % k) == text, env


def test_product_everything_else_is_unchanged_by_the_option(planted, tmp_path):
    d, text, _ = planted
    prod = _product()
    path = lambda name: str(tmp_path / name)
    read = lambda name: open(path(name), "rb").read()
    r0 = _ok(_run(prod, BASE + ["-G", "-C", "-V", "-I", path("i0"), "-U", path("u0"), "-N", path("n0"), "-M"], d))
    r1 = _ok(_run(prod, BASE + ["-G", "-C", "-V", "-I", path("i1"), "-U", path("u1"), "-N", path("n1"), "-M", "-T", path("t1")], d))
    assert r1.stdout == r0.stdout and r1.stderr == r0.stderr and len(r0.stdout) > 1000
    assert read("i1") == read("i0") and read("u1") == read("u0") and read("n1") == read("n0") and read("t1") == text


def test_product_detailed_output_ignores_the_option_and_it_is_refused_without_v(planted, tmp_path):
    d = planted[0]
    prod = _product()
    fo = str(tmp_path / "none.vcf")
    d0 = _ok(_run(prod, BASE + ["-o", "detailed"], d))
    d1 = _ok(_run(prod, BASE + ["-o", "detailed", "-G", "-C", "-V", "-T", fo], d))
    assert d1.stdout == d0.stdout and d1.stderr == d0.stderr and len(d0.stdout) > 0 and not os.path.exists(fo)
    r = _run(prod, BASE + ["-G", "-C", "-T", fo], d)
    assert r.returncode != 0 and r.stdout == b"" and r.stderr == b"indelminer: -T needs -V\n" and not os.path.exists(fo)


def test_product_after_an_overflow_of_the_mate_link_table(tmp_path):
    """2 100 pairs turned inter-contig against the 2 048 links the table of a small BAM keeps: the FILE has its header and no records,
    and stderr says so once, at the end"""
    refs, rd = ic.planted_overflow_reads()
    d = ic.write_planted(str(tmp_path), refs, rd)
    _, _, links = ic.links_of_bam(d + "/aln.bam", 10)
    assert len(links) > 4_200 and os.path.getsize(d + "/aln.bam") < 64 << 16
    prod = _product()
    f1 = str(tmp_path / "t1")
    r0 = _ok(_run(prod, BASE + ["-G", "-C", "-V"], d))
    r1 = _run(prod, BASE + ["-G", "-C", "-V", "-T", f1], d)
    assert r1.returncode == 0 and open(f1, "rb").read() == ic.render(None, None, [])
    line = b"indelminer: -T: the mate-link table overflowed (2048 links stored, %d dropped): its file has no records\n" % (len(links) - 2_048)
    assert r1.stdout == r0.stdout and r1.stderr == r0.stderr + line
