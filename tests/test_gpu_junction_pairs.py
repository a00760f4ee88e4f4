"""Junction pairs (-E): the stretched form of the pair links' scatter and junction_pairs_kernel of im_links.hip behind
im_pairlink_stretched_enable and im_junction_pairs, and what the host driver makes of them (PE= in -J's FILE).

The yardstick is the plain restatement in tests/support/junctionpairs.py, written from the rule in include/indelminer_amd.h (seam 5,
"Junction pairs"), not from the code under test; tests/test_junction_pairs_host.py pins it to cases worked by hand.  Every answer is
compared exactly.
"""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from tests.support import intercontig as ic
from tests.support import junctionpairs as jp
from tests.support import pairlinks as pk
from tests.support import splitjunctions as sj
from tests.support import splitlinks as sl
from tests.support.spanarrays import _product

pytestmark = pytest.mark.gpu

IM_OK, IM_E_ARG = 0, -1                          # include/indelminer_amd.h
Q = 10
ONES = jp.NONE
PLAIN = jp.Rec(0, 100, 60, 0x1 | 0x2 | 0x20 | 0x40, 0, 400)     # a proper pair's leftmost record: no link of either family


def contigs(clens, seed=3):
    rng = np.random.default_rng(seed)
    return [bytes(rng.choice(np.frombuffer(b"ACGT", np.uint8), n)) for n in clens]


class Device:
    """one context over contigs of these lengths with both pair tables enabled, the pair links' in the stretched form unless told otherwise"""

    def __init__(self, clens, log2_slots=12, stretched=True, pair=True, mate=True, mate_log2=None):
        from indelminer_amd import capi
        self.capi, self.clens = capi, list(clens)
        self.ctx = capi.Context(0)
        self.ctx.set_reference(contigs(clens))
        if pair:
            self.ctx.pairlink_enable(Q, log2_slots)
        if pair and stretched:
            self.ctx.pairlink_stretched_enable()
        if mate:
            self.ctx.matelink_enable(Q, mate_log2 or log2_slots)
        self.keep = []

    def scatter_raw(self, raw, off):
        capi = self.capi
        d_raw = capi.DevBuf(self.ctx, len(raw) + 64).upload(raw)
        d_off = capi.DevBuf(self.ctx, 4 * len(off)).upload(off)
        self.keep += [d_raw, d_off]
        recs = capi.DevRecords(len(off) - 1, d_raw.ptr, d_off.ptr, 0)
        self.ctx.pairlink_scatter(recs)
        self.ctx.matelink_scatter(recs)
        self.ctx._check(capi.lib().im_stream_sync(self.ctx.h, self.ctx.stream))

    def scatter(self, recs, qual=True, chunk=None):
        chunk = chunk or len(recs)
        for k in range(0, len(recs), chunk):
            self.scatter_raw(*pk.pack_records(recs[k:k + chunk], qual))

    def add(self, pairs=(), mates=()):
        for tid in range(len(self.clens)):
            mine = [x for x in pairs if x[0] == tid]
            if mine:
                self.ctx.pairlink_add(tid, [l[2] for l in mine], [l[3] for l in mine], [l[1] for l in mine])
            mine = [x for x in mates if x[0] == tid]
            if mine:
                self.ctx.matelink_add(tid, [l[2] for l in mine], [l[3] for l in mine], [l[4] for l in mine], [l[1] for l in mine])

    def reset(self):
        self.ctx.pairlink_reset(self.ctx.stream)
        self.ctx.matelink_reset(self.ctx.stream)

    def stats(self):
        return self.ctx.pairlink_stats(), self.ctx.matelink_stats()

    def pairs(self, junctions, reach=jp.REACH, back=jp.BACK, min_sep=jp.MIN_SEP):
        pe1, pe2 = self.ctx.junction_pairs(*[[j[k] for j in junctions] for k in range(6)], reach, back, min_sep)
        return [(int(a), int(b)) for a, b in zip(pe1, pe2)]

    def raw(self, n, junctions, reach=jp.REACH, back=jp.BACK, min_sep=jp.MIN_SEP, null=None):
        """the entry itself: (return code, the two columns as given back) over columns of sentinels; null: a column left out"""
        kinds = (np.int32, np.int32, np.uint8, np.int32, np.int32, np.uint8)
        cols = [np.ascontiguousarray([j[k] for j in junctions] or [0], dtype=t) for k, t in enumerate(kinds)]
        outs = [np.full(max(len(junctions), 1), 77, np.uint32) for _ in range(2)]
        ptrs = [None if k == null else a.ctypes.data_as(C.c_void_p) for k, a in enumerate(cols + outs)]
        rc = self.capi.lib().im_junction_pairs(self.ctx.h, n, *ptrs[:6], reach, back, min_sep, *ptrs[6:])
        return rc, outs

    def err(self):
        return self.capi.lib().im_last_error(self.ctx.h).decode()

    def close(self):
        for b in self.keep:
            b.free()
        self.ctx.close()


def links_of(recs, clens, stretched=True):
    return jp.pair_links_of(recs, clens, Q, stretched), ic.links_of(recs, clens, Q)


def check(dev, pairs, mates, junctions, **kw):
    """the device's answers are the restatement's, and no table has dropped a link: a '.' cannot hide a wrong count"""
    assert dev.stats() == ((len(pairs), 0), (len(mates), 0))
    want = jp.answers(pairs, mates, dev.clens, junctions, **kw)
    got = dev.pairs(junctions, **kw)
    assert got == want, [(j, g, w) for j, g, w in zip(junctions, got, want) if g != w][:6]
    return want


HAND_JUNCTIONS = [j for _, _, j, _ in jp.HAND]


@pytest.fixture(scope="module")
def hand_device():
    dev = Device(jp.HAND_CLENS)
    yield dev
    dev.close()


# ------------------------------------------------------------------------------------------ 1. the scatter

@pytest.mark.parametrize("chunk", [1, 63, 64, 65, 1_024, 1_025])
def test_scatter_the_hand_records_in_chunks(hand_device, chunk):
    """every record of the hand cases side by side among proper pairs, packed directly, in either record form, cut into chunks of one
    size: both tables hold the restatement's links and every hand junction answers what the restatement answers over all of them"""
    dev = hand_device
    hand, _ = jp.hand_records()
    recs = []
    for r in hand:
        recs += [r, PLAIN, PLAIN]
    recs = (recs * 8)[:400 if chunk == 1 else 2 * 1_025 + 7]
    pairs, mates = links_of(recs, jp.HAND_CLENS)
    assert len(recs) in (400, 2_057) and {l[1] for l in pairs} == {0, 1, 2, 3} and len(mates) > 20
    for qual in (True, False):
        dev.reset()
        dev.scatter(recs, qual, chunk)
        want = check(dev, pairs, mates, HAND_JUNCTIONS)
        assert sum(1 for w in want if w != (0, 0)) >= 20
        check(dev, pairs, mates, HAND_JUNCTIONS, min_sep=0)


def test_scatter_through_a_bam_file_in_both_record_forms(hand_device, tmp_path):
    from indelminer_amd import rawrec
    dev = hand_device
    _, recs = jp.hand_records()
    path = str(tmp_path / "hand.bam")
    jp.write_recs_bam(path, recs, jp.HAND_CLENS)
    raw, off, found = rawrec.records_from_bam(path)
    assert [n for _, n in found] == jp.HAND_CLENS and len(off) - 1 == len(recs) > 100
    pairs, mates = links_of(recs, jp.HAND_CLENS)
    assert sum(1 for l in pairs if l[1] == 3) >= 20
    for form in ((raw, off), rawrec.strip_quals(raw, off)):
        dev.reset()
        dev.scatter_raw(*form)
        check(dev, pairs, mates, HAND_JUNCTIONS)


def test_the_stretched_form_against_the_plain_form():
    """the same chunk through both forms: the same links of kinds 0 .. 2 and the same counts of them; the plain form stores no kind 3
    and goes on refusing it"""
    from tests.test_gpu_pairlink import CLENS, random_records, rule_edges
    rng = np.random.default_rng(17)
    recs = rule_edges() + random_records(rng, 3_000) + [r for r in jp.hand_records()[0] if r.tid < 2 and r.pos <= 5_000]
    stretched, plain = jp.pair_links_of(recs, CLENS, Q), pk.links_of(recs, CLENS, Q)
    assert [l for l in stretched if l[1] < 3] == plain and len(stretched) - len(plain) >= 30 and len(plain) >= 300
    queries = {tid: [(k, p - 40, p + 40, m - 300, m + 300) for t, k, p, m in plain[::5] if t == tid] + [(k, -5, 65_530, -5, 200_000) for k in range(3)] for tid in range(3)}
    answers = []
    for form in (True, False):
        dev = Device(CLENS, stretched=form, mate=False)
        try:
            raw, off = pk.pack_records(recs)
            d_raw = dev.capi.DevBuf(dev.ctx, len(raw) + 64).upload(raw); d_off = dev.capi.DevBuf(dev.ctx, 4 * len(off)).upload(off)
            dev.keep += [d_raw, d_off]
            dev.ctx.pairlink_scatter(dev.capi.DevRecords(len(off) - 1, d_raw.ptr, d_off.ptr, 0))
            assert dev.ctx.pairlink_stats() == (len(stretched if form else plain), 0)
            answers.append({tid: [int(x) for x in dev.ctx.pairlink_count(tid, *[[q[k] for q in qs] for k in range(5)], 50)] for tid, qs in queries.items()})
            if form:
                got = int(dev.ctx.pairlink_count(0, [3], [-5], [65_530], [-5], [200_000], 0)[0])
                assert got == pk.count([(t, k - 3, p, m) for t, k, p, m in stretched if k == 3], CLENS, 0, 0, -5, 65_530, -5, 200_000, 0) > 0
                dev.ctx.pairlink_add(0, [5], [900], [3])
            else:
                with pytest.raises(dev.capi.IMError, match=r"im_pairlink_count: query 0: kind 3, must be 0 \(everted\), 1 \(forward\) or 2 \(reverse\)"):
                    dev.ctx.pairlink_count(0, [3], [0], [10], [0], [10], 0)
                with pytest.raises(dev.capi.IMError, match=r"im_pairlink_add: link 0: kind 3, must be 0 \(everted\), 1 \(forward\) or 2 \(reverse\)"):
                    dev.ctx.pairlink_add(0, [5], [900], [3])
                dev.ctx.matelink_enable(Q, 8)
                with pytest.raises(dev.capi.IMError, match="im_pairlink_stretched_enable has not been called"):
                    dev.pairs([(0, 5, 0, 0, 900, 1)])
        finally:
            dev.close()
    assert answers[0] == answers[1] == {tid: [pk.count(plain, CLENS, tid, *q, 50) for q in qs] for tid, qs in queries.items()}
    assert sum(answers[0][0]) > 100


def test_the_switch_on_a_table_that_holds_links_twice_and_across_a_reset():
    clens = [10_000, 5_000]
    dev = Device(clens, log2_slots=6, stretched=False)
    try:
        stretched = jp.Rec(0, 4_500, 60, 0x1 | 0x20 | 0x40, 0, 5_900)
        J = (0, 5_000, 0, 0, 5_400, 1)
        dev.scatter([stretched])
        assert dev.ctx.pairlink_stats() == (0, 0)                                           # off: the record stores nothing
        dev.ctx.pairlink_add(0, [100], [600], [0])
        with pytest.raises(dev.capi.IMError, match="im_pairlink_stretched_enable: 1 links have been asked for already"):
            dev.ctx.pairlink_stretched_enable()
        dev.ctx.pairlink_reset(dev.ctx.stream)
        dev.ctx.pairlink_stretched_enable()                                                 # behind a reset the table is empty again
        dev.scatter([stretched])
        assert dev.ctx.pairlink_stats() == (1, 0) and dev.pairs([J]) == [(1, 0)]
        dev.ctx.pairlink_stretched_enable()                                                 # a second call is fine, whatever the table holds
        dev.ctx.pairlink_reset(dev.ctx.stream)                                              # the reset keeps the switch
        dev.scatter([stretched, stretched])
        assert dev.ctx.pairlink_stats() == (2, 0) and dev.pairs([J]) == [(2, 0)]
        # after an overflow of the table the switch stays what it is, and a dropped link counts as asked for
        dev.ctx.pairlink_add(0, [100] * 40, [600] * 40, [3] * 40)
        assert dev.ctx.pairlink_stats() == (32, 10)
        dev.ctx.pairlink_stretched_enable()
        # a new reference drops the switch with the table
        dev.ctx.set_reference(contigs(clens, seed=4))
        with pytest.raises(dev.capi.IMError, match="im_pairlink_enable has not been called"):
            dev.ctx.pairlink_stretched_enable()
        dev.ctx.pairlink_enable(Q, 6)
        with pytest.raises(dev.capi.IMError, match="kind 3"):
            dev.ctx.pairlink_add(0, [5], [900], [3])
        assert dev.capi.lib().im_pairlink_stretched_enable(None) == IM_E_ARG
    finally:
        dev.close()


# ------------------------------------------------------------------------------------------ 2. the query

@pytest.mark.parametrize("case", jp.HAND, ids=[c[0] for c in jp.HAND])
def test_query_every_case_worked_by_hand_in_three_arrival_orders(hand_device, case):
    dev = hand_device
    name, recs, junction, want = case
    orders = (recs, recs[::-1], [recs[i] for i in np.random.default_rng(len(recs)).permutation(len(recs))])
    for order in orders:
        dev.reset()
        dev.scatter(order)
        assert dev.pairs([junction]) == [want], name
        assert dev.stats()[0][1] == 0 and dev.stats()[1][1] == 0
        if name in jp.HAND_NO_SEP:
            assert dev.pairs([junction], min_sep=0) == [jp.HAND_NO_SEP[name]]


def test_kinds_0_to_2_are_the_count_query_on_the_same_windows():
    """on one contig, for the three kinds there were, the answer is im_pairlink_count's for the windows of the two ends, to the letter"""
    clens = [150_000, 5_000]
    rng = np.random.default_rng(23)
    sites = [(int(rng.integers(0, 2)), int(rng.integers(0, clens[t] + 1)), int(rng.integers(0, clens[t] + 1))) for t in rng.integers(0, 2, 60)]
    sites = [(t, min(a, b), max(a, b)) for t, a, b in sites]
    pairs = []
    for t, a, b in sites:
        for _ in range(20):
            p, m = a + int(rng.integers(-1_100, 1_101)), b + int(rng.integers(-1_100, 1_101))
            if 0 <= p <= m <= clens[t]:
                pairs.append((t, int(rng.integers(0, 4)), p, m))
    dev = Device(clens, log2_slots=12, mate=True)
    try:
        dev.add(pairs)
        for reach, back, sep in ((1_000, 32, 50), (0, 0, 0), (65_535, 0, 0), (300, 700, 1)):
            total = 0
            for t in (0, 1):
                junctions, queries = [], []
                for tt, a, b in sites:
                    for s_lo, s_hi in ((1, 0), (0, 0), (1, 1)):
                        if tt == t:
                            junctions.append((t, a, s_lo, t, b, s_hi) if rng.random() < 0.5 or a == b else (t, b, s_hi, t, a, s_lo))
                            wa = (a - back, a + reach) if s_lo else (a - reach, a + back)
                            wb = (b - back, b + reach) if s_hi else (b - reach, b + back)
                            queries.append((jp.KIND[(s_lo, s_hi)],) + wa + wb)
                want = [int(x) for x in dev.ctx.pairlink_count(t, *[[q[k] for q in queries] for k in range(5)], sep)]
                got = dev.pairs(junctions, reach, back, sep)
                assert got == [(w, 0) for w in want] == jp.answers(pairs, [], clens, junctions, reach, back, sep)
                total += sum(want)
            assert (reach, back) == (0, 0) or total > 20
    finally:
        dev.close()


@pytest.mark.parametrize("n", [1, 63, 64, 65, 200])
def test_one_key_held_by_many_links(n):
    clens = [100_000, 50_000]
    dev = Device(clens, log2_slots=10)
    try:
        pairs = [(0, 3, 30_000 + (i % 5), 30_500 + i) for i in range(n)] + [(0, 0, 30_001, 30_600), (0, 3, 30_300, 30_600)]
        mates = [(0, 2, 30_000 + (i % 5), 1, 20_000 + i) for i in range(n)] + [(1, 1, 20_000 + i, 0, 30_000 + (i % 5)) for i in range(0, n, 2)] + [(0, 2, 30_001, 1, 5)]
        dev.add(pairs, mates)
        want = check(dev, pairs, mates, [(0, 30_010, 0, 0, 30_490, 1), (0, 30_010, 0, 1, 19_990, 1), (1, 19_990, 1, 0, 30_010, 0)], reach=255, back=255)
        assert want == [(n, 0), (n, (n + 1) // 2), ((n + 1) // 2, n)]
    finally:
        dev.close()


def test_a_64_slot_table_whose_probe_runs_wrap():
    clens = [200_000, 70_000]
    dev = Device(clens, log2_slots=6)
    try:
        b = next(b for b in range(3, 700) if sl.home_slot(0, b, 3, 6) >= 60)
        b2 = next(x for x in range(3, 270) if sl.home_slot(1, x, 1, 6) >= 60)
        pairs = [(0, 3, 256 * b + 3 * i, 256 * b + 900 + i) for i in range(20)] + [(0, 1, 256 * b + 7, 256 * b + 900)] * 5
        mates = [(0, 2, 256 * b + 3 * i, 1, 256 * b2 + i) for i in range(20)] + [(1, 1, 256 * b2 + i, 0, 256 * b + 3 * i) for i in range(10)]
        dev.add(pairs, mates)
        junctions = [(0, 256 * b + 100, 0, 0, 256 * b + 880, 1), (0, 256 * b + 100, 0, 1, 256 * b2 - 10, 1), (0, 256 * b + 100, 0, 0, 256 * b + 880, 0)]
        assert check(dev, pairs, mates, junctions) == [(20, 0), (20, 10), (5, 0)]
        dev.reset()
        dev.add(pairs[::-1], mates[::-1])                                                   # other slots, the same answers
        check(dev, pairs, mates, junctions)
        check(dev, pairs, mates, junctions, reach=30, back=0, min_sep=0)
    finally:
        dev.close()


@pytest.mark.parametrize("n", [0, 1, 64, 65, 300])
def test_a_call_of_many_junctions_on_mixed_contigs(hand_device, n):
    dev = hand_device
    recs, _ = jp.hand_records()
    pairs, mates = links_of(recs, jp.HAND_CLENS)
    dev.reset()
    dev.scatter(recs)
    rng = np.random.default_rng(n)
    junctions = [HAND_JUNCTIONS[int(i)] for i in rng.integers(0, len(HAND_JUNCTIONS), n)]
    junctions = [j if rng.random() < 0.7 else j[3:6] + j[0:3] for j in junctions]
    want = check(dev, pairs, mates, junctions)
    assert n < 64 or (any(j[0] == j[3] for j in junctions) and any(j[0] != j[3] for j in junctions) and sum(1 for w in want if w != (0, 0)) > n // 3)
    if n == 0:
        rc, outs = dev.raw(0, [], null=0)
        assert rc == IM_OK and all((o == 77).all() for o in outs)                          # no launch, no column looked at


def test_either_table_overflowed_alone():
    clens = [100_000, 50_000]
    one, two = (0, 5_000, 0, 0, 5_400, 1), (0, 5_000, 0, 1, 7_000, 1)
    pairs, mates = [(0, 3, 4_500, 5_900)] * 3, [(0, 2, 4_500, 1, 7_500)] * 2 + [(1, 1, 7_500, 0, 4_500)]
    for which in ("pair", "mate"):
        dev = Device(clens, log2_slots=6 if which == "pair" else 8, mate_log2=6 if which == "mate" else 8)
        try:
            dev.add(pairs, mates)
            assert dev.pairs([one, two, one]) == [(3, 0), (2, 1), (3, 0)]
            if which == "pair":
                dev.add([(0, 0, 90_000, 90_500)] * 30)
                assert dev.stats() == ((32, 1), (3, 0))
                assert dev.pairs([one, two, one, two]) == [(ONES, ONES), (2, 1), (ONES, ONES), (2, 1)]
            else:
                dev.add([], [(0, 0, 90_000, 1, 500)] * 30)
                assert dev.stats() == ((3, 0), (32, 1))
                assert dev.pairs([one, two, one, two]) == [(3, 0), (ONES, ONES), (3, 0), (ONES, ONES)]
            rc, outs = dev.raw(2, [one, two])
            assert rc == IM_OK
        finally:
            dev.close()


def test_every_argument_error():
    clens = [10_000, 5_000]
    dev = Device(clens, log2_slots=8)
    try:
        a, b = (0, 1_000, 0, 0, 1_500, 1), (0, 1_000, 0, 1, 500, 1)
        good = [a, b, a]
        for args, kw, what in (((3, [a, (2, 5, 0, 1, 5, 1), a]), {}, "junction 1: contigs 2 and 1"), ((3, [a, a, (0, 5, 0, -1, 5, 1)]), {}, "junction 2: contigs 0 and -1"),
                               ((3, [(0, 5, 2, 1, 5, 1), a, a]), {}, "junction 0: sides 2 and 1"), ((3, [a, (0, 5, 0, 1, 5, 3), a]), {}, "junction 1: sides 0 and 3"),
                               ((3, good), {"reach": -1}, "reach -1"), ((3, good), {"back": -1}, "back -1"), ((3, good), {"reach": 65_535, "back": 1}, "reach + back <= 65535"),
                               ((3, good), {"reach": 2**31 - 1, "back": 2**31 - 1}, "reach + back <= 65535"), ((3, good), {"min_sep": -1}, "min_sep -1"), ((-1, good), {}, "n -1")):
            rc, outs = dev.raw(*args, **kw)
            assert rc == IM_E_ARG and all((o == 77).all() for o in outs) and "im_junction_pairs" in dev.err() and what in dev.err(), (args, kw, dev.err())
        for k in range(8):
            rc, outs = dev.raw(3, good, null=k)
            assert rc == IM_E_ARG and all((o == 77).all() for o in outs) and "junction 0" in dev.err(), k
        assert dev.capi.lib().im_junction_pairs(None, 0, *[None] * 6, 0, 0, 0, None, None) == IM_E_ARG
        assert dev.raw(3, good, reach=65_535, back=0)[0] == IM_OK and dev.raw(3, good, reach=0, back=65_535)[0] == IM_OK and dev.raw(3, good, 0, 0, 0)[0] == IM_OK
    finally:
        dev.close()
    for kw, what in (({"pair": False}, "im_pairlink_enable has not been called"), ({"mate": False}, "im_matelink_enable has not been called"),
                     ({"stretched": False}, "im_pairlink_stretched_enable has not been called")):
        cold = Device(clens, log2_slots=8, **kw)
        try:
            rc, outs = cold.raw(1, [(0, 5, 0, 0, 900, 1)])
            assert rc == IM_E_ARG and what in cold.err() and all((o == 77).all() for o in outs)
            assert cold.raw(0, [])[0] == IM_E_ARG
        finally:
            cold.close()


def test_seeded_soak_against_the_restatement():
    """20 000 links on 300 hot ends over 3 contigs (the ends of tests/test_gpu_splitjunction.py's soak): a link between two hot ends
    becomes a read pair whose two starts lie around the ends' windows, in and out of them; every junction between two hot ends at the
    driver's windows, at the widest and at none"""
    from tests.test_gpu_splitjunction import soak_links
    rng = np.random.default_rng(2026)
    clens = [150_000, 90_000, 40_000]
    split = soak_links(rng, clens)
    pairs, mates = [], []
    for ta, pa, sa, tb, pb, sb in split:
        a = pa + int(rng.integers(-40, 1_100)) * (1 if sa else -1)
        b = pb + int(rng.integers(-40, 1_100)) * (1 if sb else -1)
        if not (0 <= a <= clens[ta] and 0 <= b <= clens[tb]):
            continue
        if ta != tb:
            mates += [(ta, sa | sb << 1, a, tb, b), (tb, sb | sa << 1, b, ta, a)][:2 if rng.random() < 0.8 else 1]
        elif a <= b:
            pairs.append((ta, jp.KIND[(sa, sb)], a, b))
        else:
            pairs.append((ta, jp.KIND[(sb, sa)], b, a))
    junctions = sorted({sj.can(l) for l in split})[::4] + sorted({sj.rev(sj.can(l)) for l in split})[::15]
    assert len(pairs) + len(mates) >= 20_000 and len(pairs) > 4_000 and {l[1] for l in pairs} == {0, 1, 2, 3} and len(junctions) >= 600
    dev = Device(clens, log2_slots=16)
    try:
        for k in range(0, len(pairs), 7_000):
            dev.add(pairs[k:k + 7_000])
        for k in range(0, len(mates), 7_000):
            dev.add([], mates[k:k + 7_000])
        assert dev.stats() == ((len(pairs), 0), (len(mates), 0))
        want = jp.answers_fast(pairs, mates, clens, junctions)
        assert max(w[0] for w in want) >= 20 and any(w[0] != w[1] and w[1] > 0 for w in want) and sum(1 for w in want if w[0] > 0) > 300
        assert dev.pairs(junctions) == want
        assert want[::50] == jp.answers(pairs, mates, clens, junctions[::50])               # the two restatements
        assert dev.pairs(junctions, 65_535, 0, 0) == jp.answers_fast(pairs, mates, clens, junctions, 65_535, 0, 0)
        assert dev.pairs(junctions, 0, 0, 0) == jp.answers_fast(pairs, mates, clens, junctions, 0, 0, 0)
    finally:
        dev.close()


# ------------------------------------------------------------------------------------------ 3. the product

def _run(binary, flags, cwd, env=None):
    e = dict(os.environ)
    e.update(env or {})
    return subprocess.run([binary] + flags + ["ref.fa", "sample=aln.bam"], cwd=cwd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=e, timeout=120)


def _ok(r):
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    assert b"overflowed" not in r.stderr                                                    # dropped == 0: no table of the run has overflowed
    return r


def _err(r):
    """stderr without the whole seconds of its time stamps, which differ between two runs that straddle a second"""
    return re.sub(rb" : \d+ sec\. elapsed\n", b"\n", r.stderr)


BASE = ["-i", "cfg.txt", "-s", "100"]
ENVS = ({"INDELMINER_PIPELINE": "host"}, {"INDELMINER_PIECE_BYTES": "60000", "INDELMINER_WALKERS": "3"})


def _planted(kind, d, overflow=False):
    if kind == "DEL":
        refs, rd = jp.planted_deletion()
        return jp.write_planted(d, refs, rd)
    mod, refs, rd = jp.planted(kind, overflow)
    return mod.write_planted(d, refs, rd)


@pytest.mark.parametrize("kind", ["DUP", "INV", "BND", "DEL"])
def test_product_file_on_the_planted_data_sets(kind, tmp_path):
    """the planted data sets of -U, -N and -T with their pairs and the tags a split aligner would have written, and the planted deletion:
    FILE byte for byte the restatement's, alone and behind the whole chain, on the pipelined path, on the record-at-a-time path and with
    three walkers; without -E the FILE of the existing restatements; stdout, stderr and the other FILEs what they are without -E"""
    from tests.support import splitoverlap as so
    d = _planted(kind, str(tmp_path))
    bam, fa = d + "/aln.bam", d + "/ref.fa"
    want, plain, kept, pes = jp.render_of_bam(bam, fa)
    want_all, plain_all = jp.render_of_bam(bam, fa, genotype=True, overlap=True)[:2]
    assert plain == sj.render_of_bam(bam, fa, Q)[0] and plain_all == so.render_of_bam(bam, fa, Q, genotype=True)[0]
    assert len(kept) >= (1 if kind == "DEL" else 7) and sum(1 for pe in pes if pe[0] >= 3) >= (1 if kind == "DEL" else 4), pes
    if kind == "DEL":
        assert pes == [(jp.DEL_PE, 0)]
    prod = _product()
    path = lambda name: str(tmp_path / name)
    read = lambda name: open(path(name), "rb").read()
    chain = lambda k: ["-G", "-C", "-V", "-U", path("u%d" % k), "-N", path("n%d" % k), "-T", path("t%d" % k), "-M", "-S", "-J", path("j%d" % k), "-K", "-H"]
    r0 = _ok(_run(prod, BASE + chain(0), d))
    r1 = _ok(_run(prod, BASE + chain(1) + ["-E"], d))
    assert read("j0") == plain_all and read("j1") == want_all
    assert r1.stdout == r0.stdout and _err(r1) == _err(r0) and (read("u1"), read("n1"), read("t1")) == (read("u0"), read("n0"), read("t0"))
    g0 = _ok(_run(prod, BASE + ["-G", "-J", path("j2")], d))
    g1 = _ok(_run(prod, BASE + ["-G", "-J", path("j3"), "-E"], d))
    assert read("j2") == plain and read("j3") == want and g1.stdout == g0.stdout and _err(g1) == _err(g0)
    for k, env in enumerate(ENVS, 4):
        r = _ok(_run(prod, BASE + ["-E", "-G", "-J", path("j%d" % k)], d, env=env))
        assert read("j%d" % k) == want and r.stdout == g0.stdout, env


@pytest.mark.parametrize("kind", ["DUP", "BND"])
def test_product_after_a_forced_overflow_of_one_table(kind, tmp_path):
    """2 100 more links than the 2 048 a table of a small BAM keeps, in the pair-link table (DUP: everted pairs) or in the mate-link table
    (BND): every record of that class is PE=. or PE=.,. and stderr says so once, at the end"""
    d = _planted(kind, str(tmp_path), overflow=True)
    bam, fa = d + "/aln.bam", d + "/ref.fa"
    over = dict(pair_over=True) if kind == "DUP" else dict(mate_over=True)
    want, plain, kept, pes = jp.render_of_bam(bam, fa, **over)
    _, _, pairs, mates = jp.links_of_bam(bam, Q)
    n = len(pairs) if kind == "DUP" else len(mates)
    assert n > 2_048 and os.path.getsize(bam) < 64 << 16 and len(kept) >= 7 and all(pe == (ONES, ONES) for pe in pes)
    prod = _product()
    f0, f1 = str(tmp_path / "j0"), str(tmp_path / "j1")
    r0 = _ok(_run(prod, BASE + ["-G", "-J", f0], d))
    r1 = _run(prod, BASE + ["-G", "-J", f1, "-E"], d)
    assert r1.returncode == 0 and open(f0, "rb").read() == plain and open(f1, "rb").read() == want
    assert want.count(b";PE=.\n" if kind == "DUP" else b";PE=.,.\n") == len(kept)
    words = (b"pair-link", b"PE is . on one contig in the file of -J") if kind == "DUP" else (b"mate-link", b"PE is .,. on two contigs in the file of -J")
    line = b"indelminer: -E: the %s table overflowed (2048 links stored, %d dropped): %s\n" % (words[0], n - 2_048, words[1])
    assert r1.stdout == r0.stdout and _err(r1) == _err(r0) + line


def test_product_detailed_output_ignores_the_option_and_it_is_refused_alone(tmp_path):
    d = _planted("DEL", str(tmp_path))
    prod = _product()
    fo = str(tmp_path / "none.vcf")
    d0 = _ok(_run(prod, BASE + ["-o", "detailed"], d))
    d1 = _ok(_run(prod, BASE + ["-o", "detailed", "-G", "-J", fo, "-E"], d))
    assert d1.stdout == d0.stdout and _err(d1) == _err(d0) and len(d0.stdout) > 0 and not os.path.exists(fo)
    r = _run(prod, BASE + ["-G", "-E"], d)
    assert r.returncode != 0 and r.stdout == b"" and r.stderr == b"indelminer: -E needs -J\n"
    r = _run(prod, BASE + ["-E", "-J", fo], d)
    assert r.returncode != 0 and r.stdout == b"" and r.stderr == b"indelminer: -J needs -G\n" and not os.path.exists(fo)
