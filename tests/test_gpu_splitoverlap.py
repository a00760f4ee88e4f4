"""Junction overlap (-H): the overlap forms of the split-link scatter and add kernels and splitlink_overlap_kernel of im_links.hip behind
im_splitlink_overlap_enable, im_splitlink_add_overlap and im_splitlink_overlap, and what the host driver makes of them (HOMLEN, INSLEN
and OA in -J's FILE).

The yardstick is the plain restatement in tests/support/splitoverlap.py, written from the rule in include/indelminer_amd.h (seam 5,
"Junction overlap"), not from the code under test; tests/test_splitoverlap_host.py pins it to cases worked by hand.  Every answer is
compared exactly.
"""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from tests.support import junctiongt as jg
from tests.support import splitjunctions as sj
from tests.support import splitlinks as sl
from tests.support import splitoverlap as so
from tests.support.spanarrays import _product

pytestmark = pytest.mark.gpu

IM_OK, IM_E_ARG = 0, -1                          # include/indelminer_amd.h
W = so.WINDOW
ONES = 0xFFFFFFFF


def contigs(clens, seed=3):
    rng = np.random.default_rng(seed)
    return [bytes(rng.choice(np.frombuffer(b"ACGT", np.uint8), n)) for n in clens]


class Device:
    """one context over contigs of these lengths with the split-link table enabled and, unless told otherwise, its overlap array"""

    def __init__(self, clens, log2_slots=13, names=None, overlap=True, enable=True):
        from indelminer_amd import capi
        self.capi, self.clens = capi, list(clens)
        self.ctx = capi.Context(0)
        self.ctx.set_reference(contigs(clens))
        if enable:
            self.ctx.splitlink_enable(sl.MIN_CLIP, sl.MIN_MAPQ, log2_slots, names or ["c%d" % t for t in range(len(clens))])
        if enable and overlap:
            self.ctx.splitlink_overlap_enable()
        self.keep = []

    def scatter(self, raw, off):
        capi = self.capi
        d_raw = capi.DevBuf(self.ctx, len(raw) + 64).upload(raw)
        d_off = capi.DevBuf(self.ctx, 4 * len(off)).upload(off)
        self.keep += [d_raw, d_off]
        self.ctx.splitlink_scatter(capi.DevRecords(len(off) - 1, d_raw.ptr, d_off.ptr, 0))
        self.ctx._check(capi.lib().im_stream_sync(self.ctx.h, self.ctx.stream))

    def add(self, pairs):
        """pairs with their d, None for unknown"""
        cols = [[l[k] for l, _ in pairs] for k in range(6)]
        self.ctx.splitlink_add_overlap(*cols, [so.UNKNOWN if d is None else d for _, d in pairs])

    def add_plain(self, links):
        self.ctx.splitlink_add(*[[x[k] for x in links] for k in range(6)])

    def reset(self):
        self.ctx.splitlink_reset(self.ctx.stream)

    def overlap(self, junctions, window=W):
        known, median, agree = self.ctx.splitlink_overlap(*[[j[k] for j in junctions] for k in range(6)], window)
        return [(int(a), int(b), int(c)) for a, b, c in zip(known, median, agree)]

    def junctions(self, window=W, min_links=sj.MIN_LINKS, min_span=sj.MIN_SPAN):
        out = self.ctx.splitlink_junctions(window, min_links, min_span, 65536)
        return None if out is None else [tuple(int(col[i]) for col in out) for i in range(len(out[0]))]

    def raw(self, n, junctions, window, null=None):
        """the entry itself: (return code, the three columns as given back) over columns of sentinels; null: a column left out"""
        kinds = (np.int32, np.int32, np.uint8, np.int32, np.int32, np.uint8)
        cols = [np.ascontiguousarray([j[k] for j in junctions] or [0], dtype=t) for k, t in enumerate(kinds)]
        outs = [np.full(max(len(junctions), 1), 77, t) for t in (np.uint32, np.int32, np.uint32)]
        ptrs = [None if k == null else a.ctypes.data_as(C.c_void_p) for k, a in enumerate(cols + outs)]
        rc = self.capi.lib().im_splitlink_overlap(self.ctx.h, n, *ptrs[:6], window, *ptrs[6:])
        return rc, outs

    def err(self):
        return self.capi.lib().im_last_error(self.ctx.h).decode()

    def close(self):
        for b in self.keep:
            b.free()
        self.ctx.close()


def check(dev, pairs, junctions, window=W):
    want = [so.junction_summary(pairs, dev.clens, j, window) for j in junctions]
    got = dev.overlap(junctions, window)
    assert got == want, [(j, g, w) for j, g, w in zip(junctions, got, want) if g != w][:6]
    return want


# ------------------------------------------------------------------------------------------ 1. the scatter

@pytest.fixture(scope="module")
def hand_device():
    dev = Device(so.CLENS, names=so.NAMES)
    yield dev
    dev.close()


@pytest.mark.parametrize("qual", [True, False], ids=["with qualities", "without"])
def test_scatter_every_case_worked_by_hand(hand_device, qual):
    """every case of tests/test_splitoverlap_host.py, alone in the table, in either delivered record form: the d its link carries is read
    back through the query on the junction of that one link, with no window"""
    dev = hand_device
    for name, kw, want in so.HAND:
        rec = sl.make_record(qual=qual, **kw)
        link = sl.link_of(rec, so.NAMES, so.CLENS, sl.MIN_CLIP, sl.MIN_MAPQ)
        dev.reset()
        dev.scatter(*sl.pack([rec]))
        assert dev.ctx.splitlink_stats() == (1, 0), name
        got = dev.overlap([link, sj.rev(link)], 0)
        assert got == [(0, 0, 0)] * 2 if want is None else got == [(1, want, 1)] * 2, (name, got, want)


def test_scatter_a_chunk_of_all_hand_cases_among_records_without_a_link(hand_device):
    """the cases side by side at their own positions, among the split links' own cases (most of which store nothing), on several waves
    of one workgroup and across two: every link's d at its slot"""
    dev = hand_device
    recs, pairs = [], []
    for k, (name, kw, want) in enumerate(so.HAND):
        recs.append(sl.make_record(pos=300 + 70 * k, **kw))
    for k in range(12):
        recs += [sl.make_record(**kw) for _, kw, _ in sl.CASES]
    assert len(recs) > 1_024
    order = np.random.default_rng(4).permutation(len(recs))
    recs = [recs[i] for i in order]
    pairs = so.overlaps_of(recs, so.NAMES, so.CLENS, sl.MIN_CLIP, sl.MIN_MAPQ)
    assert len(pairs) > 12 * 30 and sum(d is None for _, d in pairs) >= 5 and len({d for _, d in pairs}) >= 15
    dev.reset()
    dev.scatter(*sl.pack(recs))
    assert dev.ctx.splitlink_stats() == (len(pairs), 0)
    ends = sorted({l for l, _ in pairs})
    want = check(dev, pairs, ends, 0)
    assert sum(w[0] == 1 for w in want) >= 25 and max(w[0] for w in want) >= 12
    check(dev, pairs, ends, W)


# ------------------------------------------------------------------------------------------ 2. a table whose probe runs wrap

def test_a_64_slot_table_whose_probe_runs_wrap():
    clens = [200_000, 70_000, 9_000]
    dev = Device(clens, log2_slots=6)
    try:
        found = [(b, b2) for b in range(3, 200) for b2 in range(3, 200) if sl.home_slot(0, b, 2, 6) >= 60 and sl.home_slot(1, b2, 1, 6) >= 60][:1]
        assert found
        b, b2 = found[0]
        # 20 links of one key, whose run starts in the table's last four slots, each at its own position with its own d; 10 the other way
        pairs = [((0, 256 * b + 3 * i, 0, 1, 256 * b2 + 50, 1), 5 * i - 40) for i in range(20)]
        pairs += [(sj.rev(l), 100 + i) for i, (l, _) in enumerate(pairs[:10])]
        assert len(pairs) == 30
        dev.add(pairs)
        assert dev.ctx.splitlink_stats() == (30, 0)
        ends = [l for l, _ in pairs[:20]]
        want = check(dev, pairs, ends, 0)
        assert want[:10] == [(2, 5 * i - 40, 1) for i in range(10)] and want[10:] == [(1, 5 * i - 40, 1) for i in range(10, 20)]
        assert check(dev, pairs, ends[:1], 32) == [(11 + 10, 10, 1)]       # 11 positions within 32 bases (-40 .. 10), the ten reverses above them
        # the same links in another order claim other slots: the array follows
        dev.reset()
        dev.add(pairs[::-1])
        check(dev, pairs, ends, 0)
        check(dev, pairs, ends, 255)
    finally:
        dev.close()


# ------------------------------------------------------------------------------------------ 3. the batch edges of the walk

@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 200])
def test_one_tuple_held_by_many_links_with_distinct_d(n):
    clens = [100_000, 50_000]
    dev = Device(clens, log2_slots=10)
    try:
        a = (0, 30_000, 1, 1, 20_000, 0)
        ds = [int(x) for x in np.random.default_rng(n).permutation((np.arange(n) - n // 2) * 7)]
        pairs = [(a if i % 3 else sj.rev(a), d) for i, d in enumerate(ds)] + [((0, 30_010, 0, 1, 20_000, 0), 999), ((0, 29_000, 1, 1, 20_000, 0), 999)]
        dev.add(pairs)
        want = check(dev, pairs, [a, sj.rev(a)])
        assert want[0] == want[1] == (n, sorted(ds)[(n - 1) // 2], 1)
    finally:
        dev.close()


def test_a_deep_site_of_thousands_of_links_with_few_values():
    """3 000 links on one tuple: the median of a large multiset with repeats, and the count of its value"""
    clens = [100_000, 50_000]
    dev = Device(clens, log2_slots=13)
    try:
        a = (0, 30_000, 0, 1, 20_000, 1)
        rng = np.random.default_rng(12)
        ds = [int(x) for x in rng.choice([-12, -1, 0, 0, 3, 3, 3, 40, so.D_MAX, -so.D_MAX], 3_000)]
        pairs = [(a if rng.random() < 0.6 else sj.rev(a), d) for d in ds]
        dev.add(pairs)
        assert check(dev, pairs, [a]) == [so.summary(ds)] and so.summary(ds)[2] > 500
    finally:
        dev.close()


# ------------------------------------------------------------------------------------------ 4. pooling

def test_pooling_across_directions_windows_buckets_and_contig_ends():
    clens = [10_000, 5_000, 3_000]
    dev = Device(clens, log2_slots=10)
    try:
        a = (0, 1_000, 0, 1, 500, 1)
        edge = (0, 255, 0, 1, 256, 1)
        pairs = [(a, 4), (a, 4), (sj.rev(a), 6), (sj.rev(a), 6), (sj.rev(a), 9),                       # the two directions differ
                 ((0, 1_032, 0, 1, 532, 1), -2), ((0, 1_033, 0, 1, 500, 1), 77), ((0, 1_000, 0, 1, 533, 1), 77),   # W at both ends; W + 1 at either
                 ((0, 1_000, 1, 1, 500, 1), 77), ((0, 1_000, 0, 1, 500, 0), 77), ((0, 1_000, 0, 2, 500, 1), 77),   # another kind, another tidB
                 (edge, 1), ((0, 256, 0, 1, 255, 1), 2), (sj.rev(edge), 3), ((1, 255, 1, 0, 256, 0), 5),            # pA = 255 / 256: two buckets
                 ((0, 0, 1, 1, 5_000, 0), -7), ((0, 10, 1, 1, 4_990, 0), -8), ((1, 5_000, 0, 0, 0, 1), -9),        # position 0 and the contig's length
                 ((0, 10_000, 0, 2, 3_000, 0), 11), ((2, 2_990, 0, 0, 9_980, 0), 12)]
        dev.add(pairs)
        junctions = [a, sj.rev(a), edge, (0, 0, 1, 1, 5_000, 0), (0, 10_000, 0, 2, 3_000, 0), (0, 5, 1, 1, 4_999, 0), (2, 100, 0, 1, 100, 1)]
        want = check(dev, pairs, junctions)
        assert want == [(6, 4, 2), (6, 4, 2), (4, 2, 1), (3, -8, 1), (2, 11, 1), (3, -8, 1), (0, 0, 0)]
        assert check(dev, pairs, junctions, 0) == [(5, 6, 2), (5, 6, 2), (2, 1, 1), (2, -9, 1), (1, 11, 1), (0, 0, 0), (0, 0, 0)]
        check(dev, pairs, junctions, 255)
        check(dev, pairs, [(0, 1_016, 0, 1, 516, 1), (0, 968, 0, 1, 468, 1), (0, 967, 0, 1, 500, 1)], 32)
        # ends that lie outside their contig: windows that are empty after the clip count nothing, as im_splitlink_count has it
        assert dev.overlap([(0, 10_033, 0, 2, 3_000, 0), (0, 10_032, 0, 2, 3_032, 0), (0, -33, 1, 1, 5_000, 0), (0, 2**31 - 1, 0, 1, -2**31, 1)]) == [
            (0, 0, 0), (1, 11, 1), (0, 0, 0), (0, 0, 0)]
        # both ends on one contig and side, windows that overlap: a link both count queries count is taken once
        dev.reset()
        b, inside = (0, 2_000, 0, 0, 2_050, 0), (0, 2_030, 0, 0, 2_030, 0)
        pairs = [(b, 1), (sj.rev(b), 2), (inside, 3)]
        dev.add(pairs)
        assert dev.ctx.splitlink_count([0, 0], [0, 0], [1_968, 2_018], [2_032, 2_082], [0, 0], [0, 0], [2_018, 1_968], [2_082, 2_032]).tolist() == [2, 2]
        assert check(dev, pairs, [b, inside]) == [(3, 2, 1), (3, 2, 1)]
    finally:
        dev.close()


# ------------------------------------------------------------------------------------------ 5. links with and without a d

def test_a_mix_of_both_add_calls_and_unknown_values():
    clens = [10_000, 5_000]
    dev = Device(clens, log2_slots=10)
    try:
        a, b = (0, 1_000, 0, 1, 500, 1), (0, 3_000, 1, 1, 900, 0)
        dev.add([(a, 5), (a, None), (sj.rev(a), -3)])
        dev.add_plain([a, a, sj.rev(a), b, b])
        dev.add([(b, None), (sj.rev(b), None), (a, 5)])
        pairs = [(a, 5), (a, None), (sj.rev(a), -3), (a, None), (a, None), (sj.rev(a), None), (b, None), (b, None), (b, None), (sj.rev(b), None), (a, 5)]
        assert dev.ctx.splitlink_stats() == (len(pairs), 0)
        assert check(dev, pairs, [a, b]) == [(3, 5, 2), (0, 0, 0)]
        assert dev.ctx.splitlink_count([0, 0], [0, 1], [968, 2_968], [1_032, 3_032], [1, 1], [1, 0], [468, 868], [532, 932]).tolist() == [5, 3]
        # the raw column: -32768 is unknown, its neighbours are values
        dev.reset()
        dev.ctx.splitlink_add_overlap(*[[x] * 3 for x in a], np.array([-32768, -32767, 32767], np.int16))
        assert dev.overlap([a]) == [(2, -32767, 1)]
    finally:
        dev.close()


# ------------------------------------------------------------------------------------------ 6. the table is the same with the array and without

def test_the_same_records_give_the_same_table_with_the_array_and_without():
    recs = [sl.make_record(pos=300 + 70 * k, **kw) for k, (_, kw, _) in enumerate(so.HAND)]
    for k in range(40):
        recs += [sl.make_record(**kw) for _, kw, _ in sl.CASES]
    recs = [recs[i] for i in np.random.default_rng(6).permutation(len(recs))]
    links = sl.links_of(recs, so.NAMES, so.CLENS, sl.MIN_CLIP, sl.MIN_MAPQ)
    assert len(recs) > 3 * 1_024 and len(links) > 1_000
    raw, off = sl.pack(recs)
    answers = []
    for overlap, log2_slots in ((True, 13), (False, 13), (True, 10), (False, 10)):
        dev = Device(so.CLENS, names=so.NAMES, log2_slots=log2_slots, overlap=overlap)
        try:
            dev.scatter(raw, off)
            ends = sorted(set(links))
            counts = dev.ctx.splitlink_count(*[[l[k] for l in ends] for k in (0, 2, 1, 1, 3, 5, 4, 4)]).tolist()
            answers.append((dev.ctx.splitlink_stats(), dev.junctions(W, 1, 0), counts))
        finally:
            dev.close()
    assert answers[0] == answers[1] and answers[0][0] == (len(links), 0) and answers[0][1] == sj.junctions(links, so.CLENS, W, 1, 0)
    # and after an overflow: the links stored and dropped are the same numbers, and neither form answers
    assert answers[2] == answers[3] and answers[2][0] == (512, len(links) - 512) and answers[2][1] is None


# ------------------------------------------------------------------------------------------ 7. the error paths

def test_overflow_arguments_enable_order_and_reset():
    clens = [10_000, 5_000]
    dev = Device(clens, log2_slots=6)
    try:
        a = (0, 1_000, 0, 1, 500, 1)
        good = [a, sj.rev(a), (0, 0, 1, 1, 5_000, 0)]
        dev.add([(a, 3)] * 32)
        assert dev.ctx.splitlink_stats() == (32, 0) and dev.overlap(good) == [(32, 3, 32), (32, 3, 32), (0, 0, 0)]
        # every argument error; nothing is written
        for args, what in (((3, good, -1), "window -1"), ((3, good, 256), "window 256"), ((3, [a, (2, 5, 0, 1, 5, 1), a], W), "junction 1: contigs 2 and 1"),
                           ((3, [a, a, (0, 5, 0, -1, 5, 1)], W), "junction 2: contigs 0 and -1"), ((3, [(0, 5, 2, 1, 5, 1), a, a], W), "junction 0: sides 2 and 1"),
                           ((3, [a, (0, 5, 0, 1, 5, 3), a], W), "junction 1: sides 0 and 3")):
            rc, outs = dev.raw(*args)
            assert rc == IM_E_ARG and all((o == 77).all() for o in outs) and "im_splitlink_overlap" in dev.err() and what in dev.err(), (args, dev.err())
        for k in range(9):
            rc, outs = dev.raw(3, good, W, null=k)
            assert rc == IM_E_ARG and all((o == 77).all() for o in outs), k
        assert dev.raw(-1, good, W)[0] == IM_E_ARG
        assert dev.capi.lib().im_splitlink_overlap(None, 0, *[None] * 6, W, *[None] * 3) == IM_E_ARG
        rc, outs = dev.raw(0, [], W, null=0)
        assert rc == IM_OK and all((o == 77).all() for o in outs)                          # no launch, no column looked at
        assert dev.raw(3, good, 0)[0] == IM_OK and dev.raw(3, good, 255)[0] == IM_OK
        lib = dev.capi.lib()
        cols = [np.zeros(2, np.int32).ctypes.data_as(C.c_void_p)] * 7
        assert lib.im_splitlink_add_overlap(None, 0, *[None] * 7) == IM_E_ARG and lib.im_splitlink_add_overlap(dev.ctx.h, -1, *cols) == IM_E_ARG
        assert lib.im_splitlink_add_overlap(dev.ctx.h, 2, *cols[:6], None) == IM_E_ARG and lib.im_splitlink_add_overlap(dev.ctx.h, 0, *[None] * 7) == IM_OK
        with pytest.raises(dev.capi.IMError, match="im_splitlink_add_overlap: link 0: sides 2 and 0"):
            dev.ctx.splitlink_add_overlap([0], [5], [2], [1], [5], [0], [1])
        # a second enable is fine, whatever the table holds
        dev.ctx.splitlink_overlap_enable()
        # after an overflow all three columns are all ones, and the call is IM_OK
        dev.add([(a, 4)])
        assert dev.ctx.splitlink_stats() == (32, 1)
        rc, outs = dev.raw(3, good, W)
        assert rc == IM_OK and all((o.astype(np.int64) & ONES == ONES).all() for o in outs)
        assert dev.overlap(good) == [(ONES, -1, ONES)] * 3
        # reset clears the table and the array with it: the slots the 32 links held answer "unknown" to links without a d
        dev.reset()
        assert dev.overlap(good) == [(0, 0, 0)] * 3
        dev.add_plain([a] * 32)
        assert dev.ctx.splitlink_stats() == (32, 0) and dev.overlap(good) == [(0, 0, 0)] * 3
    finally:
        dev.close()
    # the order of the enable calls
    late = Device(clens, log2_slots=6, overlap=False)
    try:
        with pytest.raises(late.capi.IMError, match="im_splitlink_overlap_enable has not been called"):
            late.overlap([(0, 5, 0, 1, 5, 1)])
        with pytest.raises(late.capi.IMError, match="im_splitlink_overlap_enable has not been called"):
            late.add([((0, 5, 0, 1, 5, 1), 0)])
        late.add_plain([(0, 5, 0, 1, 5, 1)])
        with pytest.raises(late.capi.IMError, match="im_splitlink_overlap_enable: 1 links have been asked for already"):
            late.ctx.splitlink_overlap_enable()
        late.reset()
        late.ctx.splitlink_overlap_enable()                                                 # behind a reset the table is empty again
        late.add([((0, 5, 0, 1, 5, 1), -6)])
        assert late.overlap([(0, 5, 0, 1, 5, 1)]) == [(1, -6, 1)]
        # a new reference frees the array with the table
        late.ctx.set_reference(contigs(clens, seed=4))
        with pytest.raises(late.capi.IMError, match="im_splitlink_enable has not been called"):
            late.ctx.splitlink_overlap_enable()
        late.ctx.splitlink_enable(sl.MIN_CLIP, sl.MIN_MAPQ, 6, ["c0", "c1"])
        with pytest.raises(late.capi.IMError, match="im_splitlink_overlap_enable has not been called"):
            late.overlap([(0, 5, 0, 1, 5, 1)])
    finally:
        late.close()
    cold = Device(clens, enable=False)
    try:
        with pytest.raises(cold.capi.IMError, match="im_splitlink_enable has not been called"):
            cold.ctx.splitlink_overlap_enable()
        with pytest.raises(cold.capi.IMError, match="im_splitlink_enable has not been called"):
            cold.overlap([(0, 5, 0, 1, 5, 1)])
        assert cold.capi.lib().im_splitlink_overlap_enable(None) == IM_E_ARG
    finally:
        cold.close()


# ------------------------------------------------------------------------------------------ 8. the soak

def test_seeded_soak_against_the_restatement():
    """20 000 links on 300 hot ends over 3 contigs (the links of tests/test_gpu_splitjunction.py's soak) with a d each: one site in three
    agrees on a value, the others scatter, one link in twelve states none; every junction's summary at the driver's window and at the
    widest"""
    from tests.test_gpu_splitjunction import soak_links
    rng = np.random.default_rng(2025)
    clens = [150_000, 90_000, 40_000]
    links = soak_links(rng, clens)
    site_d = {}
    pairs = []
    for l in links:
        c = sj.can(l)
        base = site_d.setdefault((c[0], c[1] // 64, c[3], c[4] // 64), int(rng.integers(-60, 61)))
        r = rng.random()
        d = None if r < 1 / 12 else base if r < 0.7 or base % 3 == 0 else base + int(rng.integers(-3, 4))
        pairs.append((l, d))
    dev = Device(clens, log2_slots=16)
    try:
        for k in range(0, len(pairs), 7_000):
            dev.add(pairs[k:k + 7_000])
        assert dev.ctx.splitlink_stats() == (len(links), 0)
        found = dev.junctions()
        assert found == sj.junctions_fast(links, clens) and len(found) >= 500
        want = so.summaries_fast(pairs, clens, found)
        assert max(w[0] for w in want) >= 20 and any(w[1] < 0 for w in want) and any(w[1] > 0 for w in want) and any(w[2] < w[0] for w in want)
        assert all(w[0] <= j[7] + j[8] for w, j in zip(want, found)) and any(w[0] < j[7] + j[8] for w, j in zip(want, found))
        assert dev.overlap(found) == want
        sample = found[::40]
        assert want[::40] == [so.junction_summary(pairs, clens, j) for j in sample]          # the two restatements
        assert dev.overlap(found, 255) == so.summaries_fast(pairs, clens, found, 255)
        assert dev.overlap(found, 0) == so.summaries_fast(pairs, clens, found, 0)
    finally:
        dev.close()


# ------------------------------------------------------------------------------------------ 9. the product

def _run(binary, flags, cwd, env=None):
    e = dict(os.environ)
    e.update(env or {})
    return subprocess.run([binary] + flags + ["ref.fa", "sample=aln.bam"], cwd=cwd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=e, timeout=120)


def _ok(r):
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    assert b"overflowed" not in r.stderr
    return r


def _err(r):
    """stderr without the whole seconds of its time stamps, which differ between two runs that straddle a second"""
    return re.sub(rb" : \d+ sec\. elapsed\n", b"\n", r.stderr)


BASE = ["-i", "cfg.txt", "-s", "100"]
PATHS = {"pipelined": {}, "record at a time": {"INDELMINER_PIPELINE": "host"}, "three walkers": {"INDELMINER_PIECE_BYTES": "60000", "INDELMINER_WALKERS": "3"}}


@pytest.fixture(scope="module")
def planted(tmp_path_factory):
    refs, rd = so.planted_truth()
    d = so.write_planted(str(tmp_path_factory.mktemp("splitoverlap")), refs, rd)
    bam, fa = d + "/aln.bam", d + "/ref.fa"
    with_h, found, sums = so.render_of_bam(bam, fa)
    with_hk = so.render_of_bam(bam, fa, genotype=True)[0]
    assert sums == so.PLANTED_SUMMARY and len(found) == 4 and with_h != with_hk
    return d, with_h, with_hk, sj.render_of_bam(bam, fa, 10)[0], jg.render_of_bam(bam, fa)[0]


@pytest.mark.parametrize("path", list(PATHS))
def test_product_file_on_the_planted_data_set(planted, path, tmp_path):
    """a clean junction, 7 and 40 bases of homology and 12 inserted bases, reads from both ends: FILE with -H and with -H -K byte for
    byte the restatement's; stdout and stderr what they are without -H"""
    d, with_h, with_hk, _, _ = planted
    prod = _product()
    f = lambda name: str(tmp_path / name)
    read = lambda name: open(f(name), "rb").read()
    r0 = _ok(_run(prod, BASE + ["-G", "-J", f("j0"), "-K"], d, env=PATHS[path]))
    r1 = _ok(_run(prod, BASE + ["-G", "-J", f("j1"), "-H"], d, env=PATHS[path]))
    r2 = _ok(_run(prod, BASE + ["-H", "-K", "-G", "-J", f("j2")], d, env=PATHS[path]))
    assert read("j1") == with_h and read("j2") == with_hk
    assert r1.stdout == r0.stdout == r2.stdout and _err(r1) == _err(r0) == _err(r2)
    info = [ln.split(b"\t")[7].split(b";", 6)[6].decode() for ln in read("j2").split(b"\n") if ln and not ln.startswith(b"#")]
    assert info == so.PLANTED_INFO


def test_product_without_the_option_detailed_output_and_the_refusal(planted, tmp_path):
    d, with_h, _, plain, plain_k = planted
    prod = _product()
    f = lambda name: str(tmp_path / name)
    read = lambda name: open(f(name), "rb").read()
    _ok(_run(prod, BASE + ["-G", "-J", f("j0")], d))
    _ok(_run(prod, BASE + ["-G", "-J", f("j1"), "-K"], d))
    assert read("j0") == plain and read("j1") == plain_k                                    # without -H: the parent's FILE
    d0 = _ok(_run(prod, BASE + ["-o", "detailed"], d))
    d1 = _ok(_run(prod, BASE + ["-o", "detailed", "-G", "-J", f("none"), "-H"], d))
    assert d1.stdout == d0.stdout and _err(d1) == _err(d0) and not os.path.exists(f("none"))
    r = _run(prod, BASE + ["-G", "-H"], d)
    assert r.returncode != 0 and r.stdout == b"" and r.stderr == b"indelminer: -H needs -J\n"
    r = _run(prod, BASE + ["-H", "-J", f("none")], d)
    assert r.returncode != 0 and r.stdout == b"" and r.stderr == b"indelminer: -J needs -G\n" and not os.path.exists(f("none"))
    # the chain in front of it leaves the other FILEs alone
    chain = lambda k: ["-G", "-C", "-V", "-U", f("u%d" % k), "-N", f("n%d" % k), "-T", f("t%d" % k), "-M", "-S", "-J", f("c%d" % k)]
    c0 = _ok(_run(prod, BASE + chain(0), d))
    c1 = _ok(_run(prod, BASE + chain(1) + ["-H"], d))
    assert read("c0") == plain and read("c1") == with_h and c1.stdout == c0.stdout and _err(c1) == _err(c0)
    assert (read("u1"), read("n1"), read("t1")) == (read("u0"), read("n0"), read("t0"))
