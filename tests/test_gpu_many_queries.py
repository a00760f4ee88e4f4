"""The query kernels past one grid: pairlink_count_kernel, matelink_partner_kernel, splitlink_count_kernel, splitlink_overlap_kernel and
junction_pairs_kernel of im_links.hip and cliptail_verify_kernel, cliptail_consensus_kernel and cliptail_junction_kernel of
im_cliptail.hip give one wave to a query and take query q + 8 192 in the same wave (wave_grid, im_keyed.hpp).  Every entry point is asked
8 192, 8 193, 16 385 and 20 011 queries -- one trip, one wave on a second trip, one wave on a third, a ragged last trip -- and 8 193 once
more with the queries rotated by one, so that another wave makes the second trip.

The queries are the 97 hand-classed base queries of tests/support/manyqueries.py, tiled; the expected answers are the plain restatements'
answers to the 97, tiled the same way (tests/test_manyqueries_host.py pins the plan).  Every output column is compared whole and exactly,
over output arrays that went in full of a sentinel: an answer that was not written shows as well as a wrong one.
"""
import ctypes as C

import numpy as np
import pytest

from tests.support import manyqueries as mq
from tests.support import splitoverlap as so

pytestmark = pytest.mark.gpu

SENTINEL = 0x77777777
MAX_SHIFT = 32
Q = 10


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


class Device:
    """one context over the plan's contigs with the tables asked for, filled through the _add entries with the plan's entries"""

    def __init__(self, pair=False, mate=False, split=False, tail=False):
        from indelminer_amd import capi
        self.capi, self.lib = capi, capi.lib()
        self.ctx = ctx = capi.Context(0)
        ctx.set_reference(mq.refs())
        L, tids = mq.LOG2_SLOTS, range(len(mq.CLENS))
        if pair:
            links = mq.pair_links()[0]
            ctx.pairlink_enable(Q, L["pair"])
            ctx.pairlink_stretched_enable()
            for t in tids:
                mine = [l for l in links if l[0] == t]
                if mine:
                    ctx.pairlink_add(t, [l[2] for l in mine], [l[3] for l in mine], [l[1] for l in mine])
            assert ctx.pairlink_stats() == (len(links), 0)
        if mate:
            links = mq.mate_links()[0]
            ctx.matelink_enable(Q, L["mate"])
            for t in tids:
                mine = [l for l in links if l[0] == t]
                if mine:
                    ctx.matelink_add(t, [l[2] for l in mine], [l[3] for l in mine], [l[4] for l in mine], [l[1] for l in mine])
            assert ctx.matelink_stats() == (len(links), 0)
        if split:
            pairs = mq.split_pairs()[0]
            ctx.splitlink_enable(20, Q, L["split"], ["ctg%d" % t for t in tids])
            ctx.splitlink_overlap_enable()
            ctx.splitlink_add_overlap(*[[l[k] for l, _ in pairs] for k in range(6)], [so.UNKNOWN if d is None else d for _, d in pairs])
            assert ctx.splitlink_stats() == (len(pairs), 0)
        if tail:
            entries = mq.tail_entries(mq.tail_table()[0])
            ctx.cliptail_enable(20, Q, L["tail"])
            for t, (pos, side, nbases, planes) in entries.items():
                ctx.cliptail_add(t, pos, side, nbases, planes)
            assert ctx.cliptail_stats() == (sum(len(e[0]) for e in entries.values()), 0)

    def close(self):
        self.ctx.close()


def _call(dev, name, nq, qs):
    """the entry itself over output columns full of SENTINEL: the answer columns in the order of the plan's answers"""
    h, lib = dev.ctx.h, dev.lib
    out = lambda kinds, n=nq: [np.full(n, SENTINEL, t) for t in kinds]
    q = [_p(c) for c in qs]
    P = mq.plan(name)
    if name == "im_cliptail_consensus":
        entries, ln, agree = out((np.uint32,) * 3)
        planes = np.full(2 * nq, SENTINEL, np.uint32)
        rc = lib.im_cliptail_consensus(h, 0, nq, *q, mq.MIN_COVER, _p(entries), _p(ln), _p(planes), _p(agree))
        outs = [entries, ln, planes[0::2].copy(), planes[1::2].copy(), agree]
    else:
        outs = out(P.out_kinds)
        o = [_p(c) for c in outs]
        if name == "im_pairlink_count":
            rc = lib.im_pairlink_count(h, 0, nq, *q, mq.MIN_SEP, *o)
        elif name == "im_matelink_partner":
            rc = lib.im_matelink_partner(h, 0, nq, *q, *o)
        elif name == "im_splitlink_count":
            rc = lib.im_splitlink_count(h, nq, *q, *o)
        elif name == "im_splitlink_overlap":
            rc = lib.im_splitlink_overlap(h, nq, *q, mq.OVERLAP_WINDOW, *o)
        elif name == "im_junction_pairs":
            from tests.support import junctionpairs as jp
            rc = lib.im_junction_pairs(h, nq, *q, jp.REACH, jp.BACK, jp.MIN_SEP, *o)
        elif name == "im_cliptail_verify":
            rc = lib.im_cliptail_verify(h, 0, nq, *q, MAX_SHIFT, *o)
        else:
            assert name == "im_cliptail_junction"
            rc = lib.im_cliptail_junction(h, nq, *q, MAX_SHIFT, *o)
    assert rc == 0, (name, nq, lib.im_last_error(h).decode())
    return outs


def ask(dev, name, nq, by=0):
    """one call of nq tiled queries (the base set rotated by `by`): every column equals the tiled expectation; returns the columns"""
    P = mq.plan(name)
    qs, want = P.columns(nq, by)
    got = _call(dev, name, nq, qs)
    assert len(got) == len(want) == len(P.out_kinds)
    for k, (g, w) in enumerate(zip(got, want)):
        # (i, i % 97 -- the base query is that plus `by` --, trip i // 8192, got, expected) of the first rows that differ
        assert g.dtype == w.dtype and len(g) == nq and np.array_equal(g, w), (name, "nq %d" % nq, "rotated by %d" % by, "column %d" % k, mq.first_mismatches(g, w))
    return got


def every_size(dev, name):
    for nq in mq.SIZES:
        ask(dev, name, nq)
    ask(dev, name, 8193, by=1)


@pytest.fixture(scope="module")
def links_device():
    dev = Device(pair=True, mate=True, split=True)
    yield dev
    dev.close()


@pytest.fixture(scope="module")
def tails_device():
    dev = Device(tail=True)
    yield dev
    dev.close()


def test_pairlink_count_past_one_grid(links_device):
    """kinds 0 .. 3 with the stretched form enabled"""
    every_size(links_device, "im_pairlink_count")


def test_matelink_partner_past_one_grid(links_device):
    """the wave's LDS cell table after a query of many cells, of one, of none"""
    every_size(links_device, "im_matelink_partner")


def test_splitlink_count_past_one_grid(links_device):
    every_size(links_device, "im_splitlink_count")


def test_splitlink_overlap_past_one_grid(links_device):
    """the eighteen passes of the bisection after a junction of 130 and more links, of none that states an overlap, of none at all"""
    every_size(links_device, "im_splitlink_overlap")


def test_junction_pairs_past_one_grid(links_device):
    """ends on one contig (the pair links) and on two (the mate links) in one call"""
    every_size(links_device, "im_junction_pairs")


def test_cliptail_verify_past_one_grid(tails_device):
    every_size(tails_device, "im_cliptail_verify")


def test_cliptail_consensus_past_one_grid(tails_device):
    every_size(tails_device, "im_cliptail_consensus")


def test_cliptail_junction_past_one_grid(tails_device):
    every_size(tails_device, "im_cliptail_junction")


def _small_tasks():
    """50 small Smith-Waterman tasks: windows of 30 .. 120 bases of contig 0, queries cut from them with a deletion or a substitution"""
    rng = np.random.default_rng(50)
    ref = mq.refs()[0]
    targets, queries = [], []
    for i in range(50):
        p, n = int(rng.integers(0, 50_000)), int(rng.integers(30, 121))
        t = ref[p:p + n]
        q = bytearray(t[3:n // 2] + t[n // 2 + i % 4:n - 2])
        q[len(q) // 3] = ord("ACGT"[i % 4])
        targets.append(t)
        queries.append(bytes(q))
    return targets, queries


def test_the_workspace_in_sequence():
    """one context's workspace grows, is carved another way by im_support_batch, and takes an answer of 8-byte elements over two columns:
    every answer of the sequence is what a context that has done nothing else gives (and, for the queries, the restatement's)"""
    from tests.support import knowncounts as kc
    targets, queries = _small_tasks()
    steps = [("im_pairlink_count", 20_011), ("im_pairlink_count", 3), ("im_pairlink_count", 8_193), ("im_support_batch", 50),
             ("im_cliptail_consensus", 8_193), ("im_pairlink_count", 8_193)]

    def run(dev, name, n):
        if name == "im_support_batch":
            return [dev.ctx.support_batch(targets, queries)]
        return ask(dev, name, n)

    one = Device(pair=True, tail=True)
    try:
        for name, n in steps:
            got = run(one, name, n)
            fresh = Device(pair=name == "im_pairlink_count", tail=name == "im_cliptail_consensus")
            try:
                want = run(fresh, name, n)
            finally:
                fresh.close()
            assert len(got) == len(want) and all(np.array_equal(g, w) for g, w in zip(got, want)), (name, n)
            if name == "im_support_batch":
                assert [tuple(int(x) for x in r[:3]) for r in got[0]] == [kc.sw_stats(t, q) for t, q in zip(targets, queries)] and (got[0][:, 3] == 1).all()
    finally:
        one.close()
