"""The tiled scan of im_depth.hip at the shapes where it can go wrong, through the C ABI only: im_depth_build + im_depth_query on the
one-contig array, and im_depth_scan / im_depth_reset / im_depth_query_tid on the genome-wide array of a two-contig context.

The yardstick is numpy.cumsum of the difference array, position by position: integers, so equality.  Nothing here knows how the
scan is laid out beyond the three sizes the shapes are chosen by: the tile of 8192 positions, the 32 tiles that count their arrival
into one word, and the 1024 tile totals of one round of the offset pass.
"""
import numpy as np
import pytest

from tests.support.matchrecs import BASES, match_records

pytestmark = pytest.mark.gpu

TILE, GROUP, ROUND = 8192, 32, 1024

# clen + 1, the number of entries of the array
SMALL = [1, 2, 7, 8, 9, TILE - 1, TILE, TILE + 1]
GROUP_EDGES = [GROUP * TILE - 1, GROUP * TILE, GROUP * TILE + 1, (GROUP + 1) * TILE + 5]
SECOND_ROUND = [ROUND * TILE + 1]


def _segments(rng, clen, nseg):
    """intervals of 1..100 positions, one in eight up to 20 000 long (it closes tiles behind the one it opens in: their local sums
    run negative), some reaching out of the contig on both sides"""
    start = rng.integers(-50, clen + 20, nseg)
    ln = np.where(rng.integers(0, 8, nseg) == 0, rng.integers(1, 20_001, nseg), rng.integers(1, 101, nseg))
    return start.astype(np.int32), ln.astype(np.int32)


def _depth(clen, start, ln):
    """the difference array of the clipped intervals and its cumsum: depth[0 .. clen - 1], and the whole array's last entry"""
    diff = np.zeros(clen + 1, np.int64)
    a = np.clip(start.astype(np.int64), 0, clen); b = np.clip(start.astype(np.int64) + ln, 0, clen)
    ok = a < b
    np.add.at(diff, a[ok], 1); np.add.at(diff, b[ok], -1)
    full = np.cumsum(diff)
    assert full[clen] == 0 and (full >= 0).all()
    return full[:clen], diff


def _check_build(ctx, clen, start, ln):
    ctx.depth_build(clen, start, ln)
    depth, _ = _depth(clen, start, ln)
    p = np.arange(clen, dtype=np.int32)
    got = ctx.depth_query(p, p + 1).astype(np.int64)
    bad = np.nonzero(got != depth)[0]
    assert len(bad) == 0, (clen, bad[:8], got[bad[:8]], depth[bad[:8]])
    # whole-contig and cross-tile range sums, clipped at both ends
    csum = np.concatenate([[0], np.cumsum(depth)])
    qb = np.array([0, -7, clen // 2, max(clen - 3, 0), TILE - 1, 0], np.int64)
    qe = np.array([clen, clen + 9, clen, clen + 1, TILE + 1, 1], np.int64)
    ca, cb = np.clip(qb, 0, clen), np.clip(qe, 0, clen)
    want = np.where(ca < cb, csum[cb] - csum[ca], 0).astype(np.uint32)
    assert np.array_equal(ctx.depth_query(qb.astype(np.int32), qe.astype(np.int32)), want), clen


@pytest.fixture(scope="module")
def ctx():
    from indelminer_amd import capi
    c = capi.Context(0)
    yield c
    c.close()


@pytest.mark.parametrize("n", SMALL + GROUP_EDGES)
def test_build_and_query_at_tile_and_group_edges(ctx, n):
    rng = np.random.default_rng(n)
    clen = n - 1
    start, ln = _segments(rng, clen, min(60_000, 40 + clen // 4))
    _check_build(ctx, clen, start, ln)


def test_second_round_of_the_offset_pass(ctx):
    """one tile more than a round of the offset pass takes: the running offset crosses into the second round"""
    rng = np.random.default_rng(5)
    for n in SECOND_ROUND:
        start, ln = _segments(rng, n - 1, 300_000)
        _check_build(ctx, n - 1, start, ln)


def test_long_contig_then_short_one_on_one_array():
    """two builds in sequence on ONE ContigArray: where the short contig's arrival counters lie, the long one left tile offsets"""
    from indelminer_amd import capi
    rng = np.random.default_rng(9)
    c = capi.Context(0)
    try:
        for n in ((GROUP + 1) * TILE + 5, TILE + 1, 2 * GROUP * TILE + 3, 7, GROUP * TILE, 1):
            start, ln = _segments(rng, n - 1, min(60_000, 40 + n // 4))
            _check_build(c, n - 1, start, ln)
    finally:
        c.close()


def test_negative_running_sums_inside_a_tile(ctx):
    """-1 events in front of +1 events in index order: intervals that open in one tile and close in a later one leave the later
    tile's local sums, and its total, below zero"""
    clen = 4 * TILE
    start = np.array([100, TILE + 50, TILE - 200, 5, 2 * TILE + 9, 3 * TILE - 1, TILE - 1, 3 * TILE + 7000], np.int32)
    end = np.array([TILE + 10, TILE + 60, 3 * TILE + 5, 2 * TILE + 1, 2 * TILE + 10, 3 * TILE + 1, TILE, 4 * TILE + 90], np.int32)
    ln = (end - start).astype(np.int32)
    _, diff = _depth(clen, start, ln)
    local = np.cumsum(diff[:clen].reshape(-1, TILE), axis=1)
    assert local[1].min() < 0 and local[1][-1] < 0 and local[2].min() < 0 and local[3].min() < 0       # what the case is for
    _check_build(ctx, clen, start, ln)


def _genome_depth(ctx, capi, pipe, clens):
    out = []
    for t, clen in enumerate(clens):
        ctx.depth_scan(t)
        p = np.arange(clen, dtype=np.int32)
        out.append(ctx.depth_query_tid(t, p, p + 1).astype(np.int64))
    return out


def test_genome_array_scanned_twice_with_a_reset_between():
    """the tid form on a two-contig context: each contig's run is scanned at its own length only, so its counters are zeroed once,
    at allocation -- a second scan (reset, the same scatter, scan) is right only if the first left every counter at zero.  The
    first contig has a second arrival group of one tile, the second ends one entry into its second tile."""
    from indelminer_amd import capi
    rng = np.random.default_rng(21)
    clens = [(GROUP + 1) * TILE + 4, TILE]            # clen + 1 = 33 * 8192 + 5 and 8193
    tid, pos = [], []
    for t, clen in enumerate(clens):
        edges = np.concatenate([np.arange(TILE, clen, TILE) - 2, np.arange(TILE, clen, TILE), [0, clen - 2, clen - BASES, clen - 1]])
        p = np.sort(np.concatenate([rng.integers(0, clen, 6000 if t == 0 else 500), edges]))
        tid.append(np.full(len(p), t)); pos.append(p)
    tid, pos = np.concatenate(tid), np.concatenate(pos)
    raw, off = match_records(tid, pos)
    want = []
    for t, clen in enumerate(clens):
        sel = pos[tid == t]
        depth, _ = _depth(clen, sel.astype(np.int32), np.full(len(sel), BASES, np.int32))
        want.append(depth)
    ctx = capi.Context(0)
    try:
        ctx.set_reference([b"A" * n for n in clens])
        ctx.set_insert_ranges(["generic"], [700])
        ctx.depth_enable()
        pipe = capi.Pipeline(ctx, len(off) - 1, len(raw), cap_cand=len(off) - 1, want_depth=True)
        pipe.upload(raw, off)
        for _round in range(2):
            pipe.triage()
            pipe.sync()
            got = _genome_depth(ctx, capi, pipe, clens)
            for t in range(len(clens)):
                bad = np.nonzero(got[t] != want[t])[0]
                assert len(bad) == 0, (_round, t, bad[:8], got[t][bad[:8]], want[t][bad[:8]])
            for t in range(len(clens)):
                ctx._check(capi.lib().im_depth_reset(ctx.h, t, ctx.stream))
    finally:
        ctx.close()
