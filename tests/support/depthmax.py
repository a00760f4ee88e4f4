"""Inputs and yardstick for im_depth_query_max_tid and im_depth_query_max: the sum over [beg, end) and the DEEPEST position of
[beg - 1, end], the query the host driver makes for every printed variant (host_logic.c, depth_sum_deepest: on the genome-wide array in
pipeline mode, on what im_depth_build left on the record-at-a-time path); its maximum decides whether DP= is re-derived from the
file (deepest >= 4000).  A maximum that comes out too low is silent everywhere but at a deep locus.  The driver sends every window
twice: as it is, and drawn out to the front by the longest reference span it has seen (lookback_queries).

Records: plain matching reads of matchrecs.BASES bases on the two contigs of tests/test_gpu_depth_scan_shapes.py's genome-wide test, a
random background, and SPIKES -- k records starting at one position p, which raise the depth on [p, p + BASES) by k.  A query with
beg = p + BASES sees the spike at beg - 1 alone; one with end = p sees it at position `end` alone.

The yardstick is numpy on the cumsum of the difference array, independent of the CPU shim: tests/test_depth_max_host.py holds the
shim (the product's CPU stand-in) to it, tests/test_gpu_depth_max.py the kernel."""
import numpy as np

from tests.support.matchrecs import BASES, match_records

TILE = 8192
CLENS = [33 * TILE + 4, TILE]
DEEP = 8200                 # once: the maximum crosses the driver's threshold (4000) and samtools' pileup cap (8000)
K = 37

# (tid, position, records): interior of a tile; the last BASES positions of a tile; the first of a tile; and on the second contig
# an interior one and the contig's last BASES positions
SPIKES = [(0, 3 * TILE + 100, DEEP), (0, 5 * TILE - BASES, K), (0, 7 * TILE, K + 1), (0, 40, K + 2),
          (1, 1000, 4100), (1, CLENS[1] - BASES, K), (1, 3000, K + 3)]


def positions(seed=33):
    """per contig the sorted start positions of its records"""
    rng = np.random.default_rng(seed)
    pos = []
    for t, clen in enumerate(CLENS):
        p = [rng.integers(0, clen, 6000 if t == 0 else 500)]
        p += [np.full(k, at) for tt, at, k in SPIKES if tt == t]
        pos.append(np.sort(np.concatenate(p)))
    return pos


def records(seed=33):
    """(raw, rec_off, depth): the records sorted by (tid, pos) and per contig depth[0 .. clen - 1] by the difference array's cumsum"""
    tid, pos, depth = [], [], []
    for t, (clen, p) in enumerate(zip(CLENS, positions(seed))):
        tid.append(np.full(len(p), t)); pos.append(p)
        diff = np.zeros(clen + 1, np.int64)
        np.add.at(diff, p, 1); np.add.at(diff, np.minimum(p + BASES, clen), -1)
        full = np.cumsum(diff)
        assert full[clen] == 0
        depth.append(full[:clen])
    raw, off = match_records(np.concatenate(tid), np.concatenate(pos))
    return raw, off, depth


def queries(t):
    """(beg, end) int32 arrays for contig t: the grid, the spike queries, and clipped ones; every one has beg < end and meets the contig"""
    clen = CLENS[t]
    q = []
    for beg in (0, 1, TILE - 1, TILE, TILE + 1):
        for end in (beg + 1, beg + 63, beg + 64, beg + 65, beg + 129, clen - 1, clen, clen + 9):
            q.append((beg, end))
    for tt, p, _k in SPIKES:
        if tt != t:
            continue
        b = p + BASES                       # the spike at beg - 1 alone
        q += [(b, b + 1), (b, b + 65)]
        q += [(p - 1, p), (p - 70, p)]      # the spike at position `end` alone
        q += [(p, p + BASES), (p - 3, p + 9)]
    q += [(-5, 3), (-5, clen + 9), (clen - 1, clen), (clen - 1, clen + 9), (clen - 2, clen - 1)]
    q = [(b, e) for b, e in q if b < e and max(b, 0) < min(e, clen)]
    return np.array([b for b, e in q], np.int32), np.array([e for b, e in q], np.int32)


BACKS = (260, TILE + 1000)        # a record with a gap; a record longer than a tile of the scan


def lookback_queries(t):
    """the second half of the driver's call: every query of queries(t) with beg drawn out to the front by `back` bases, not below 0
    (as depth_sum_deepest does) -- across tile edges, and at beg - back < 0"""
    beg, end = queries(t)
    b = np.concatenate([np.where(beg > back, beg - back, 0) for back in BACKS]).astype(np.int32)
    crossing = int(((b // TILE) != (np.concatenate([beg, beg]) // TILE)).sum())          # the second contig is one tile long
    assert (b == 0).sum() > 10 and (b > 0).sum() > 10 and (crossing > 10 or CLENS[t] <= TILE)
    return b, np.concatenate([end, end]).astype(np.int32)


def model(depth, beg, end):
    """(sum, max) per query by the statement in include/indelminer_amd.h"""
    clen = len(depth)
    s, m = [], []
    for b0, e0 in zip(beg, end):
        a, b = max(int(b0), 0), min(int(e0), clen)
        assert a < b
        s.append(int(depth[a:b].sum()))
        m.append(int(depth[a - 1 if a > 0 else a:b + 1 if b < clen else b].max()))
    return np.array(s, np.uint32), np.array(m, np.uint32)


def check_teeth(depth):
    """the spike queries are what they claim: the maximum of the yardstick lies outside [beg, end) for them"""
    n = 0
    for t, p, k in SPIKES:
        d = depth[t]
        for b, e in ((p + BASES, p + BASES + 1), (p + BASES, p + BASES + 65), (p - 1, p), (p - 70, p)):
            if b < 0 or e > len(d):
                continue
            inside = int(d[b:e].max())
            _, m = model(d, [b], [e])
            assert int(m[0]) >= k > inside, (t, p, k, b, e, inside, int(m[0]))
            n += 1
    return n
