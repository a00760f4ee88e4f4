"""The median query on the depth arrays (im_depth_median, im_depth_median_tid; the kernel is in im_depth.hip).

The yardstick is the plain restatement in this file and in tests/support/depthmedian.py (pinned to hand-worked cases by
tests/test_depth_evidence_host.py, without a GPU), written from the definition in include/indelminer_amd.h: difference array ->
cumsum -> clamp at 4095 -> sort -> element (n - 1) // 2 of the n positions of [beg, end) clipped to [0, clen); 0xFFFFFFFF for an
interval without positions.  The kernel cuts an interval into slabs of 32768 positions counted from its first position rounded down
to a multiple of 4, and the scan leaves the array in tiles of 8192 positions: the queries below sit on both kinds of boundary.
"""
import ctypes as C
import struct

import numpy as np
import pytest

from tests.support.depthmedian import CAP, NONE, medians

pytestmark = pytest.mark.gpu

TILE = 8192
SLAB = 32768


# ------------------------------------------------------------------------------------------ the restatement

def depth_of_intervals(start, length, clen):
    """[start, start + length) clipped to [0, clen), +1 each -> depth[0 .. clen)"""
    a = np.clip(start.astype(np.int64), 0, clen); b = np.clip(start.astype(np.int64) + length, 0, clen)
    ok = a < b
    d = np.zeros(clen + 1, np.int64)
    np.add.at(d, a[ok], 1); np.add.at(d, b[ok], -1)
    return np.cumsum(d)[:clen]


# ------------------------------------------------------------------------------------------ the host-buffer form

def queries_for(clen, rng):
    q = [(0, clen), (-7, clen + 9), (0, clen - 1), (1, clen)]                                   # the whole contig, hanging off both ends
    q += [(int(p), int(p) + 1) for p in rng.integers(0, clen, 12)] + [(0, 1), (clen - 1, clen)]  # single positions
    edges = [TILE - 1, TILE, TILE + 1, SLAB - 1, SLAB, SLAB + 1, 2 * SLAB - 1, 2 * SLAB, 2 * SLAB + 1]
    for e in edges:
        for s in (0, 1, 2, 3, 4, 5, e - 3, e - 2, e - 1):                                        # even and odd lengths among them
            q += [(s, e), (e, e + 1 + s % 7), (e, e + 700)]
        q += [(e, clen), (e - 1, clen + 3), (5, 4 + SLAB + e % 3 - 1), (5, 4 + SLAB + e % 3)]    # ends on the query's own slab boundary
    for s in (0, 3, 5, 4097):                                                                    # the slab boundaries of a query that starts at s
        b0 = (s & ~3) + SLAB
        q += [(s, b0 - 1), (s, b0), (s, b0 + 1), (s, b0 + SLAB - 1), (s, b0 + SLAB), (s, b0 + SLAB + 1)]
    q += [(int(a), int(a) + int(l)) for a, l in zip(rng.integers(-50, clen + 20, 60), rng.integers(0, 3000, 60))]
    q += [(clen, clen + 5), (clen + 1, clen + 9), (-9, -2), (-5, 0), (40, 40), (41, 40), (clen, 0), (7, -7)]   # empty after the clip, beg > end
    return np.array([a for a, b in q], np.int32), np.array([b for a, b in q], np.int32)


@pytest.fixture(scope="module")
def ctx():
    from indelminer_amd import capi
    c = capi.Context(0)
    yield c
    c.close()


@pytest.mark.parametrize("clen", [1, 8191, 8192, 8193, 20_000, 70_000])
def test_host_buffer_form(ctx, clen):
    rng = np.random.default_rng(clen)
    n = 4000
    start = rng.integers(-80, clen + 20, n).astype(np.int32)
    length = rng.choice([1, 30, 100, 250, 3000], n).astype(np.int32)
    depth = depth_of_intervals(start, length, clen)
    ctx.depth_build(clen, start, length)
    beg, end = queries_for(clen, rng)
    want = medians(depth, beg, end)
    assert (want == NONE).sum() >= 8 and (want != NONE).sum() > (100 if clen > 1 else 20)
    got = ctx.depth_median(beg, end).astype(np.int64)
    bad = np.nonzero(got != want)[0]
    assert len(bad) == 0, (clen, [(int(beg[i]), int(end[i]), int(got[i]), int(want[i])) for i in bad[:8]])
    if clen == 70_000:
        # more than two slabs, mixed with one-slab queries in the same call: the hand-over between the slabs of a query and the
        # histograms in device memory, which the same call a second time finds as the first left them
        assert ((np.minimum(end, clen) - np.maximum(beg, 0)) > 2 * SLAB).sum() >= 4
        order = rng.permutation(len(beg))
        for _again in range(2):
            assert np.array_equal(ctx.depth_median(beg[order], end[order]).astype(np.int64), want[order])
    # the same call a second time
    assert np.array_equal(ctx.depth_median(beg, end).astype(np.int64), want)
    assert len(ctx.depth_median(np.zeros(0, np.int32), np.zeros(0, np.int32))) == 0
    # the sum query next to it reads the same array
    assert np.array_equal(ctx.depth_query(beg[:4], end[:4]).astype(np.int64),
                          [depth[max(int(a), 0):min(int(b), clen)].sum() for a, b in zip(beg[:4], end[:4])])


def test_saturation(ctx):
    clen = 1000
    start = np.full(4200, 300, np.int32); length = np.full(4200, 300, np.int32)
    depth = depth_of_intervals(start, length, clen)
    assert depth[300] == 4200 and depth[299] == 0 and depth[600] == 0
    ctx.depth_build(clen, start, length)
    beg = np.array([350, 300, 150, 151, 0, 450], np.int32); end = np.array([400, 600, 450, 450, 1000, 751], np.int32)
    want = medians(depth, beg, end)
    assert list(want[:4]) == [CAP, CAP, 0, CAP]              # inside; half inside: 150 of 300 at zero, then 149 of 299
    assert np.array_equal(ctx.depth_median(beg, end).astype(np.int64), want)


# ------------------------------------------------------------------------------------------ the genome-wide form

def raw_records(records):
    """[(tid, pos, mapq, flag, [(op, len)])] -> the device layout (raw uint8, rec_off uint32[n + 1]), 4-byte aligned starts"""
    blob, off = bytearray(), [0]
    for i, (tid, pos, mapq, flag, cigar) in enumerate(records):
        qname = b"m%d\0" % i
        l_seq = sum(ln for op, ln in cigar if op in (0, 1, 4, 7, 8))
        core = struct.pack("<iiBBHHHiiii", tid, pos, len(qname), mapq, 4680, len(cigar), flag, l_seq, tid, pos, 0)
        body = core + qname + b"".join(struct.pack("<I", (ln << 4) | op) for op, ln in cigar) + b"\x11" * ((l_seq + 1) // 2) + b"\x28" * l_seq
        blob += body + b"\0" * (-len(body) % 4)
        off.append(len(blob))
    return np.frombuffer(bytes(blob), np.uint8).copy(), np.array(off, np.uint32)


def pileup_depth(records, clens):
    """what samtools' pileup counts: records outside the mask, the positions under M / = / X"""
    out = [np.zeros(c + 1, np.int64) for c in clens]
    for tid, pos, mapq, flag, cigar in records:
        if flag & (0x4 | 0x100 | 0x200 | 0x400) or not 0 <= tid < len(clens):
            continue
        x = pos
        for op, ln in cigar:
            if op in (0, 7, 8):
                a, b = max(x, 0), min(x + ln, clens[tid])
                if a < b:
                    out[tid][a] += 1; out[tid][b] -= 1
            if op in (0, 2, 3, 7, 8):
                x += ln
    return [np.cumsum(d)[:c] for d, c in zip(out, clens)]


def test_genome_wide_form():
    from indelminer_amd import capi
    clens = [3_000, 20_000]                 # the second contig's run starts behind the first's and has tile sums of its own
    rng = np.random.default_rng(8)
    F = 0x63
    recs = [(0, int(p), 60, F, [(0, 100)]) for p in rng.integers(0, clens[0] - 100, 500)]
    cigars = [[(0, 100)], [(0, 50), (2, 20), (0, 50)], [(4, 30), (0, 70)], [(7, 40), (8, 1), (7, 59)]]
    recs += [(1, int(p), 60, F, cigars[k]) for p, k in zip(rng.integers(0, clens[1] - 120, 5000), rng.integers(0, len(cigars), 5000))]
    recs += [(1, 9000, 60, F | 0x400, [(0, 100)]), (1, 9001, 60, F | 0x4, [(0, 100)]), (1, clens[1] - 40, 60, F, [(0, 100)])]
    recs.sort(key=lambda r: (r[0], r[1]))
    want_depth = pileup_depth(recs, clens)
    assert want_depth[1].max() > 20 and want_depth[0].max() > 5
    raw, off = raw_records(recs)
    L = capi.lib()
    ctx = capi.Context(0)
    try:
        ctx.set_reference([bytes(rng.choice(np.frombuffer(b"ACGT", np.uint8), n)) for n in clens])
        one = np.zeros(1, np.int32); ten = np.full(1, 10, np.int32); out = np.zeros(1, np.uint32)
        p = lambda a: a.ctypes.data_as(C.c_void_p)
        # in front of im_depth_enable / im_depth_build: what the sum queries answer
        assert L.im_depth_median_tid(ctx.h, 0, 1, p(one), p(ten), p(out)) == L.im_depth_query_tid(ctx.h, 0, 1, p(one), p(ten), p(out)) == capi.E_ARG
        assert L.im_depth_median(ctx.h, 1, p(one), p(ten), p(out)) == L.im_depth_query(ctx.h, 1, p(one), p(ten), p(out)) == capi.E_ARG
        assert L.im_last_error(ctx.h) == b"im_depth_build has not been called"
        ctx.set_insert_ranges(["generic"], [700])
        ctx.depth_enable()
        n = len(off) - 1
        pipe = capi.Pipeline(ctx, n, len(raw), cap_cand=max(n, 16), want_depth=True)
        pipe.upload(raw, off)
        pipe.triage()
        pipe.sync()
        for t, clen in enumerate(clens):
            ctx.depth_scan(t)
        for t, clen in enumerate(clens):
            pos = np.arange(clen, dtype=np.int32)
            assert np.array_equal(ctx.depth_query_tid(t, pos, pos + 1).astype(np.int64), want_depth[t]), t      # the array is what the restatement says
            beg, end = queries_for(clen, rng)
            want = medians(want_depth[t], beg, end)
            got = ctx.depth_median_tid(t, beg, end).astype(np.int64)
            bad = np.nonzero(got != want)[0]
            assert len(bad) == 0, (t, [(int(beg[i]), int(end[i]), int(got[i]), int(want[i])) for i in bad[:8]])
            assert np.array_equal(ctx.depth_median_tid(t, beg, end).astype(np.int64), want)
        for tid, nq in ((-1, 1), (2, 1), (0, -1)):
            assert L.im_depth_median_tid(ctx.h, tid, nq, p(one), p(ten), p(out)) == L.im_depth_query_tid(ctx.h, tid, nq, p(one), p(ten), p(out)) == capi.E_ARG
        assert L.im_depth_median_tid(ctx.h, 0, 1, None, p(ten), p(out)) == capi.E_ARG
        assert L.im_depth_median_tid(ctx.h, 0, 0, None, None, None) == capi.IM_OK
    finally:
        ctx.close()
