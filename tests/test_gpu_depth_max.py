"""im_depth_query_max_tid on the GPU (depth_query_tiled_kernel with out_max, im_depth.hip): the query behind every DP= the product
prints in pipeline mode.  The records of tests/support/depthmax.py go through triage (want_depth) into the genome-wide difference
array of a two-contig context, im_depth_scan turns each contig into depths, and every query is held to the numpy statement of
depthmax.model -- the same statement tests/test_depth_max_host.py holds the CPU shim to.  Integers: equality."""
import numpy as np
import pytest

from tests.support import depthmax as dm

pytestmark = pytest.mark.gpu


def test_sum_and_deepest_position_on_both_contigs():
    from indelminer_amd import capi
    raw, off, depth = dm.records()
    ctx = capi.Context(0)
    try:
        ctx.set_reference([b"A" * n for n in dm.CLENS])
        ctx.set_insert_ranges(["generic"], [700])
        ctx.depth_enable()
        pipe = capi.Pipeline(ctx, len(off) - 1, len(raw), cap_cand=len(off) - 1, want_depth=True)
        pipe.upload(raw, off)
        pipe.triage()
        pipe.sync()
        for t in range(len(dm.CLENS)):
            ctx.depth_scan(t)
        for t in range(len(dm.CLENS)):
            beg, end = dm.queries(t)
            want_sum, want_max = dm.model(depth[t], beg, end)
            got_sum, got_max = ctx.depth_query_max_tid(t, beg, end)
            bad = np.nonzero((got_sum != want_sum) | (got_max != want_max))[0]
            assert len(bad) == 0, (t, [(int(beg[i]), int(end[i]), int(got_sum[i]), int(want_sum[i]), int(got_max[i]), int(want_max[i])) for i in bad[:6]])
            assert np.array_equal(ctx.depth_query_tid(t, beg, end), got_sum)
            # one query to a call, as region_depth asks: the same answers
            for i in (0, len(beg) // 2, len(beg) - 1):
                s, m = ctx.depth_query_max_tid(t, beg[i:i + 1], end[i:i + 1])
                assert (int(s[0]), int(m[0])) == (int(want_sum[i]), int(want_max[i]))
            # the windows drawn out to the front, as the driver sends them beside the plain ones
            beg, end = dm.lookback_queries(t)
            want_sum, want_max = dm.model(depth[t], beg, end)
            got_sum, got_max = ctx.depth_query_max_tid(t, beg, end)
            assert np.array_equal(got_sum, want_sum) and np.array_equal(got_max, want_max), t
        assert int(max(m.max() for m in (dm.model(depth[t], *dm.queries(t))[1] for t in range(2)))) >= dm.DEEP
    finally:
        ctx.close()


def test_sum_and_deepest_position_on_the_one_contig_array():
    """im_depth_query_max: the same kernel on what im_depth_build left, the query of the record-at-a-time path.  Each of the two
    contigs in turn is the built one; plain and drawn-out windows in one call, as the driver sends them."""
    from indelminer_amd import capi
    _, _, depth = dm.records()
    pos = dm.positions()
    ctx = capi.Context(0)
    try:
        for t, clen in enumerate(dm.CLENS):
            ctx.depth_build(clen, pos[t].astype(np.int32), np.full(len(pos[t]), dm.BASES, np.int32))
            b0, e0 = dm.queries(t)
            b1, e1 = dm.lookback_queries(t)
            beg, end = np.concatenate([b0, b1]), np.concatenate([e0, e1])
            want_sum, want_max = dm.model(depth[t], beg, end)
            got_sum, got_max = ctx.depth_query_max(beg, end)
            bad = np.nonzero((got_sum != want_sum) | (got_max != want_max))[0]
            assert len(bad) == 0, (t, [(int(beg[i]), int(end[i]), int(got_sum[i]), int(want_sum[i]), int(got_max[i]), int(want_max[i])) for i in bad[:6]])
            assert np.array_equal(ctx.depth_query(beg, end), got_sum)
            s, m = ctx.depth_query_max(beg[:1], end[:1])
            assert (int(s[0]), int(m[0])) == (int(want_sum[0]), int(want_max[0]))
    finally:
        ctx.close()
