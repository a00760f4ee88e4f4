"""im_depth_reset as one fill launch (16-byte stores and the tail, runs shorter than one store) and the "generic" look-up that
im_set_insert_ranges does once per table on the host: every output compared exactly with the CPU oracle.  The inputs come from
tests/support/resetcases.py; tests/test_reset_generic_host.py proves on the CPU that they reach what they name.  The span, pair-span
and clip resets go through the same launch and are held by their own tests (tests/test_gpu_span.py, test_gpu_pairspan.py,
test_gpu_clip.py)."""
import numpy as np
import pytest

from indelminer_amd import capi
from tests.support import oraclebind as ob
from tests.support import resetcases as rc
from tests.support import triagecases as tc
from tests.test_gpu_triage import _compare_triage

pytestmark = pytest.mark.gpu


def test_depth_of_every_position_and_again_after_the_reset():
    recs = rc.depth_records()
    raw, off = tc.batch(recs)
    n = len(recs)
    clens = rc.CONTIGS
    want = [ob.depth_of(raw, off, t, clen).astype(np.int64) for t, clen in enumerate(clens)]
    ctx = capi.Context(0)
    try:
        ctx.set_reference([b"ACGT"[t % 4:t % 4 + 1] * clen for t, clen in enumerate(clens)])
        ctx.set_insert_ranges(["generic"], [700])
        ctx.depth_enable()
        pipe = capi.Pipeline(ctx, n, len(raw), cap_cand=n, want_depth=True)

        def query(t):
            ctx.depth_scan(t)
            p = np.arange(clens[t], dtype=np.int32)
            return ctx.depth_query_tid(t, p, p + 1).astype(np.int64)

        def reset():
            for t in range(len(clens)):
                ctx._check(capi.lib().im_depth_reset(ctx.h, t, ctx.stream))

        def check(what):
            for t in range(len(clens)):
                got = query(t)
                bad = np.nonzero(got != want[t])[0]
                assert len(bad) == 0, (what, t, bad[:8], got[bad[:8]], want[t][bad[:8]])
        pipe.upload(raw, off)
        pipe.triage()
        pipe.sync()
        check("one chunk")          # the scan has turned every run into prefix sums: no int of a run is zero by chance
        reset()
        for t in range(len(clens)):
            assert not query(t).any(), t
        reset()
        pipe.triage()
        pipe.sync()
        check("after a reset")
        # a reset of one contig leaves its neighbours alone
        reset()
        pipe.triage()
        pipe.sync()
        for t in range(len(clens)):
            ctx.depth_scan(t)
        ctx._check(capi.lib().im_depth_reset(ctx.h, 2, ctx.stream))
        p = [np.arange(clen, dtype=np.int32) for clen in clens]
        for t in (1, 3):
            assert np.array_equal(ctx.depth_query_tid(t, p[t], p[t] + 1).astype(np.int64), want[t]), t
    finally:
        ctx.close()


def test_generic_follows_the_table(gpu_ctx):
    """table after table on one context: what a record without an RG tag gets is what the table of the moment says"""
    recs = rc.generic_records()
    raw, off = tc.batch(recs)
    gpu_ctx.set_reference([b"ACGT" * 500])
    pipe = capi.Pipeline(gpu_ctx, len(recs), len(raw), cap_cand=len(recs), read_len_max=100)
    for names, ranges, want in rc.GENERIC_TABLES:
        gpu_ctx.set_insert_ranges(names, ranges)
        tri, cand = _compare_triage(pipe, raw, off, names, ranges)
        assert (tri[0][0].cls, tri[0][0].range_max) == ((16, 0) if want is None else (3, want)), names
