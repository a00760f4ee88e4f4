"""The overlapped form of the library: several streams on one context, every stage.

The product gives each walker a stream of its own and lets up to 16 of them triage, realign, flush and scatter into the same genome-wide
arrays and keyed tables at once; bench.py times four buffer sets on four streams, each captured into a launch graph and replayed back to
back.  The rest of the suite drives the library on one stream, one pass after the other.  Here the passes of several buffer sets
interleave call by call, their graphs are replayed back to back and over new records, and the scatters of one record set arrive from
four streams -- and every buffer is compared, exactly, with what tests/support/stepmodel.py works out from the CPU oracle and with the
CPU restatements of the genome-wide arrays and keyed tables.  tests/test_overlapped_host.py shows without a GPU that the inputs reach
what these tests name.

Only -g 0 is bound here: the general realign pass (-g 1..60) holds a context mutex and synchronises on the host, so it cannot be
captured into a graph, and it serialises its callers by contract.  Every graph is a plain chain on one stream.  Each test has a context
of its own: they enable context-wide arrays, and the session's context stays as it was.
"""
import ctypes as C

import numpy as np
import pytest

from indelminer_amd import capi
from tests.support import stepmodel as sm

pytestmark = pytest.mark.gpu

MODES = [pytest.param(dict(wide=True), id="wide"), pytest.param(dict(wide=False, one_launch_flushes=True), id="flush-list")]


class Sets:
    """one context holding one contig per input, and per input a buffer set with its own stream, its bound calls and an event"""

    def __init__(self, inputs, mode, also=()):
        """also: further inputs that will be loaded into the set of the same contig -- its buffers are sized for the largest"""
        self.ctx = capi.Context(0)
        self.sets = []
        try:
            self.ctx.set_reference([inp.contig for inp in inputs])
            self.ctx.set_insert_ranges(sm.RG_NAMES, sm.RG_RANGE)
            self.ctx.expect_read_length(300)            # the long-read kernel follows every set's realign launch
            self.ctx.depth_enable()
            for inp in inputs:
                same = [inp] + [x for x in also if x.tid == inp.tid]
                pipe = sm.new_pipeline(self.ctx, inp, n_pe=max([len(x.pe_b1) for x in same] + [1]), raw_bytes=max(len(x.raw) for x in same))
                stream = capi.new_stream(self.ctx)
                calls = pipe.bind_async(inp.flushes, stream, depth_tid=inp.tid, **mode)
                self.sets.append({"pipe": pipe, "stream": stream, "calls": calls, "done": capi.Event(self.ctx), "graph": None})
        except BaseException:
            self.close()
            raise

    def capture(self):
        """one graph per set, a chain on the set's own stream (as bench.PipeStep.capture)"""
        L = capi.lib()
        for cur in self.sets:
            self.ctx._check(L.im_capture_begin(self.ctx.h, cur["stream"]))
            rc = 0
            for fn, args in cur["calls"]:
                rc = rc or fn(*args)
            g = C.c_void_p()
            rc2 = L.im_capture_end(self.ctx.h, cur["stream"], C.byref(g))
            self.ctx._check(rc)
            self.ctx._check(rc2)
            cur["graph"] = g.value

    def replay(self, cur, wait=True):
        """the set's graph once more: the host waits for the set's previous use, nothing else (as bench.PipeStep.step)"""
        if wait:
            cur["done"].sync()
        self.ctx._check(capi.lib().im_graph_launch(cur["graph"], cur["stream"]))
        cur["done"].record(cur["stream"])

    def sync(self):
        for cur in self.sets:
            self.ctx._check(capi.lib().im_stream_sync(self.ctx.h, cur["stream"]))

    def close(self):
        L = capi.lib()
        if self.ctx.h:
            for cur in self.sets:
                L.im_stream_sync(self.ctx.h, cur["stream"])
                if cur["graph"]:
                    L.im_graph_destroy(cur["graph"])
                cur["done"].close()
                L.im_stream_destroy(self.ctx.h, cur["stream"])
        self.ctx.close()


@pytest.mark.parametrize("mode", MODES)
def test_interleaved_calls_match_the_oracle(mode):
    """Call j of every set is issued before call j + 1 of any, four sets on four streams, nothing synchronised in between.  Catches
    state of the context or of a kernel family that one set's launch leaves for the next launch of the SAME stream but that another
    stream's launch of the same kind overwrites in between: the group-by and flush-group layouts, the expected read length, the
    triage group counters, the sums runs of the depth scan -- any of them shows as a wrong candidate list, evidence, mark, cluster or
    depth of some set."""
    four = sm.four_sets()
    s = Sets([inp for inp, _ in four], mode)
    try:
        n_calls = len(s.sets[0]["calls"])
        assert all(len(cur["calls"]) == n_calls for cur in s.sets)
        for j in range(n_calls):
            for cur in s.sets:
                fn, args = cur["calls"][j]
                s.ctx._check(fn(*args))
        s.sync()
        for cur, (_, model) in zip(s.sets, four):
            sm.check(cur["pipe"], model)
    finally:
        s.close()


@pytest.mark.parametrize("mode", MODES)
def test_graphs_replayed_back_to_back(mode):
    """One graph per set, replayed three rounds over the four sets; the only wait is each set's event before that set's reuse.  Catches
    a pass that is right once but leaves its scratch, tree, table or counters unfit for the next pass over the same buffers when other
    sets' passes run beside it -- and, with each graph replayed once more alone, scratch that only LOOKED clean because a neighbour's
    pass happened to follow."""
    four = sm.four_sets()
    s = Sets([inp for inp, _ in four], mode)
    try:
        s.capture()
        for r in range(3):
            for cur in s.sets:
                s.replay(cur, wait=r > 0)
        s.sync()
        for cur, (_, model) in zip(s.sets, four):
            sm.check(cur["pipe"], model)
        for cur, (_, model) in zip(s.sets, four):
            s.replay(cur)
            s.ctx._check(capi.lib().im_stream_sync(s.ctx.h, cur["stream"]))
            sm.check(cur["pipe"], model)
    finally:
        s.close()


@pytest.mark.parametrize("mode", MODES)
def test_a_replayed_graph_over_new_records(mode):
    """A graph captured over a busy record set (455 candidates) is replayed over a quiet one of the same record count (41 candidates)
    uploaded into the same buffers, then busy again, then quiet, while a second set replays its own graph on another stream
    throughout.  Catches a replay that takes its candidate count from the capture instead of the device; a smaller pass that leaves a
    cluster, a mark or a depth of the larger one behind (tests/test_overlapped_host.py: busy's slots beyond quiet's hold consumed
    evidence, so a leak shows, and handing check() the other input's model fails); and an im_depth_reset inside the graph that does
    not zero the run."""
    (busy, busy_model), (quiet, quiet_model) = sm.busy_and_quiet()
    other, other_model = sm.four_sets()[1]
    assert other.tid == 1 and quiet.rd.n == busy.rd.n and len(quiet.flushes) == len(busy.flushes)      # the counts the capture bakes in
    s = Sets([busy, other], mode, also=[quiet])             # the record buffer and the paired-read region hold the larger of the two
    try:
        a, b = s.sets
        pipe = a["pipe"]
        s.capture()
        first = True
        for inp, model in ((busy, busy_model), (quiet, quiet_model), (busy, busy_model), (quiet, quiet_model)):
            sm.load(pipe, inp)                              # records, offsets, paired-read entries ...
            pipe.d_desc.upload(pipe.flush_descs(inp.flushes))           # ... and flush descriptors, into the captured buffers
            s.replay(b, wait=not first)
            s.replay(a, wait=not first)
            s.replay(b)
            s.ctx._check(capi.lib().im_stream_sync(s.ctx.h, a["stream"]))
            sm.check(pipe, model)
            first = False
        s.sync()
        sm.check(b["pipe"], other_model)
    finally:
        s.close()


# ------------------------------------------------------------------------------------------ the scatters

SCATTERS = ("span_scatter", "pairspan_scatter", "clip_scatter", "cliptail_scatter", "pairlink_scatter")


def _scatter_answers(ctx, inp):
    """every answer of the five structures after the scatters, each compared with the CPU restatements over all chunks' records"""
    from tests.support import cliptails as ct, crossedpiles as cp, facingpiles as fp, pairlinks as pk, spanarrays
    from tests.support.clipcounts import LEFT, RIGHT
    span, pspan, R, L, table, links, _ = inp["models"]
    clens, par = inp["clens"], sm.SCATTER
    out = []
    for tid, clen in enumerate(clens):
        ctx.span_scan(tid); ctx.pairspan_scan(tid)
    ctx._check(capi.lib().im_stream_sync(ctx.h, ctx.stream))
    rng = np.random.default_rng(9)
    for tid, clen in enumerate(clens):
        beg, end = spanarrays.interval_queries(rng, clen)
        p = np.arange(clen + 1, dtype=np.int32)
        beg, end = np.concatenate([beg, p]), np.concatenate([end, p])          # the intervals, then every position by itself
        for query, want in ((ctx.span_query_tid, span), (ctx.pairspan_query_tid, pspan)):
            got = query(tid, beg, end).astype(np.int64)
            assert np.array_equal(got, spanarrays.interval_minima(want[tid], beg, end, clen)), (tid, query.__name__)
            out.append(got)
        for side, want in ((RIGHT, R), (LEFT, L)):
            cnt, _ = ctx.clip_query_tid(tid, np.full(clen + 1, side, np.uint8), p, p)
            assert np.array_equal(cnt.astype(np.int64), want[tid]), (tid, side, np.nonzero(cnt.astype(np.int64) != want[tid])[0][:10])
            out.append(cnt)
    n_tails = sum(len(v) for v in table.values())
    assert ctx.cliptail_stats() == (n_tails, 0) and ctx.pairlink_stats() == (len(links), 0)
    for tid, clen in enumerate(clens):
        peaks = {side: [p for p, _ in cp.peaks_many(A[tid], 3, 30)] for side, A in ((RIGHT, R), (LEFT, L))}
        assert len(peaks[RIGHT]) >= 9 and len(peaks[LEFT]) >= 9
        pr = [a for a in peaks[RIGHT] for _ in peaks[LEFT]]
        pl = [b for _ in peaks[RIGHT] for b in peaks[LEFT]]
        got = [tuple(int(x) for x in row) for row in zip(*ctx.cliptail_verify(tid, pr, pl, 32))]
        assert got == ct.answer_many(table, inp["contigs"][tid], tid, pr, pl, 32), tid
        out.append(got)
        keys = [(side, p) for side in (RIGHT, LEFT) for p in peaks[side]]
        got = [tuple(int(x) for x in row) for row in zip(*ctx.cliptail_consensus(tid, [p for _, p in keys], [s for s, _ in keys], par["min_cover"]))]
        assert got == [fp.answer(table, tid, p, side, par["min_cover"], clen) for side, p in keys], tid
        assert any(g[1] > 0 for g in got)
        out.append(got)
        # the crossed piles read both arrays and the table's bases at once
        got = [tuple(int(x) for x in row) for row in zip(*ctx.clip_crossed_tid(tid, *sm.CROSSED_PAR))]
        want = cp.crossed(R[tid], L[tid], table, inp["contigs"][tid], tid, *sm.CROSSED_PAR)[0]
        assert got == want and len(want) >= 9, (tid, len(got), len(want))
        out.append(got)
        windows = [pk.window_of("DUP", None, a, a + n) for a, n in cp.SITES] + [(k, -5, clen + 5, -5, clen + 5) for k in range(3)]
        for sep in (0, pk.MIN_SEP):
            got = [int(x) for x in ctx.pairlink_count(tid, *[[w[k] for w in windows] for k in range(5)], sep)]
            assert got == [pk.count(links, clens, tid, *w, sep) for w in windows], (tid, sep)
            assert sum(got) > 0
            out.append(got)
    return [x.tobytes() if isinstance(x, np.ndarray) else x for x in out]


def test_scatters_from_four_streams():
    """One record set (reference-spanning reads, concordant pairs, right and left clips with their clipped bases, everted pairs) cut
    into four chunks at records that are no multiple of 64; every chunk's five scatters go to a stream of the chunk's own, interleaved
    across the streams call by call, into ONE set of genome-wide arrays and keyed tables.  Catches a lost update in the counted arrays
    (an add that is not atomic), a slot of a keyed table claimed twice or an entry written over while its key is being claimed from
    another stream, and a stored / dropped counter that misses an entry: tests/test_overlapped_host.py shows that every chunk holds
    every kind and that dropping any chunk changes every model.  Then the same chunks on one stream, in order, after the resets: the
    answers must be the same bytes."""
    inp = sm.scatter_input()
    par = sm.SCATTER
    ctx = capi.Context(0)
    keep, streams = [], []
    try:
        ctx.set_reference(inp["contigs"])
        ctx.set_insert_ranges(["generic"], [inp["range_max"]])
        ctx.span_enable(par["m"], par["q"]); ctx.pairspan_enable(par["m"], par["q"])
        ctx.clip_enable(par["c"], par["q"]); ctx.cliptail_enable(par["c"], par["q"], par["log2_slots"]); ctx.pairlink_enable(par["q"], par["log2_slots"])
        recs = []
        for raw, off in inp["chunks"]:
            d_raw = capi.DevBuf(ctx, len(raw) + 64).upload(raw)
            d_off = capi.DevBuf(ctx, 4 * len(off)).upload(off)
            keep += [d_raw, d_off]
            recs.append(capi.DevRecords(len(off) - 1, d_raw.ptr, d_off.ptr, 0))
            streams.append(capi.new_stream(ctx))
        ctx._check(capi.lib().im_stream_sync(ctx.h, ctx.stream))        # the enables' fills are done before another stream scatters
        for name in SCATTERS:
            for r, st in zip(recs, streams):
                getattr(ctx, name)(r, st)
        for st in streams:
            ctx._check(capi.lib().im_stream_sync(ctx.h, st))
        overlapped = _scatter_answers(ctx, inp)
        # reset everything, then one stream, chunk after chunk
        for tid in range(len(inp["clens"])):
            ctx.span_reset(tid); ctx.pairspan_reset(tid); ctx.clip_reset(tid)
        ctx.cliptail_reset(); ctx.pairlink_reset()
        for r in recs:
            for name in SCATTERS:
                getattr(ctx, name)(r)
        ctx._check(capi.lib().im_stream_sync(ctx.h, ctx.stream))
        assert _scatter_answers(ctx, inp) == overlapped
    finally:
        if ctx.h:
            for st in streams:
                capi.lib().im_stream_sync(ctx.h, st)
                capi.lib().im_stream_destroy(ctx.h, st)
            for b in keep:
                b.free()
        ctx.close()
