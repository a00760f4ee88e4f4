"""im_depth_query_max_tid where there is no GPU: the CPU shim's restatement (tests/shim/im_shim.c, what the host-driver tests run the
product's DP= logic against) held to the numpy statement of tests/support/depthmax.py -- the statement the kernel is held to in
tests/test_gpu_depth_max.py -- on the same records and queries."""
import ctypes as C

import numpy as np

from tests.support import depthmax as dm


def test_the_spike_queries_have_teeth():
    raw, off, depth = dm.records()
    assert dm.check_teeth(depth) >= 20
    assert max(int(d.max()) for d in depth) >= dm.DEEP > 8000 and any(4000 <= int(d.max()) < 8000 for d in depth)
    for t in range(len(dm.CLENS)):
        beg, end = dm.queries(t)
        assert len(beg) >= 40 and (beg < end).all()
        s, m = dm.model(depth[t], beg, end)
        assert (m.astype(np.int64) * (np.minimum(end, dm.CLENS[t]) - np.maximum(beg, 0)) >= s).all()
    # the tile-edge spike: beg - 1 is the last position of a tile, beg the first of the next
    assert any(p + dm.BASES == 5 * dm.TILE for t, p, k in dm.SPIKES if t == 0)


def test_shim_matches_the_numpy_statement():
    from indelminer_amd import capi
    from tests.support.shimbuild import build_shim_lib
    L = C.CDLL(build_shim_lib())
    L.im_ctx_create.argtypes = [C.c_int, C.POINTER(C.c_void_p)]
    L.im_set_reference.argtypes = [C.c_void_p, C.c_int32, C.POINTER(C.c_char_p), C.POINTER(C.c_int64)]
    L.im_set_insert_ranges.argtypes = [C.c_void_p, C.c_int32, C.POINTER(C.c_char_p), C.c_void_p]
    L.im_depth_enable.argtypes = [C.c_void_p]
    L.im_depth_scan.argtypes = [C.c_void_p, C.c_int32, C.c_void_p]
    L.im_dev_triage.argtypes = [C.c_void_p, C.POINTER(capi.TriageParams), C.POINTER(capi.DevRecords), C.POINTER(capi.DevCands),
                                C.c_void_p, C.c_size_t, C.c_void_p]
    q_args = [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]
    L.im_depth_query_tid.argtypes = q_args
    L.im_depth_query_max_tid.argtypes = q_args + [C.c_void_p]
    L.im_ctx_destroy.argtypes = [C.c_void_p]
    L.im_ctx_destroy.restype = None

    raw, off, depth = dm.records()
    off = np.ascontiguousarray(off, np.uint32)
    n = len(off) - 1
    h = C.c_void_p()
    assert L.im_ctx_create(0, C.byref(h)) == 0
    try:
        seqs = [b"A" * clen for clen in dm.CLENS]
        assert L.im_set_reference(h, len(seqs), (C.c_char_p * len(seqs))(*seqs), (C.c_int64 * len(seqs))(*dm.CLENS)) == 0
        rm = np.array([700], np.int32)
        assert L.im_set_insert_ranges(h, 1, (C.c_char_p * 1)(b"generic"), rm.ctypes.data) == 0
        assert L.im_depth_enable(h) == 0
        # no record is a candidate (unpaired reads); the buffers a candidate would go to are there all the same
        buf = {k: np.zeros(64, np.int64) for k in ("bases", "off", "len", "tid", "anchor", "range", "cls", "b1", "b2", "cand_rec")}
        counters = np.zeros(16, np.int32)
        rec_class = np.zeros(n, np.uint8)
        p = {k: v.ctypes.data for k, v in buf.items()}
        batch = capi.DevBatch(0, p["bases"], p["off"], p["len"], p["tid"], p["anchor"], p["range"], None, p["cls"], p["b1"], p["b2"])
        cands = capi.DevCands(batch, p["cand_rec"], counters.ctypes.data, rec_class.ctypes.data, 4, 256, None)
        recs = capi.DevRecords(n, raw.ctypes.data, off.ctypes.data, 0)
        tp = capi.TriageParams(10, 10, 1000000, 1, 0, 1)
        assert L.im_dev_triage(h, C.byref(tp), C.byref(recs), C.byref(cands), None, 0, None) == 0
        assert counters[0] == 0 and counters[4] == 0
        for t, clen in enumerate(dm.CLENS):
            assert L.im_depth_scan(h, t, None) == 0
            beg, end = dm.queries(t)
            want_sum, want_max = dm.model(depth[t], beg, end)
            got_sum, got_max, plain = (np.zeros(len(beg), np.uint32) for _ in range(3))
            assert L.im_depth_query_max_tid(h, t, len(beg), beg.ctypes.data, end.ctypes.data, got_sum.ctypes.data, got_max.ctypes.data) == 0
            assert L.im_depth_query_tid(h, t, len(beg), beg.ctypes.data, end.ctypes.data, plain.ctypes.data) == 0
            bad = np.nonzero((got_sum != want_sum) | (got_max != want_max))[0]
            assert len(bad) == 0, (t, [(int(beg[i]), int(end[i]), int(got_sum[i]), int(want_sum[i]), int(got_max[i]), int(want_max[i])) for i in bad[:6]])
            assert np.array_equal(plain, want_sum)
            # the windows drawn out to the front, as the driver sends them beside the plain ones
            beg, end = dm.lookback_queries(t)
            want_sum, want_max = dm.model(depth[t], beg, end)
            got_sum, got_max = (np.zeros(len(beg), np.uint32) for _ in range(2))
            assert L.im_depth_query_max_tid(h, t, len(beg), beg.ctypes.data, end.ctypes.data, got_sum.ctypes.data, got_max.ctypes.data) == 0
            assert np.array_equal(got_sum, want_sum) and np.array_equal(got_max, want_max), t
        # im_depth_query_max: the same statement on what im_depth_build left (the record-at-a-time path), each contig in turn
        L.im_depth_build.argtypes = [C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.c_void_p]
        L.im_depth_query.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]
        L.im_depth_query_max.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        for t, (clen, pos) in enumerate(zip(dm.CLENS, dm.positions())):
            start, length = pos.astype(np.int32), np.full(len(pos), dm.BASES, np.int32)
            assert L.im_depth_build(h, clen, len(start), start.ctypes.data, length.ctypes.data) == 0
            beg, end = (np.concatenate(x) for x in zip(dm.queries(t), dm.lookback_queries(t)))
            want_sum, want_max = dm.model(depth[t], beg, end)
            got_sum, got_max, plain = (np.zeros(len(beg), np.uint32) for _ in range(3))
            assert L.im_depth_query_max(h, len(beg), beg.ctypes.data, end.ctypes.data, got_sum.ctypes.data, got_max.ctypes.data) == 0
            assert L.im_depth_query(h, len(beg), beg.ctypes.data, end.ctypes.data, plain.ctypes.data) == 0
            assert np.array_equal(got_sum, want_sum) and np.array_equal(got_max, want_max) and np.array_equal(plain, want_sum), t
    finally:
        L.im_ctx_destroy(h)
