"""The triage's scan launch (triage_scan_kernel in im_triage.hip) between classify and emit, through capi.Pipeline and the public
entries only, exact against the CPU oracle: record counts around every edge of the launch, patterns that put known totals into the
classify workgroups' words, chunk after chunk on running counters, a scratch buffer reused by a smaller launch, both overflows, and
the four launches captured into a graph.  The counts come from tests/support/scancases.py, derived from the constants the kernels are
built with: a lane of the scan takes a group of 32 classify workgroups (8 emit workgroups) a pass, the workgroup has 256 lanes in 4
waves, so

    1, 255, 256, 257                one emit workgroup and its base entry, and the second
    2047, 2048, 2049                a group of 32 classify workgroups: the scan's first lane, and its second
    131 071, 131 072, 131 073       64 groups: the scan's first wave, and its second (the waves' totals go through LDS)
    524 224, 524 288, 524 289       8 191, 8 192 and 8 193 classify workgroups: a pass of the scan less one word, whole, and the
                                    first launch that takes a second pass (and fetches a second time)

tests/test_triage_scan_host.py proves on the CPU that these are what they claim."""
import ctypes as C

import numpy as np
import pytest

from indelminer_amd import capi
from tests.support import oraclebind as ob
from tests.support import scancases as sc
from tests.support import triagecases as tc
from tests.support import wavecases as wc
from tests.test_gpu_triage_wave import _batch_of, tiles  # noqa: F401  (tiles: the templates and what the oracle says of each, once)

pytestmark = pytest.mark.gpu

REF = [b"ACGT" * 500]


def _expect(tiles, name, n):
    """the records of a pattern and, from the oracle's verdict on each template, what the triage must leave"""
    tpl, flat, first, T = tiles
    role, sub = sc.pattern(name, n, tpl)
    tmpl = first[role] + sub
    raw, off = _batch_of(flat, T, tmpl)
    cls = T["cls"][tmpl]
    cand = np.nonzero(T["want"][tmpl])[0].astype(np.int32)
    lens = T["len"][tmpl[cand]]
    pad = (lens + 3) // 4 * 4
    return dict(raw=raw, off=off, cls=cls, cand=cand, len=lens, pad=pad, boff=(np.cumsum(pad) - pad).astype(np.int64),
                counters=[len(cand), int(pad.sum()), int((cls != 0).sum()), int((cls >= 16).sum()), 0])


def _compare(pipe, want, what, n=None, accepted=None, counters=None):
    c = pipe.fetch_counts()
    assert list(c[:5]) == (counters or want["counters"]), (what, list(c[:5]), counters or want["counters"])
    assert np.array_equal(pipe.d_class.download(np.uint8, n or len(want["cls"])), want["cls"]), what
    m = len(want["cand"]) if accepted is None else accepted
    if m:
        assert np.array_equal(pipe.d_cand_rec.download(np.int32, m), want["cand"][:m]), what
        assert np.array_equal(pipe.d_boff.download(np.int64, m), want["boff"][:m]), what
        assert np.array_equal(pipe.d_len.download(np.int32, m), want["len"][:m]), what


def _pipeline(gpu_ctx, n, cap_cand=None):
    gpu_ctx.set_reference(REF)
    gpu_ctx.set_insert_ranges(["generic"], [700])
    return capi.Pipeline(gpu_ctx, n, 64 * n + 64, cap_cand=max(cap_cand if cap_cand is not None else n, 1), read_len_max=12, ethreshold_vcfcheck=0)


@pytest.mark.parametrize("n", sc.COUNTS)
def test_counts_around_every_edge_of_the_scan(gpu_ctx, tiles, n):
    pipe = _pipeline(gpu_ctx, n)
    for name in sc.PATTERNS:
        want = _expect(tiles, name, n)
        pipe.upload(want["raw"], want["off"])
        pipe.triage()
        _compare(pipe, want, (name, n))


def _oracle(recs, names, ranges):
    raw, off = tc.batch(recs)
    tri = ob.triage_records(raw, off, names, ranges)
    cls = np.array([t.cls for t, _ in tri], np.uint8)
    cand = np.array([k for k, (t, _) in enumerate(tri) if t.want], np.int32)
    lens = np.array([tri[k][0].l_seq for k in cand], np.int32)
    pad = (lens + 3) // 4 * 4
    return raw, off, dict(cls=cls, cand=cand, len=lens, pad=pad, boff=(np.cumsum(pad) - pad).astype(np.int64),
                          counters=[len(cand), int(pad.sum()), int((cls != 0).sum()), int((cls >= 16).sum()), 0])


def test_three_chunks_append_behind_poisoned_counters(gpu_ctx):
    """chunks of 1, 63 and 65 records, restart on the first only, the counters holding 0x7F bytes before it"""
    recs = wc.append_batch(sum(sc.CHUNKS))
    raw, off, want = _oracle(recs, tc.AUX_NAMES, tc.AUX_RANGES)
    n = len(recs)
    gpu_ctx.set_reference(REF)
    gpu_ctx.set_insert_ranges(tc.AUX_NAMES, tc.AUX_RANGES)
    pipe = capi.Pipeline(gpu_ctx, max(sc.CHUNKS), len(raw), cap_cand=n, read_len_max=2600)
    pipe.d_counters.upload(np.full(64, 0x7F, np.uint8))
    bounds = np.cumsum([0] + sc.CHUNKS)
    got_cls = []
    for k, (a, b) in enumerate(zip(bounds[:-1], bounds[1:])):
        a, b = int(a), int(b)
        pipe.upload(raw[int(off[a]):int(off[b])], (off[a:b + 1] - off[a]).astype(np.uint32))
        pipe.triage_append(b - a, a, restart=k == 0)
        pipe.sync()                                     # before the next chunk overwrites the record buffer
        got_cls.append(pipe.d_class.download(np.uint8, b - a))
    assert np.array_equal(np.concatenate(got_cls), want["cls"])
    want = dict(want, cls=got_cls[-1])                  # the class buffer holds the last chunk's
    _compare(pipe, want, "chunks", n=sc.CHUNKS[-1])


def test_a_smaller_launch_on_the_scratch_of_a_larger_one(gpu_ctx, tiles):
    """no im_dev_triage_scratch_init in between: what the larger launch left behind the smaller one's count is not read"""
    pipe = _pipeline(gpu_ctx, sc.REUSE_LARGE)
    large = _expect(tiles, "all", sc.REUSE_LARGE)
    pipe.upload(large["raw"], large["off"])
    pipe.triage()
    _compare(pipe, large, "large")
    for name in ("last_block", "lane63"):
        small = _expect(tiles, name, sc.REUSE_SMALL)
        pipe.upload(small["raw"], small["off"])
        pipe.d_counters.upload(np.full(64, 0x7F, np.uint8))
        pipe.triage_append(sc.REUSE_SMALL, 0, restart=True)
        _compare(pipe, small, ("small", name), n=sc.REUSE_SMALL)


@pytest.mark.parametrize("short", ["cap_cand", "cap_bases"])
def test_overflow_keeps_the_accepted_prefix(gpu_ctx, tiles, short):
    """one candidate too many, one byte too few: counters[0..1] count every candidate, counters[4] the refused one, and the
    candidates in front of it are whole (include/indelminer_amd.h, im_dev_cands)"""
    n = sc.EMIT + 1
    want = _expect(tiles, "all", n)
    m = len(want["cand"])
    if short == "cap_cand":
        pipe = _pipeline(gpu_ctx, n, cap_cand=m - 1)
    else:
        pipe = _pipeline(gpu_ctx, n)
        pipe.cap_bases = int(want["pad"].sum()) + 16 - 1
        pipe.cands = capi.DevCands(pipe.batch, pipe.d_cand_rec.ptr, pipe.d_counters.ptr, pipe.d_class.ptr, pipe.cap_cand, pipe.cap_bases, None)
    pipe.upload(want["raw"], want["off"])
    pipe.triage()
    _compare(pipe, want, short, accepted=m - 1, counters=want["counters"][:4] + [1])
    if short == "cap_bases":                            # refused for its bytes below cap_cand: length 0 and offset 0
        assert int(pipe.d_len.download(np.int32, m)[m - 1]) == 0 and int(pipe.d_boff.download(np.int64, m)[m - 1]) == 0


def test_the_four_launches_captured_into_a_graph(gpu_ctx, tiles):
    """im_dev_triage captured on a second stream and replayed three times leaves what the call-by-call pass leaves"""
    n = sc.GROUP_RECORDS + 1
    want = _expect(tiles, "lane63", n)
    pipe = _pipeline(gpu_ctx, n)
    pipe.upload(want["raw"], want["off"])
    pipe.triage()
    _compare(pipe, want, "call by call")
    m = len(want["cand"])
    direct = [pipe.d_cand_rec.download(np.int32, m), pipe.d_boff.download(np.int64, m), pipe.d_len.download(np.int32, m),
              pipe.d_bases.download(np.uint8, want["counters"][1]), pipe.d_class.download(np.uint8, n)]
    L = capi.lib()
    stream = capi.new_stream(gpu_ctx)
    graph = C.c_void_p()
    try:
        gpu_ctx._check(L.im_capture_begin(gpu_ctx.h, stream))
        try:
            pipe.triage_append(n, 0, restart=True, stream=stream)
        finally:
            rc = L.im_capture_end(gpu_ctx.h, stream, C.byref(graph))
        gpu_ctx._check(rc)
        for buf, nbytes in ((pipe.d_cand_rec, 4 * m), (pipe.d_boff, 8 * m), (pipe.d_len, 4 * m), (pipe.d_class, n)):
            buf.upload(np.full(nbytes, 0x7F, np.uint8))
        pipe.d_counters.upload(np.full(64, 0x7F, np.uint8))
        pipe.sync()
        for _ in range(3):
            gpu_ctx._check(L.im_graph_launch(graph.value, stream))
        gpu_ctx._check(L.im_stream_sync(gpu_ctx.h, stream))
        _compare(pipe, want, "replayed")
        replayed = [pipe.d_cand_rec.download(np.int32, m), pipe.d_boff.download(np.int64, m), pipe.d_len.download(np.int32, m),
                    pipe.d_bases.download(np.uint8, want["counters"][1]), pipe.d_class.download(np.uint8, n)]
        for a, b in zip(direct, replayed):
            assert np.array_equal(a, b)
    finally:
        L.im_stream_sync(gpu_ctx.h, stream)
        if graph.value:
            L.im_graph_destroy(graph.value)
        L.im_stream_destroy(gpu_ctx.h, stream)
