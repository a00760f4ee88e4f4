"""The classify kernel in one-wave workgroups (im_triage.hip), every output compared exactly with the CPU oracle: record counts
around the 64-record workgroup and the group of 32 workgroups, counts that take the scan of the groups' totals through its second
round and its second fetch, the chunk-after-chunk form cut at 1, 63, 64 and 65 records, the 1024-position depth window with the
first eligible record in lane 0, 1 and 63, the reset of a contig's run (whole 16-byte stores, a tail, a run shorter than 16 bytes),
and read-group tables on both sides of the LDS copy's limit.  The inputs come from tests/support/wavecases.py;
tests/test_triage_wave_host.py proves on the CPU that they reach what they name.

Not here: the doubling of the group size (beyond 2048 groups of 32 workgroups: over 4 million records).  tests/test_gpu_large.py
runs triage at scale."""
import numpy as np
import pytest

from indelminer_amd import capi
from tests.support import oraclebind as ob
from tests.support import triagecases as tc
from tests.support import wavecases as wc
from tests.test_gpu_triage import _compare_triage

pytestmark = pytest.mark.gpu

REF = [b"ACGT" * 500]
E = capi.MAX_EV


@pytest.fixture(scope="module")
def tiles():
    """the small records of triagecases section 5 and what the oracle says of each, once"""
    tpl = tc.tile_templates()
    keys = ["cand", "counted", "skip", "err"]
    flat = [r for k in keys for r in tpl[k]]
    first = np.cumsum([0] + [len(tpl[k]) for k in keys])[:4]
    raw, off = tc.batch(flat)
    tri = ob.triage_records(raw, off, ["generic"], [700], eth_vcf=0)
    T = dict(cls=np.array([t.cls for t, _ in tri], np.uint8), want=np.array([t.want != 0 for t, _ in tri]),
             len=np.array([t.l_seq for t, _ in tri], np.int32), tid=np.array([t.tid for t, _ in tri], np.int32),
             anchor=np.array([t.anchor for t, _ in tri], np.int32), range=np.array([t.range_max for t, _ in tri], np.int32),
             bases=[(b or b"") + bytes((-len(b or b"")) % 4) for _, b in tri],
             ev=np.array([[(t.ev_cls[k], t.ev_b1[k], t.ev_b2[k]) if k < t.n_ev else (-1, 0, 0) for k in range(E)] for t, _ in tri], np.int32),
             rec_len=np.array([len(r) for r in flat], np.int64))
    return tpl, flat, first, T


def _batch_of(flat, T, tmpl):
    """tc.batch for a template index per record, without a Python loop over the records"""
    lens = T["rec_len"][tmpl]
    off = np.zeros(len(tmpl) + 1, np.uint32)
    np.cumsum(lens, out=off[1:])
    width = int(T["rec_len"].max())
    table = np.zeros((len(flat), width), np.uint8)
    for k, r in enumerate(flat):
        table[k, :len(r)] = np.frombuffer(r, np.uint8)
    rows = table[tmpl]
    keep = np.arange(width)[None, :] < lens[:, None]
    return rows[keep], off


def _check_tiles(pipe, tiles, name, n):
    tpl, flat, first, T = tiles
    role, sub = wc.tile_pattern(name, n, tpl)
    tmpl = first[role] + sub
    raw, off = _batch_of(flat, T, tmpl)
    assert len(raw) <= 64 * n
    pipe.upload(raw, off)
    pipe.triage()
    c = pipe.fetch_counts()
    cls = T["cls"][tmpl]
    cand = np.nonzero(T["want"][tmpl])[0]
    m = len(cand)
    lens = T["len"][tmpl[cand]]
    pad = (lens + 3) // 4 * 4
    print(name, n, c[:5], m)
    assert list(c[:5]) == [m, int(pad.sum()), int((cls != 0).sum()), int((cls >= 16).sum()), 0], (name, c[:5])
    assert np.array_equal(pipe.d_class.download(np.uint8, n), cls), name
    if m == 0:
        return
    assert np.array_equal(pipe.d_cand_rec.download(np.int32, m), cand.astype(np.int32)), name
    assert np.array_equal(pipe.d_boff.download(np.int64, m), np.cumsum(pad) - pad), name
    assert np.array_equal(pipe.d_len.download(np.int32, m), lens), name
    width = max(len(b) for b in T["bases"])
    bt = np.zeros((len(flat), width), np.uint8)
    for k, b in enumerate(T["bases"]):
        bt[k, :len(b)] = np.frombuffer(b, np.uint8)
    want_bases = bt[tmpl[cand]][np.arange(width)[None, :] < pad[:, None]]
    assert np.array_equal(pipe.d_bases.download(np.uint8, int(pad.sum())), want_bases), name
    assert np.array_equal(pipe.d_tid.download(np.int32, m), T["tid"][tmpl[cand]]), name
    assert np.array_equal(pipe.d_anchor.download(np.int32, m), T["anchor"][tmpl[cand]]), name
    assert np.array_equal(pipe.d_range.download(np.int32, m), T["range"][tmpl[cand]]), name
    ev = T["ev"][tmpl[cand]].reshape(m * E, 3)
    for buf, col in ((pipe.d_cls, 0), (pipe.d_b1, 1), (pipe.d_b2, 2)):
        assert np.array_equal(buf.download(np.int32, m * E), ev[:, col]), (name, col)


def test_batch_of_builds_what_tc_batch_builds(tiles):
    tpl, flat, first, T = tiles
    tmpl = np.array([3, 0, len(flat) - 1, 7, 7, 1])
    raw, off = _batch_of(flat, T, tmpl)
    raw2, off2 = tc.batch([flat[k] for k in tmpl])
    assert np.array_equal(raw, raw2) and np.array_equal(off, off2)


@pytest.mark.parametrize("n", wc.TILE_COUNTS)
def test_counts_around_the_workgroup_and_the_group(gpu_ctx, tiles, n):
    """patterns that put 0, 1 and 64 candidates, counted records and error records into a workgroup's packed totals"""
    gpu_ctx.set_reference(REF)
    gpu_ctx.set_insert_ranges(["generic"], [700])
    pipe = capi.Pipeline(gpu_ctx, n, 64 * n + 64, cap_cand=n, read_len_max=12, ethreshold_vcfcheck=0)
    for name in wc.TILE_PATTERNS:
        _check_tiles(pipe, tiles, name, n)


@pytest.mark.parametrize("n", wc.SCAN_COUNTS)
def test_scan_of_the_groups_second_round_and_second_fetch(gpu_ctx, tiles, n):
    """65 and 513 groups: the scanning wave takes 64 a round and fetches eight rounds' totals together"""
    assert -(-n // wc.GROUP_RECORDS) in (wc.SCAN_LANES + 1, wc.SCAN_AHEAD * wc.SCAN_LANES + 1)
    gpu_ctx.set_reference(REF)
    gpu_ctx.set_insert_ranges(["generic"], [700])
    pipe = capi.Pipeline(gpu_ctx, n, 64 * n + 64, cap_cand=n, read_len_max=12, ethreshold_vcfcheck=0)
    _check_tiles(pipe, tiles, "mix", n)


def _outputs(pipe, m, nbytes):
    return dict(cand_rec=pipe.d_cand_rec.download(np.int32, m), boff=pipe.d_boff.download(np.int64, m), len=pipe.d_len.download(np.int32, m),
                bases=pipe.d_bases.download(np.uint8, nbytes), tid=pipe.d_tid.download(np.int32, m), anchor=pipe.d_anchor.download(np.int32, m),
                range=pipe.d_range.download(np.int32, m), cls=pipe.d_cls.download(np.int32, m * E), b1=pipe.d_b1.download(np.int32, m * E),
                b2=pipe.d_b2.download(np.int32, m * E))


def _run_chunks(pipe, raw, off, bounds):
    out = []
    for k in range(len(bounds) - 1):
        a, b = int(bounds[k]), int(bounds[k + 1])
        pipe.upload(raw[int(off[a]):int(off[b])], (off[a:b + 1] - off[a]).astype(np.uint32))
        pipe.triage_append(b - a, a, restart=k == 0, clear=False)
        pipe.sync()                                     # before the next chunk overwrites the record buffer
        out.append(pipe.d_class.download(np.uint8, b - a))
    return out


def test_chunks_cut_at_the_workgroup_append_to_one_candidate_set(gpu_ctx):
    """chunk after chunk with rec_base, restart and appending counters, chunks of 1, 63, 64 and 65 records, against the same records
    as one chunk (itself against the oracle)"""
    recs = wc.append_batch()
    n = len(recs)
    gpu_ctx.set_reference(REF)
    gpu_ctx.set_insert_ranges(tc.AUX_NAMES, tc.AUX_RANGES)
    raw, off = tc.batch(recs)
    one = capi.Pipeline(gpu_ctx, n, len(raw), cap_cand=n, read_len_max=2600)
    tri, cand = _compare_triage(one, raw, off, tc.AUX_NAMES, tc.AUX_RANGES)
    m = len(cand)
    want_c = one.fetch_counts()
    nbytes = int(want_c[1])
    want = _outputs(one, m, nbytes)
    want_cls = one.d_class.download(np.uint8, n)
    bounds = wc.append_bounds(n)
    pipe = capi.Pipeline(gpu_ctx, max(wc.CHUNK_CUTS), len(raw), cap_cand=n, read_len_max=2600)
    pipe.d_counters.upload(np.full(64, 0x7F, np.uint8))
    got_cls = np.concatenate(_run_chunks(pipe, raw, off, bounds))
    c = pipe.d_counters.download(np.int32, 8)
    assert list(c[:5]) == [m, nbytes, int(want_c[2]), int(want_c[3]), 0], (c, want_c)
    assert np.array_equal(got_cls, want_cls), np.nonzero(got_cls != want_cls)[0][:8]
    got = _outputs(pipe, m, nbytes)
    for key in want:
        assert np.array_equal(got[key], want[key]), (key, np.nonzero(got[key] != want[key])[0][:8])


def test_depth_window_of_a_wave_and_the_reset():
    """the pileup scatter through the workgroup's LDS window and past it, every position of every contig against imo_depth_add --
    and again after im_depth_reset, whose runs are 20 004, 36 004 and 12 bytes long"""
    recs = wc.depth_cases()
    raw, off = tc.batch(recs)
    n = len(recs)
    clens = wc.DEPTH_CONTIGS
    want = [ob.depth_of(raw, off, t, clen).astype(np.int64) for t, clen in enumerate(clens)]
    o_cls = np.array([t.cls for t, _ in ob.triage_records(raw, off, ["generic"], [700])], np.uint8)
    ctx = capi.Context(0)
    try:
        ctx.set_reference([b"A" * clens[0], b"C" * clens[1], b"G" * clens[2]])
        ctx.set_insert_ranges(["generic"], [700])
        ctx.depth_enable()
        pipe = capi.Pipeline(ctx, n, len(raw), cap_cand=n, want_depth=True)

        def check(what):
            for t, clen in enumerate(clens):
                ctx.depth_scan(t)
                p = np.arange(clen, dtype=np.int32)
                got = ctx.depth_query_tid(t, p, p + 1).astype(np.int64)
                bad = np.nonzero(got != want[t])[0]
                assert len(bad) == 0, (what, t, bad[:8], got[bad[:8]], want[t][bad[:8]])
            for t in range(len(clens)):
                ctx._check(capi.lib().im_depth_reset(ctx.h, t, ctx.stream))
        pipe.upload(raw, off)
        pipe.triage()
        pipe.sync()
        assert np.array_equal(pipe.d_class.download(np.uint8, n), o_cls)
        check("one chunk")
        pipe.triage()                                   # im_depth_reset, then the same chunk again
        pipe.sync()
        check("after a reset")
        _run_chunks(pipe, raw, off, [0, wc.DEPTH_CHUNK_CUT, n])     # two chunks on one array, cut inside a workgroup
        check("two chunks")
    finally:
        ctx.close()


@pytest.mark.parametrize("table", [str(wc.RG_LDS), str(wc.RG_LDS + 4)])
def test_read_group_tables_around_the_lds_copy(gpu_ctx, table):
    names, ranges = tc.rg_table(int(table))
    assert tc.table_bytes(names) == int(table)
    recs = [r for r, _ in tc.rg_table_cases(names)]
    gpu_ctx.set_reference(REF)
    gpu_ctx.set_insert_ranges(names, ranges)
    raw, off = tc.batch(recs)
    pipe = capi.Pipeline(gpu_ctx, len(recs), len(raw), cap_cand=len(recs), read_len_max=100)
    tri, cand = _compare_triage(pipe, raw, off, names, ranges)
    assert {3, 16} <= {t.cls for t, _ in tri}
