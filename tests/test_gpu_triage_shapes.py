"""The triage kernels (im_triage.hip: classify, emit, decode) at the edges of their index arithmetic, every output compared exactly
with the CPU oracle (imo_triage_record, imo_depth_add): read lengths around the four / eight lanes per record switch and the
tail loop behind 256 bases, refused base codes at every piece boundary against refused ops, aux areas that make the 24-byte
window slide, read-group tables on both sides of the LDS limit, record counts around the workgroup and the group of 32
workgroups, the chunk-after-chunk form the product issues (rec_base, restart, appending counters), the 4096-position depth
window, and candidates that do not fit the batch.  The inputs come from tests/support/triagecases.py;
tests/test_triage_cases_host.py proves on the CPU that they reach what they name.

Not here, because they need inputs no test of seconds can hold: the second round of the scan of the groups' totals (more than
256 groups: over 2.1 million records) and the doubling of the group size (beyond 2048 groups of 32 workgroups: over 16 million
records).  tests/test_gpu_large.py runs triage at that scale."""
import numpy as np
import pytest

from indelminer_amd import capi
from tests.support import oraclebind as ob
from tests.support import triagecases as tc
from tests.test_gpu_triage import _compare_triage, _rec

pytestmark = pytest.mark.gpu

REF = [b"ACGT" * 500]


def _pipe_for(ctx, recs, read_len_max, **kw):
    raw, off = tc.batch(recs)
    return capi.Pipeline(ctx, len(recs), len(raw), cap_cand=len(recs), read_len_max=read_len_max, **kw), raw, off


def test_generator_builds_records_the_way_rec_does():
    for kw in (dict(), dict(cigar=tc.CLIP, tags=b"RGZlib1\0", qname=b"qq\0"), dict(l_seq=33, seq=bytes([0x48] * 17), cigar=((33, 0),), pad=b"MQ")):
        assert tc.rec(tc.P, **kw) == _rec(tc.P, **kw)


def test_read_length_edges(gpu_ctx):
    """every length of triagecases.LENGTHS forward and reverse-complemented, in waves whose lanes-per-record ballots differ"""
    recs, waves = tc.length_layout(tc.length_cases())
    gpu_ctx.set_reference(REF)
    gpu_ctx.set_insert_ranges(["generic"], [700])
    pipe, raw, off = _pipe_for(gpu_ctx, recs, 2600)
    tri, cand = _compare_triage(pipe, raw, off, ["generic"], [700])
    assert {t.cls for t, _ in tri} == {1, 2, 3} and len(cand) > 400
    assert {t.l_seq for t, _ in tri if t.cls == 2} == set(tc.LENGTHS)


def test_first_refused_base_against_first_refused_op(gpu_ctx):
    recs = tc.base_layout(tc.base_cases())
    gpu_ctx.set_reference(REF)
    gpu_ctx.set_insert_ranges(["generic"], [700])
    pipe, raw, off = _pipe_for(gpu_ctx, recs, 600)
    tri, cand = _compare_triage(pipe, raw, off, ["generic"], [700])
    assert {t.cls for t, _ in tri} >= {1, 3, 18, 20}


@pytest.mark.parametrize("which", ["prefixes_and_mq", "rg_names"])
def test_aux_walk(gpu_ctx, which):
    if which == "prefixes_and_mq":
        recs, names, ranges = tc.aux_layout(tc.aux_cases() + tc.mq_cases()), tc.AUX_NAMES, tc.AUX_RANGES
    else:
        (names, ranges), recs = tc.rg_name_table(), tc.aux_layout(tc.rg_name_cases())
    gpu_ctx.set_reference(REF)
    gpu_ctx.set_insert_ranges(names, ranges)
    pipe, raw, off = _pipe_for(gpu_ctx, recs, 100)
    tri, cand = _compare_triage(pipe, raw, off, names, ranges)
    assert len({t.range_max for t, _ in tri if t.cls == 3}) >= 2 and {3, 16} <= {t.cls for t, _ in tri}


@pytest.mark.parametrize("table", ["2048", "2052", "6144", "no_generic", "empty", "defer"])
def test_read_group_tables(gpu_ctx, table):
    names, ranges = tc.rg_table(int(table) if table.isdigit() else 2048)
    cases = tc.rg_table_cases(names)
    if table.isdigit():
        assert tc.table_bytes(names) == int(table)
    if table == "no_generic":
        k = names.index("generic")
        names, ranges = names[:k] + names[k + 1:], ranges[:k] + ranges[k + 1:]
    if table == "empty":
        names, ranges = [], []
    if table == "defer":
        cases = cases + tc.defer_cases()
    recs = [r for r, _ in cases]
    gpu_ctx.set_reference(REF)
    gpu_ctx.set_insert_ranges(names, ranges)
    pipe, raw, off = _pipe_for(gpu_ctx, recs, 100)
    if table != "defer":
        tri, cand = _compare_triage(pipe, raw, off, names, ranges)
        if table == "no_generic":
            assert all(t.cls == 16 for (_, m), (t, _) in zip(cases, tri) if m["kind"] == "no_rg") and any(t.cls == 3 for t, _ in tri)
        if table == "empty":
            assert all(t.cls == 16 for t, _ in tri)
        return
    pipe.tp.defer_ranges = 1
    tri, cand = _compare_triage(pipe, raw, off, names, ranges, defer=True)
    h_cls = pipe.d_class.download(np.uint8, len(recs))
    assert not pipe.d_range.download(np.int32, len(cand)).any()
    for (r, m), c in zip(cases, h_cls):
        assert (c == 16) == (m["kind"] == "rg_type" or b"RGAx" in r), m
        if m["kind"] == "pe":
            assert (c == 4) == (0 < abs(m["isize"]) < 1000000 and m["opposite"] and b"RGAx" not in r), m


@pytest.fixture(scope="module")
def tiles():
    """the small records of section 5 and what the oracle says of each, once"""
    tpl = tc.tile_templates()
    keys = ["cand", "counted", "skip", "err"]
    flat = [r for k in keys for r in tpl[k]]
    first = np.cumsum([0] + [len(tpl[k]) for k in keys])[:4]
    raw, off = tc.batch(flat)
    tri = ob.triage_records(raw, off, ["generic"], [700], eth_vcf=0)
    E = capi.MAX_EV
    T = dict(cls=np.array([t.cls for t, _ in tri], np.uint8), want=np.array([t.want != 0 for t, _ in tri]),
             len=np.array([t.l_seq for t, _ in tri], np.int32), tid=np.array([t.tid for t, _ in tri], np.int32),
             anchor=np.array([t.anchor for t, _ in tri], np.int32), range=np.array([t.range_max for t, _ in tri], np.int32),
             bases=[(b or b"") + bytes((-len(b or b"")) % 4) for _, b in tri],
             ev=np.array([[(t.ev_cls[k], t.ev_b1[k], t.ev_b2[k]) if k < t.n_ev else (-1, 0, 0) for k in range(E)] for t, _ in tri], np.int32))
    assert (T["cls"][T["want"]] < 16).all()
    return tpl, keys, flat, first, T


@pytest.mark.parametrize("n", tc.TILE_COUNTS)
def test_tiles_and_groups(gpu_ctx, tiles, n):
    """record counts around the workgroup (256) and the group of 32 workgroups (8192), patterns that put 0, 1 and 256 candidates,
    counted records and error records into a workgroup's packed totals"""
    tpl, keys, flat, first, T = tiles
    gpu_ctx.set_reference(REF)
    gpu_ctx.set_insert_ranges(["generic"], [700])
    pipe = capi.Pipeline(gpu_ctx, n, 64 * n + 64, cap_cand=n, read_len_max=12, ethreshold_vcfcheck=0)
    E = capi.MAX_EV
    for name in tc.TILE_PATTERNS:
        role, sub = tc.tile_pattern(name, n, tpl)
        tmpl = first[role] + sub
        raw, off = tc.batch([flat[k] for k in tmpl])
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
            continue
        assert np.array_equal(pipe.d_cand_rec.download(np.int32, m), cand.astype(np.int32)), name
        assert np.array_equal(pipe.d_boff.download(np.int64, m), np.cumsum(pad) - pad), name
        assert np.array_equal(pipe.d_len.download(np.int32, m), lens), name
        assert pipe.d_bases.download(np.uint8, int(pad.sum())).tobytes() == b"".join(T["bases"][k] for k in tmpl[cand]), name
        assert np.array_equal(pipe.d_tid.download(np.int32, m), T["tid"][tmpl[cand]]), name
        assert np.array_equal(pipe.d_anchor.download(np.int32, m), T["anchor"][tmpl[cand]]), name
        assert np.array_equal(pipe.d_range.download(np.int32, m), T["range"][tmpl[cand]]), name
        ev = T["ev"][tmpl[cand]].reshape(m * E, 3)
        for buf, col in ((pipe.d_cls, 0), (pipe.d_b1, 1), (pipe.d_b2, 2)):
            assert np.array_equal(buf.download(np.int32, m * E), ev[:, col]), (name, col)


def _outputs(pipe, m, nbytes):
    E = capi.MAX_EV
    return dict(cand_rec=pipe.d_cand_rec.download(np.int32, m), boff=pipe.d_boff.download(np.int64, m), len=pipe.d_len.download(np.int32, m),
                bases=pipe.d_bases.download(np.uint8, nbytes), tid=pipe.d_tid.download(np.int32, m), anchor=pipe.d_anchor.download(np.int32, m),
                range=pipe.d_range.download(np.int32, m), cls=pipe.d_cls.download(np.int32, m * E), b1=pipe.d_b1.download(np.int32, m * E),
                b2=pipe.d_b2.download(np.int32, m * E))


def _scribble(pipe):
    for buf in (pipe.d_cand_rec, pipe.d_boff, pipe.d_len, pipe.d_bases, pipe.d_tid, pipe.d_anchor, pipe.d_range, pipe.d_cls, pipe.d_b1, pipe.d_b2):
        buf.upload(np.full(buf.nbytes, 0xCD, np.uint8))


def _run_chunks(pipe, raw, off, bounds, which, clear=False, restart_first=True):
    """chunks bounds[k]..bounds[k + 1] for k in which, each uploaded over the last one once that has been triaged; returns the
    chunks' rec_class"""
    out = []
    for k in which:
        a, b = int(bounds[k]), int(bounds[k + 1])
        pipe.upload(raw[int(off[a]):int(off[b])], (off[a:b + 1] - off[a]).astype(np.uint32))
        pipe.triage_append(b - a, a, restart=restart_first and k == 0, clear=clear)
        pipe.sync()                                     # before the next chunk overwrites the record buffer
        out.append(pipe.d_class.download(np.uint8, b - a))
    return out


def test_chunks_append_to_one_candidate_set(gpu_ctx):
    """im_dev_triage chunk after chunk the way the product calls it: rec_base running on, restart = 1 on the first call over
    counters that hold 0x7F bytes, appending calls behind it -- against the same records as one chunk"""
    recs = tc.append_batch()
    n = len(recs)
    gpu_ctx.set_reference(REF)
    gpu_ctx.set_insert_ranges(tc.AUX_NAMES, tc.AUX_RANGES)
    one, raw, off = _pipe_for(gpu_ctx, recs, 2600)
    tri, cand = _compare_triage(one, raw, off, tc.AUX_NAMES, tc.AUX_RANGES)
    m = len(cand)
    want_c = one.fetch_counts()
    nbytes = int(want_c[1])
    want = _outputs(one, m, nbytes)
    want_cls = one.d_class.download(np.uint8, n)
    bounds = np.concatenate([[0], np.cumsum(tc.APPEND_CHUNKS), [n]])
    pipe = capi.Pipeline(gpu_ctx, int(np.diff(bounds).max()), len(raw), cap_cand=n, read_len_max=2600)
    E = capi.MAX_EV
    for _pass in range(2):                              # the second pass: restart = 1 over the first one's counters
        _scribble(pipe)
        if _pass == 0:
            pipe.d_counters.upload(np.full(64, 0x7F, np.uint8))
        got_cls = np.concatenate(_run_chunks(pipe, raw, off, bounds, range(len(bounds) - 1)))
        c = pipe.d_counters.download(np.int32, 8)
        assert list(c[:5]) == [m, nbytes, int(want_c[2]), int(want_c[3]), 0], (_pass, c, want_c)
        assert np.array_equal(got_cls, want_cls), (_pass, np.nonzero(got_cls != want_cls)[0][:8])
        got = _outputs(pipe, m, nbytes)
        for key in want:
            assert np.array_equal(got[key], want[key]), (_pass, key, np.nonzero(got[key] != want[key])[0][:8])
    # the triage clears the flush marks of its own new candidates and of no others
    pipe.d_consumed.upload(np.full(pipe.n_slots, 7, np.int32))
    _run_chunks(pipe, raw, off, bounds, range(4), clear=True)
    c0 = int(pipe.d_counters.download(np.int32, 8)[0])
    assert 0 < c0 < m
    marks = pipe.d_consumed.download(np.int32, pipe.n_slots)
    assert not marks[:c0 * E].any() and (marks[c0 * E:] == 7).all()
    pipe.d_consumed.upload(np.full(pipe.n_slots, 9, np.int32))
    _run_chunks(pipe, raw, off, bounds, range(4, len(bounds) - 1), clear=True)
    marks = pipe.d_consumed.download(np.int32, pipe.n_slots)
    assert int(pipe.d_counters.download(np.int32, 8)[0]) == m
    assert (marks[:c0 * E] == 9).all() and not marks[c0 * E:m * E].any() and (marks[m * E:] == 9).all()


def test_depth_feed_window_edges():
    """the pileup scatter through the workgroup's LDS window and past it, every position of both contigs against imo_depth_add"""
    recs = tc.depth_cases()
    raw, off = tc.batch(recs)
    n = len(recs)
    clens = tc.DEPTH_CONTIGS
    want = [ob.depth_of(raw, off, t, clen).astype(np.int64) for t, clen in enumerate(clens)]
    o_cls = np.array([t.cls for t, _ in ob.triage_records(raw, off, ["generic"], [700])], np.uint8)
    ctx = capi.Context(0)
    try:
        ctx.set_reference([b"A" * clens[0], b"C" * clens[1]])
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
        bounds = [0, 389, n]                            # two chunks in sequence on one array, cut inside a workgroup
        _run_chunks(pipe, raw, off, bounds, range(2))
        check("two chunks")
    finally:
        ctx.close()


def _unmapped_batch(rng, lens):
    return [tc.rec(0x1 | 0x4 | 0x40 | (0x20 if k & 1 else 0), cigar=(), l_seq=int(L), seq=tc.pack(tc.good_codes(rng, int(L))), mpos=1000 + k)
            for k, L in enumerate(lens)]


def test_candidates_that_do_not_fit(gpu_ctx):
    """A candidate is accepted iff ci < cap_cand and base_off + padded length + 16 <= cap_bases (include/indelminer_amd.h,
    im_dev_cands); every other one counts in counters[4] and nothing of it is written.  The decode kernel used to walk the
    refused candidates below cap_cand with whatever base_off / read_len / seq_at held: a pass that fits runs first, so that every
    such word holds an in-range value, and the bytes behind the accepted reads must still hold the 0xEE they are filled with."""
    rng = np.random.default_rng(808)
    n = 600
    gpu_ctx.set_reference(REF)
    gpu_ctx.set_insert_ranges(["generic"], [700])
    # the pass that fits: 16 bases each, so the words it leaves name 16 bytes at 16 * ci, up to the buffer's end.  The pass that
    # does not: thirty reads of about 256 bases fill most of the buffer, the 2600-base read behind them does not fit, and
    # no read behind that one does (base_off only grows) -- their stale offsets lie behind the accepted reads from ci = 480 on
    first = _unmapped_batch(rng, np.full(n, 16))
    second = _unmapped_batch(rng, np.concatenate([rng.integers(250, 261, 30), [2600], rng.integers(97, 132, n - 31)]))
    raw1, off1 = tc.batch(first)
    raw2, off2 = tc.batch(second)
    pipe = capi.Pipeline(gpu_ctx, n, len(raw2), cap_cand=n, read_len_max=16)
    pipe.upload(raw1, off1)
    pipe.triage()
    c = pipe.fetch_counts()
    assert list(c[:5]) == [n, 16 * n, n, 0, 0]
    pipe.d_bases.upload(np.full(pipe.cap_bases, 0xEE, np.uint8))
    tri = ob.triage_records(raw2, off2, ["generic"], [700])
    assert all(t.cls == 2 for t, _ in tri)
    lens = np.array([t.l_seq for t, _ in tri], np.int64)
    pad = (lens + 3) // 4 * 4
    bo = np.cumsum(pad) - pad
    fits = bo + pad + 16 <= pipe.cap_bases
    k = int(fits.sum())
    assert k == 30 and fits[:k].all() and 16 * (n - 1) + 16 > bo[k] and 16 * n <= pipe.cap_bases
    pipe.upload(raw2, off2)
    pipe.triage()
    c = pipe.fetch_counts()
    print("bytes: accepted", k, "of", n, "counters", c[:5])
    assert list(c[:5]) == [n, int(pad.sum()), n, 0, n - k]
    assert np.array_equal(pipe.d_cand_rec.download(np.int32, k), np.arange(k, dtype=np.int32))
    assert np.array_equal(pipe.d_boff.download(np.int64, k), bo[:k]) and np.array_equal(pipe.d_len.download(np.int32, k), lens[:k])
    assert np.array_equal(pipe.d_anchor.download(np.int32, k), 1000 + np.arange(k, dtype=np.int32))
    bases = pipe.d_bases.download(np.uint8, pipe.cap_bases)
    end = int(bo[k - 1] + pad[k - 1])
    assert bases[:end].tobytes() == b"".join(b + bytes((-len(b)) % 4) for _, b in tri[:k])
    assert (bases[end:] == 0xEE).all(), np.nonzero(bases[end:] != 0xEE)[0][:8] + end
    assert np.array_equal(pipe.d_class.download(np.uint8, n), np.full(n, 2, np.uint8))
    # the opposite case: room for the bytes, not for the candidates
    cap = 300
    small = capi.Pipeline(gpu_ctx, n, len(raw2), cap_cand=cap, read_len_max=600)
    small.upload(raw2, off2)
    small.triage()
    c = small.fetch_counts()
    print("candidates: accepted", cap, "of", n, "counters", c[:5])
    assert list(c[:5]) == [n, int(pad.sum()), n, 0, n - cap]
    assert np.array_equal(small.d_cand_rec.download(np.int32, cap), np.arange(cap, dtype=np.int32))
    assert np.array_equal(small.d_boff.download(np.int64, cap), bo[:cap]) and np.array_equal(small.d_len.download(np.int32, cap), lens[:cap])
    end = int(bo[cap - 1] + pad[cap - 1])
    assert small.d_bases.download(np.uint8, end).tobytes() == b"".join(b + bytes((-len(b)) % 4) for _, b in tri[:cap])
    assert (small.d_cls.download(np.int32, cap * capi.MAX_EV) == -1).all()
