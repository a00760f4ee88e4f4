"""What one bound pass (capi.Pipeline.bind_async: triage -> realign -> flush list -> group-by, with the contig's depth run) leaves in a
Pipeline's buffers, worked out from the CPU oracle alone, and the comparison of a Pipeline with it.  Nothing here runs the code under
test to learn what to expect; check() only downloads.  Test infrastructure only.

The inputs of tests/test_gpu_overlapped.py are built here as well, so that tests/test_overlapped_host.py can show without a GPU what
they reach."""
import collections

import numpy as np

from indelminer_amd import capi, rawrec, synth
from . import gpucmp, oraclebind as ob

E = capi.MAX_EV
INT_MAX = 2**31 - 1

# read groups of the context the sets share: the 2 x 300 set has its own insert range
RG_NAMES = ["generic", "wide"]
RG_RANGE = [700, 1100]

# (name, simulate() arguments): four sets that differ in size, density and read length
SETS = (("s21", dict(seed=21, ref_len=60_000, coverage=20, big_every=5)),
        ("s22", dict(seed=22, ref_len=150_000, coverage=20, big_every=5)),
        ("s23", dict(seed=23, ref_len=20_000, coverage=8, big_every=5)),
        ("long", dict(seed=8, ref_len=60_000, coverage=20, read_len=300, isize_mean=900, isize_sd=50, isize_min=700, isize_max=1100)))
BUSY = dict(seed=21, ref_len=60_000, coverage=20, big_every=5)
QUIET = dict(seed=31, ref_len=60_000, coverage=20, sub_rate=0.0005, indel_spacing=30000)

Input = collections.namedtuple("Input", "contig rd raw off flushes pe_b1 pe_b2 tid")
Model = collections.namedtuple("Model", "n_records rec_class cand_rec results cls b1 b2 kept n_pe pe_b1 pe_b2 cons cons_pe clusters depth tid")


def fine_flushes(rd):
    """bench.flush_schedule's paired-read entries, and a flush list cut finer than READCHUNK: three mid-contig record cuts whose marker
    is the position of the last record in front of the cut, then the closing flush"""
    import bench
    flushes, pe_b1, pe_b2 = bench.flush_schedule(rd)
    cuts = [rd.n // 4, rd.n // 2, 3 * rd.n // 4]
    fine = [(0, c, len(pe_b1) * c // rd.n, int(rd.pos[c - 1])) for c in cuts] + [flushes[-1]]
    assert fine[-1] == (0, rd.n, len(pe_b1), INT_MAX)
    return fine, pe_b1, pe_b2


def make_input(tid=0, qual=True, contig=None, **sim):
    """one simulated contig as contig `tid` of a context: refID / next_refID of the raw records rewritten the way bench.PipeStep does.
    contig: the bases the context holds for `tid` where they are not the simulated ones (records of another sample on a resident
    reference)"""
    refs, rd = synth.simulate(**sim)
    if contig is not None:
        assert len(contig) == len(refs[0])
        refs = [np.frombuffer(contig, np.uint8)]
    rg = "wide" if rd.range_max == RG_RANGE[1] else None
    assert rd.range_max == RG_RANGE[1 if rg else 0]
    raw, off = rawrec.records(rd, rg=rg, qual=qual)
    raw = raw.copy()
    r32 = raw[:len(raw) // 4 * 4].view(np.int32)
    at = (off[:-1] // 4).astype(np.int64)
    for word in (0, 5):                 # refID, next_refID
        v = r32[at + word]
        r32[at + word] = np.where(v >= 0, tid, v)
    flushes, pe_b1, pe_b2 = fine_flushes(rd)
    return Input(refs[0].tobytes(), rd, raw, off, flushes, pe_b1, pe_b2, tid)


def model_of(contig, rd, raw, off, flushes, pe_b1, pe_b2, tid):
    """everything a bound pass over the input leaves behind, from the oracle: ob.triage_records, ob.realign per candidate (CIGAR-derived
    evidence stays where realignment finds none, src/indelminer.c:494-512), ob.flush_cut flush by flush, a plain group-by, ob.depth_of"""
    n = len(off) - 1
    tri = ob.triage_records(raw, off, RG_NAMES, RG_RANGE)
    rec_class = np.array([21 if (t.cls == 3 and t.n_ev > E) else t.cls for t, _ in tri], np.uint8)
    cand = [i for i in range(n) if tri[i][0].want]
    # the simulator writes no record that is refused while it is being written as a candidate; the model does not cover those
    assert all(tri[i][0].cls in (2, 3) and tri[i][0].n_ev <= E and tri[i][0].tid == tid for i in cand)
    m = len(cand)
    n_pe = len(pe_b1)
    P = ob.params()
    cls = np.full(m * E, -1, np.int32); b1 = np.zeros(m * E, np.int32); b2 = np.zeros(m * E, np.int32)
    results, kept = [], 0
    for j, i in enumerate(cand):
        t, bases = tri[i]
        st, res = ob.realign(P, contig, len(contig), t.anchor, t.range_max, bases)
        results.append((st, res))
        if st == 1 and res.n_ev > 0:
            ev = [(res.ev[k].cls, res.ev[k].b1, res.ev[k].b2) for k in range(res.n_ev)]
        else:
            ev = [(t.ev_cls[k], t.ev_b1[k], t.ev_b2[k]) for k in range(t.n_ev)]
            kept += bool(ev)
        for k, e in enumerate(ev):
            cls[j * E + k], b1[j * E + k], b2[j * E + k] = e
    # the flushes: split-read slots of the candidates inside the record bounds, then the paired-read entries in front of pe_hi
    cand_rec = np.array(cand, np.int32)
    a_cls = np.concatenate([cls, np.full(n_pe, 2, np.int32)])
    a_b1 = np.concatenate([b1, np.asarray(pe_b1, np.int32)]); a_b2 = np.concatenate([b2, np.asarray(pe_b2, np.int32)])
    cons = np.zeros(m * E + n_pe, np.int32)
    for k, (r0, r1, pe_hi, marker) in enumerate(flushes):
        lo, hi = int(np.searchsorted(cand_rec, r0)), int(np.searchsorted(cand_rec, r1))
        vis = np.full(m * E + n_pe, -1, np.int32)
        vis[lo * E:hi * E] = cls[lo * E:hi * E]; vis[m * E:m * E + pe_hi] = 2
        ob.flush_cut(vis, a_b1, a_b2, cons, marker, k + 1)
    clusters = {}
    for s in np.nonzero((cls >= 0) & (cons[:m * E] > 0))[0]:
        clusters.setdefault((int(cons[s]), int(cls[s]), int(b1[s]), int(b2[s])), []).append(int(s))
    depth = ob.depth_of(raw, off, tid, len(contig))
    return Model(n, rec_class, cand_rec, results, cls, b1, b2, kept, n_pe, np.asarray(pe_b1, np.int32), np.asarray(pe_b2, np.int32),
                 cons[:m * E].copy(), cons[m * E:].copy(), clusters, depth, tid)


def digest(model):
    """the parts of a model that two different inputs cannot share by accident (for the premise tests)"""
    return (len(model.cand_rec), model.cons.tobytes(), model.cons_pe.tobytes(), sorted(model.clusters.items()), model.depth.tobytes())


def new_pipeline(ctx, inp, n_pe=None, n_flushes=None, raw_bytes=None):
    """a buffer set sized for the input (or for more: n_pe, n_flushes, raw_bytes), holding its records and paired-read entries"""
    n_pe = max(len(inp.pe_b1), 1) if n_pe is None else n_pe
    pipe = capi.Pipeline(ctx, inp.rd.n, max(len(inp.raw), raw_bytes or 0), cap_cand=inp.rd.n // 4, read_len_max=inp.rd.read_len, n_pe=n_pe,
                         n_flushes=len(inp.flushes) if n_flushes is None else n_flushes, want_depth=True)
    load(pipe, inp)
    return pipe


def load(pipe, inp):
    """the input's records, offsets and paired-read entries into the set's buffers (the part of the region the input does not use
    holds no entry)"""
    assert len(inp.off) - 1 == pipe.n_records and len(inp.pe_b1) <= pipe.n_pe and len(inp.flushes) <= pipe.n_flushes
    pipe.upload(inp.raw, inp.off)
    base = pipe.cap_cand * E
    pad = np.full(pipe.n_pe, -1, np.int32)
    pipe.ctx._check(capi.lib().im_dev_upload(pipe.ctx.h, pipe.d_cls.ptr + 4 * base, pad.ctypes.data, 4 * pipe.n_pe))
    pipe.set_pe(inp.pe_b1, inp.pe_b2)


def check(pipe, model, depth=True):
    """downloads the Pipeline's buffers after a pass and asserts every part of the model.  Slots at or beyond n_cand * MAX_EV and below
    the paired-read base are nobody's business; clusters must name live slots only."""
    ctx = pipe.ctx
    c = pipe.fetch_counts()
    m = len(model.cand_rec)
    assert int(c[0]) == m and pipe.n_cand == m, (int(c[0]), m)
    assert int(c[2]) == int((model.rec_class != 0).sum()) and int(c[3]) == int((model.rec_class >= 16).sum()) and int(c[4]) == 0, c
    got_class = pipe.d_class.download(np.uint8, model.n_records)
    assert np.array_equal(got_class, model.rec_class), np.nonzero(got_class != model.rec_class)[0][:10]
    assert np.array_equal(pipe.d_cand_rec.download(np.int32, max(m, 1))[:m], model.cand_rec)
    out = pipe.d_res.download(capi.RESULT_DTYPE, max(m, 1))[:m]
    for j, (st, res) in enumerate(model.results):
        msg = gpucmp.hip_vs_oracle(out[j], st, res)
        assert msg is None, (j, msg)
    live, base = m * E, pipe.cap_cand * E
    h_cls = pipe.d_cls.download(np.int32, pipe.n_slots); h_b1 = pipe.d_b1.download(np.int32, pipe.n_slots); h_b2 = pipe.d_b2.download(np.int32, pipe.n_slots)
    for name, got, want in (("cls", h_cls, model.cls), ("b1", h_b1, model.b1), ("b2", h_b2, model.b2)):
        assert np.array_equal(got[:live], want), (name, np.nonzero(got[:live] != want)[0][:10])
    n_pe = model.n_pe
    assert (h_cls[base:base + n_pe] == 2).all() and np.array_equal(h_b1[base:base + n_pe], model.pe_b1) and np.array_equal(h_b2[base:base + n_pe], model.pe_b2)
    cons = pipe.d_consumed.download(np.int32, pipe.n_slots)
    assert np.array_equal(cons[:live], model.cons), np.nonzero(cons[:live] != model.cons)[0][:10]
    assert np.array_equal(cons[base:base + n_pe], model.cons_pe), np.nonzero(cons[base:base + n_pe] != model.cons_pe)[0][:10]
    key, first, count, order = pipe.clusters()
    assert len(order) == 0 or (0 <= int(order.min()) and int(order.max()) < live), (int(order.min()), int(order.max()), live)
    assert int(count.sum()) == len(order)
    got = {tuple(int(x) for x in key[k]): [int(x) for x in order[first[k]:first[k] + count[k]]] for k in range(len(key))}
    assert len(got) == len(key)                 # no key twice
    assert got == model.clusters, (len(got), len(model.clusters))
    if depth:
        check_depth(ctx, model)


def check_depth(ctx, model):
    """depth_query_tid(tid, p, p + 1) over every position of the model's contig"""
    p = np.arange(len(model.depth), dtype=np.int32)
    got = ctx.depth_query_tid(model.tid, p, p + 1)
    assert np.array_equal(got.astype(np.int64), model.depth.astype(np.int64)), np.nonzero(got.astype(np.int64) != model.depth)[0][:10]


_cache = {}


def four_sets():
    """[(Input, Model)] of SETS, set k on contig k; computed once, shared by the tests and left unchanged"""
    if "four" not in _cache:
        inputs = [make_input(tid=k, qual=k % 2 == 0, **kw) for k, (_, kw) in enumerate(SETS)]
        _cache["four"] = [(inp, model_of(*inp)) for inp in inputs]
    return _cache["four"]


def busy_and_quiet():
    """((busy Input, Model), (quiet Input, Model)): two record sets of one size for contig 0 of one context.  The context keeps busy's
    contig, so quiet's reads are realigned against it -- in the model as on the device."""
    if "bq" not in _cache:
        busy = make_input(tid=0, **BUSY)
        quiet = make_input(tid=0, contig=busy.contig, **QUIET)
        _cache["bq"] = ((busy, model_of(*busy)), (quiet, model_of(*quiet)))
    return _cache["bq"]


# ---------------------------------------------------------------------- one record set for the five scatters

SCATTER = dict(m=10, q=10, c=20, log2_slots=14, min_cover=2)
SCATTER_CUTS = (4_417, 9_003, 13_530)          # record cuts, none a multiple of 64
CROSSED_PAR = (3, 30, 50, 5_000, 32, 2)         # min_reads, reach, min_len, max_len, max_shift, min_verified


def scatter_models(chunks, clens, range_max):
    """the CPU restatements of the five structures over the parsed records of the chunks together: (span, pair-span, clipR, clipL,
    clip-tail table, links)"""
    from tests.support import clipcounts as cc, cliptails as ct, pairlinks as pk
    from tests.test_gpu_pairspan import parse_raw as parse_pairs, pspan_of
    from tests.test_gpu_span import parse_raw as parse_spans, span_of
    m, q, c = SCATTER["m"], SCATTER["q"], SCATTER["c"]
    spans, pairs, tails = [], [], []
    for raw, off in chunks:
        spans += parse_spans(raw, off); pairs += parse_pairs(raw, off); tails += ct.parse_raw(raw, off)
    R, L = cc.arrays_of(tails, clens, c, q)
    links = pk.links_of([pk.Rec(*p[:6]) for p in pairs], clens, q)
    return (span_of(spans, clens, m, q), pspan_of(pairs, clens, m, q, {"generic": range_max}), R, L, ct.table_of(tails, clens, c, q), links,
            (spans, pairs, tails))


def scatter_input():
    """pairlinks.planted_dup_reads (a 60 kb contig at 30x: reference-spanning reads, concordant pairs, the clipped reads of nine tandem
    duplications with their clipped bases, everted pairs at the longer ones) with its records in a seeded random order, so that every
    stretch of the file holds every kind, cut into four chunks.  Returns a dict: contigs, clens, range_max, chunks [(raw, off)],
    models (scatter_models of all chunks)."""
    if "scatter" not in _cache:
        from tests.support import pairlinks as pk
        refs, rd, planted = pk.planted_dup_reads()
        raw, off = rawrec.records(rd)
        order = np.random.default_rng(5).permutation(rd.n)
        b = raw.tobytes()
        parts = [b[int(off[i]):int(off[i + 1])] for i in order]
        raw = np.frombuffer(b"".join(parts), np.uint8).copy()
        off = np.concatenate([[0], np.cumsum([len(p) for p in parts])]).astype(np.uint32)
        cuts = (0,) + SCATTER_CUTS + (rd.n,)
        assert all(0 < a < rd.n and a % 64 for a in SCATTER_CUTS)
        chunks = []
        for a, e in zip(cuts[:-1], cuts[1:]):
            chunks.append((raw[int(off[a]):int(off[e])].copy(), (off[a:e + 1] - off[a]).astype(np.uint32)))
        contigs = [r.tobytes() for r in refs]
        clens = [len(x) for x in contigs]
        _cache["scatter"] = dict(contigs=contigs, clens=clens, range_max=rd.range_max, chunks=chunks, planted=planted,
                                 models=scatter_models(chunks, clens, rd.range_max))
    return _cache["scatter"]
