"""The premises of tests/test_gpu_overlapped.py, from the CPU oracle and the restatements alone (no GPU): the inputs reach what those
tests name.  These are conditions on the inputs, not measurements of the code under test."""
import numpy as np

from indelminer_amd import capi
from tests.support import stepmodel as sm

E = capi.MAX_EV


def test_the_four_sets_differ_and_reach_every_stage():
    four = sm.four_sets()
    counts = [len(m.cand_rec) for _, m in four]
    assert len(set(counts)) == 4 and [i.rd.n for i, _ in four] == [12_000, 30_000, 1_600, 4_000], counts
    assert [i.tid for i, _ in four] == [0, 1, 2, 3] and len({len(i.contig) for i, _ in four}) == 3
    for (inp, m), (name, _) in zip(four, sm.SETS):
        live = m.cls >= 0
        assert len(inp.flushes) == 4 and all(a[3] <= b[3] for a, b in zip(inp.flushes, inp.flushes[1:])), name     # markers never decrease
        assert len(set(m.cons[live].tolist())) >= 3 and (m.cons[live] > 0).all(), name           # at least three flushes consume split-read slots
        assert max(len(v) for v in m.clusters.values()) >= 2, name
        assert m.kept > 0 and sum(1 for st, r in m.results if st == 1 and r.n_ev > 0) > m.kept // 8, name       # realigned and kept evidence
        assert {st for st, _ in m.results} == {0, 1}, name
        assert m.depth.max() > 0 and m.n_records == inp.rd.n, name
        assert len(m.cand_rec) <= inp.rd.n // 4                                             # the capacity new_pipeline gives
    # the two larger sets have paired-read entries in every cut; the long set has reads above 255 bases among its candidates
    assert all(set(four[k][1].cons_pe.tolist()) == {1, 2, 3, 4} for k in (0, 1))
    long_inp, long_model = four[3]
    assert long_inp.rd.read_len == 300 > capi.SHORT_READ and len(long_model.cand_rec) > 100
    assert long_inp.rd.range_max == sm.RG_RANGE[1] != four[0][0].rd.range_max == sm.RG_RANGE[0]


def test_quiet_is_much_smaller_than_busy_and_a_leak_would_show():
    (busy, bm), (quiet, qm) = sm.busy_and_quiet()
    assert quiet.rd.n == busy.rd.n == 12_000 and len(quiet.flushes) == len(busy.flushes)
    assert 0 < 4 * len(qm.cand_rec) < len(bm.cand_rec)
    assert quiet.contig == busy.contig and len(quiet.pe_b1) < len(busy.pe_b1)
    # busy's live slots beyond quiet's hold consumed split-read evidence: a replay that left them in reach would be seen
    beyond = slice(len(qm.cand_rec) * E, None)
    assert int(((bm.cls[beyond] >= 0) & (bm.cons[beyond] > 0)).sum()) > 100
    assert any(min(v) >= len(qm.cand_rec) * E for v in bm.clusters.values())
    # check() handed the other input's model fails on every part
    assert len(qm.clusters) > 0 and not set(qm.clusters) & set(bm.clusters)
    assert not np.array_equal(qm.depth, bm.depth) and not np.array_equal(qm.rec_class, bm.rec_class)
    assert not np.array_equal(qm.cand_rec, bm.cand_rec[:len(qm.cand_rec)])
    assert all(a != b for a, b in zip(sm.digest(qm), sm.digest(bm)))


def _kinds(parsed, clens, range_max):
    """how many records of each kind a chunk holds: reference-spanning, concordant pair, right clip, left clip, clip tail, mis-oriented pair"""
    from tests.support import clipcounts as cc, cliptails as ct, pairlinks as pk
    from tests.test_gpu_pairspan import fragment_of
    from tests.test_gpu_span import eligible, runs_of
    spans, pairs, tails = parsed
    m, q, c = sm.SCATTER["m"], sm.SCATTER["q"], sm.SCATTER["c"]
    ev = [e for r in tails for e in cc.events_of(r, clens, c, q)]
    return (sum(1 for t, p, mq, f, cg in spans if eligible(t, f, mq, len(clens), q) and any(e - s >= 2 * m for s, e in runs_of(p, cg))),
            sum(1 for r in pairs if fragment_of(r, len(clens), q, {"generic": range_max}) is not None),
            sum(1 for e in ev if e[1] == cc.RIGHT), sum(1 for e in ev if e[1] == cc.LEFT),
            sum(len(ct.entries_of(r, clens, c, q)) for r in tails),
            len(pk.links_of([pk.Rec(*p[:6]) for p in pairs], clens, q)))


def test_every_scatter_chunk_holds_every_kind_and_dropping_one_shows():
    from tests.support import crossedpiles as cp, pairlinks as pk
    inp = sm.scatter_input()
    clens, chunks = inp["clens"], inp["chunks"]
    span, pspan, R, L, table, links, _ = inp["models"]
    assert len(chunks) == 4 and all((len(off) - 1) % 64 for _, off in chunks)
    total = [0] * 6
    alone = [sm.scatter_models([ch], clens, inp["range_max"]) for ch in chunks]
    for part in alone:
        kinds = _kinds(part[6], clens, inp["range_max"])
        assert all(k >= 1 for k in kinds), kinds
        total = [a + b for a, b in zip(total, kinds)]
    # no overflow is expected: both tables keep half of their 2^14 slots
    assert total[4] == sum(len(v) for v in table.values()) and total[5] == len(links)
    assert 0 < total[4] < 2**sm.SCATTER["log2_slots"] // 2 and 0 < total[5] < 2**sm.SCATTER["log2_slots"] // 2
    # what the GPU test asks of the models
    assert len(cp.peaks_many(R[0], 3, 30)) >= 9 and len(cp.peaks_many(L[0], 3, 30)) >= 9
    assert len(cp.crossed(R[0], L[0], table, inp["contigs"][0], 0, *sm.CROSSED_PAR)[0]) >= 9
    windows = [pk.window_of("DUP", None, a, a + n) for a, n in cp.SITES]
    assert sum(pk.count(links, clens, 0, *w, pk.MIN_SEP) for w in windows) >= 9
    # the four-stream scatter fails if one chunk is dropped.  Every structure is the sum of its chunks' contributions ...
    for k, whole in enumerate((span, pspan, R, L)):
        assert np.array_equal(sum(part[k][0] for part in alone), whole[0])
    assert sorted(x for part in alone for x in part[5]) == sorted(links)
    assert {key: sorted(v) for key, v in table.items()} == \
        {key: sorted(b for part in alone for b in part[4].get(key, [])) for key in set().union(*[part[4] for part in alone])}
    # ... and no chunk's contribution to any of them is empty: the models without chunk k differ from the models of all four
    for part in alone:
        assert all(part[k][0].any() for k in range(4)) and len(part[4]) > 0 and len(part[5]) > 0
