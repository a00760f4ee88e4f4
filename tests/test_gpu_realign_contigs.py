"""The realign kernels with SIX contigs resident and reads on all of them (tests/support/contigedges.py): every table form of
realign_kernel and both lane layouts, the band kernel, the long-read kernel and the general pass, each with a contig index other than
0, with windows clipped at a contig's first and last base, and with another contig's bases 64 bytes behind the end of its own.  Every
record is held to the CPU oracle on that read's OWN contig; tests/test_contig_edges_host.py proves that the oracle's answer changes
when the contig's length is ignored.  Bit-exact: integer / index work."""
import ctypes as C

import numpy as np
import pytest

from tests.support import contigedges as ce, gpucmp, oraclebind as ob

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", sorted(ce.BATCHES))
def test_hip_matches_oracle_on_six_resident_contigs(name):
    from indelminer_amd import capi
    cases, want, _dropped = ce.checked(name)
    kw = ce.params(name)
    contigs = [s.encode() for s in ce.contigs()]
    ctx = capi.Context(0)           # its own context: which kernels follow one another depends on the longest read a context has seen
    try:
        ctx.set_reference(contigs)
        rc, out = ctx.realign_batch(capi.params(**kw), [c["read"].encode() for c in cases],
                                    np.array([c["tid"] for c in cases], np.int32),
                                    np.array([c["anchor"] for c in cases], np.int32),
                                    np.array([c["range_max"] for c in cases], np.int32), allow=(capi.E_ABORT,))
    finally:
        ctx.close()
    bad, n_bad_tid = [], 0
    for i, (c, w) in enumerate(zip(cases, want)):
        if c["kind"] == "bad_tid":
            n_bad_tid += 1
            if (int(out[i]["status"]), int(out[i]["n_ev"])) != (capi.ST_ABORT, 0):
                bad.append((i, "bad tid: status %d n_ev %d" % (out[i]["status"], out[i]["n_ev"]), c))
            continue
        msg = gpucmp.hip_vs_oracle(out[i], *w)
        if msg:
            bad.append((i, msg, c))
    # the failing reads whole (index, difference, case): each is a case to keep by name
    assert not bad, "%s %r: %d of %d differ, first: %r" % (name, kw, len(bad), len(cases), bad[:5])
    assert n_bad_tid == 2 and rc == capi.E_ABORT
    assert not (out["status"] == capi.ST_UNSUPPORTED).any()
    has = [int(r["status"]) == capi.ST_EVIDENCE and int(r["n_ev"]) > 0 for r in out]
    per = ce.evidence_per_contig(cases, has)
    assert min(per) >= ce.MIN_EVIDENCE, per
    assert not any(h for c, h in zip(cases, has) if c["kind"].startswith("continue"))
    assert all(int(r["status"]) != capi.ST_ABORT for c, r in zip(cases, out) if c["kind"] == "a_run")


@pytest.mark.parametrize("read_len,g,coverage", ce.PIPELINE_RUNS)
def test_pipeline_paths_on_several_contigs(read_len, g, coverage):
    """device triage of a few thousand records on three contigs, then im_dev_realign_n with the candidate count left on the device (the
    entry the product's passes use): the long-read kernel on 300-base reads at -g 0, the band kernel on 100-base reads at -g 2; every
    candidate against the oracle on its own contig"""
    from indelminer_amd import capi, rawrec
    from tests.test_gpu_triage import _compare_triage
    refs, rd = ce.pipeline_input(read_len, coverage)
    raw, off = rawrec.records(rd)
    contigs = [r.tobytes() for r in refs]
    ctx = capi.Context(0)
    try:
        ctx.set_reference(contigs)
        ctx.set_insert_ranges(["generic"], [rd.range_max])
        ctx.expect_read_length(read_len)
        pipe = capi.Pipeline(ctx, rd.n, len(raw), cap_cand=rd.n, read_len_max=read_len)
        pipe.P = capi.params(numgaps=g)
        tri, cand = _compare_triage(pipe, raw, off, ["generic"], [rd.range_max])
        assert {tri[i][0].tid for i in cand} == {0, 1, 2}
        bound = capi.DevBatch(pipe.cap_cand, pipe.d_bases.ptr, pipe.d_boff.ptr, pipe.d_len.ptr, pipe.d_tid.ptr, pipe.d_anchor.ptr,
                              pipe.d_range.ptr, pipe.d_res.ptr, pipe.d_cls.ptr, pipe.d_b1.ptr, pipe.d_b2.ptr)
        ctx._check(capi.lib().im_dev_realign_n(ctx.h, C.byref(pipe.P), C.byref(bound), pipe.d_counters.ptr, 1, ctx.stream))
        pipe.sync()
        out = pipe.d_res.download(capi.RESULT_DTYPE, len(cand))
    finally:
        ctx.close()
    P = ob.params(numgaps=g)
    found = [0, 0, 0]
    for j, i in enumerate(cand):
        t, b = tri[i]
        st, res = ob.realign(P, contigs[t.tid], len(contigs[t.tid]), t.anchor, t.range_max, b)
        msg = gpucmp.hip_vs_oracle(out[j], st, res)
        assert msg is None, (j, i, t.tid, t.anchor, msg)
        found[t.tid] += ce.has_evidence(st, res)
    assert sum(found) >= 30 and min(found) >= 1, found
