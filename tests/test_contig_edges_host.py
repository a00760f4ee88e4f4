"""The cases of tests/support/contigedges.py are what they claim -- on the CPU oracle, no GPU: the planted reads yield evidence on every
contig, a read that continues into the neighbouring contig yields NONE on its own contig and a deletion of the pad on the memory
image, and the reads carried on with 'A' come back with a defined status.  The second and third together are the proof that a
kernel which ignores a contig's length on any path fails tests/test_gpu_realign_contigs.py."""
import pytest

from tests.support import contigedges as ce, oraclebind as ob


def test_layout_and_contigs():
    c = ce.contigs()
    assert [len(s) for s in c] == ce.LENGTHS and ce.pads(ce.LENGTHS) == ce.PADS
    assert ce.PADS[0] == ce.PADS[1] == ce.PADS[4] == 64 and ce.PADS[2] == 64 + 255
    for t in ce.ENDS_IN_A:
        assert c[t].endswith("A" * ce.A_RUN) and c[t + 1].startswith("A" * ce.A_RUN)
    assert ce.BEGINS_WITH_A == tuple(t + 1 for t in ce.ENDS_IN_A)
    assert all(set(s) <= set("ACGT") for s in c)
    seq, at = ce.image(2)
    assert at == 2497 + 319 and seq[at:] == c[3] and seq[:2497] == c[2] and set(seq[2497:at]) == {ce.FILLER}


@pytest.mark.parametrize("name", sorted(ce.BATCHES))
def test_batch_is_what_it_claims(name):
    raw = ce.batch(name)
    cases, want, dropped = ce.checked(name)
    k, g, lengths, Rm, maxdel = ce.BATCHES[name]
    assert len(raw) <= ce.MAX_READS and len(cases) == len(raw) - dropped
    kinds = [c["kind"] for c in raw]
    assert kinds.count("bad_tid") == 2 and sorted(c["tid"] for c in raw if c["kind"] == "bad_tid") == [-1, len(ce.LENGTHS)]
    n_cont = kinds.count("continue_right") + kinds.count("continue_left")
    assert kinds.count("continue_right") == kinds.count("continue_left") == 30
    assert {(c["kind"], c["tid"]) for c in raw if c["kind"].startswith("continue")} == \
        {("continue_right", t) for t in range(5)} | {("continue_left", t + 1) for t in range(5)}
    assert 20 * dropped <= n_cont, dropped
    assert {c["tid"] for c in raw if c["kind"] == "a_run"} == set(ce.ENDS_IN_A + ce.BEGINS_WITH_A)
    got_lengths = {len(c["read"]) for c in raw if c["kind"] == "indel"}
    assert set(lengths) <= got_lengths, (lengths, got_lengths)
    assert not any(c["tid"] == 3 and len(c["read"]) >= 300 for c in raw)
    assert all(len(c["read"]) <= ce.LENGTHS[c["tid"]] for c in raw if c["kind"] == "indel")
    for c in raw:
        L = len(c["read"])
        if c["kind"].startswith("continue"):
            assert (L + 2) // 3 <= c["own"] <= L - (L + 2) // 3 + 1, (L, c["own"])

    # every contig gets planted reads, and they yield evidence there
    has = [w is not None and ce.has_evidence(*w) for w in want]
    per = ce.evidence_per_contig(cases, has)
    print(name, "indel reads with evidence per contig", per, "continue reads dropped", dropped)
    assert {c["tid"] for c in cases if c["kind"] == "indel"} == set(range(len(ce.LENGTHS)))
    assert min(per) >= ce.MIN_EVIDENCE, per

    # nothing to find for a continued read on its own contig (checked() dropped the exceptions); no abort on the 'A' runs
    for c, w in zip(cases, want):
        if c["kind"].startswith("continue"):
            assert not ce.has_evidence(*w)
        if c["kind"] == "a_run":
            assert w[0] in (0, 1, -2), (c, w[0])

    # ... and a deletion to find on the memory image: what a kernel that ran over the contig's end (or start) would report
    P = ob.params(**ce.params(name))
    found = 0
    for c in raw:
        if c["kind"] == "continue_right":
            seq, at = ce.image(c["tid"])
            st, res = ob.realign(P, seq.encode(), len(seq), c["anchor"], c["range_max"], c["read"])
        elif c["kind"] == "continue_left":
            seq, at = ce.image(c["tid"] - 1)
            st, res = ob.realign(P, seq.encode(), len(seq), c["anchor"] + at, c["range_max"], c["read"])
        else:
            continue
        found += ce.has_evidence(st, res)
    print(name, "continued reads with evidence on the memory image: %d of %d" % (found, n_cont))
    assert 4 * found >= 3 * n_cont, (found, n_cont)


@pytest.mark.parametrize("read_len,g,coverage", ce.PIPELINE_RUNS)
def test_pipeline_input_delivers_candidates_with_evidence_on_every_contig(read_len, g, coverage):
    """the input of test_pipeline_paths_on_several_contigs: a few thousand reads, candidates on all three contigs, at least 30 of
    them with evidence"""
    from indelminer_amd import synth
    refs, rd = ce.pipeline_input(read_len, coverage)
    assert [len(r) for r in refs] == ce.PIPELINE_REF_LENS and 2000 <= rd.n <= 6000, rd.n
    cand = synth.candidates(rd)
    assert set(int(t) for t in cand["tid"]) == {0, 1, 2}
    P = ob.params(numgaps=g)
    contigs = [r.tobytes() for r in refs]
    found = [0, 0, 0]
    for t, a, r, b in zip(cand["tid"], cand["anchor"], cand["range_max"], cand["bases"]):
        st, res = ob.realign(P, contigs[t], len(contigs[t]), int(a), int(r), bytes(b))
        found[t] += ce.has_evidence(st, res)
    print(read_len, g, "candidates", len(cand["tid"]), "with evidence per contig", found)
    assert sum(found) >= 30 and min(found) >= 1, found
