"""tests/support/linkcases.py, pinned where no GPU is needed: every class of record the two link rules treat differently is there, the
two restatements (tests/support/pairlinks.py, tests/support/intercontig.py) say of every case what the case states by hand, and the
chunks put the cases where a scatter workgroup of 1 024 records has its edges."""
import struct

from tests.support import intercontig as ic
from tests.support import linkcases as lc
from tests.support import pairlinks as pk


def test_every_class_is_present():
    names = [c.name for c in lc.CASES]
    assert len(set(names)) == len(names)
    want = ["same contig, everted", "same contig, forward", "same contig, reverse", "same contig, normal", "mtid -1", "mtid n_contigs",
            "pos == mpos, first in pair", "pos == mpos, second in pair", "same contig, not paired", "inter-contig, not paired",
            "same contig, 28 bytes", "inter-contig, 28 bytes"]
    want += ["inter-contig, kind %d, from contig %d" % (k, t) for t in (0, 1) for k in range(4)]
    want += ["mpos 5 000, mtid %d, from contig %d" % (m, t) for t in (0, 1) for m in (0, 1)]
    want += ["%s, mapq %d" % (w, q) for w in ("same contig", "inter-contig") for q in (lc.MIN_MAPQ - 1, lc.MIN_MAPQ)]
    want += ["%s, flag 0x%x" % (w, b) for w in ("same contig", "inter-contig") for b in (0x4, 0x8, 0x100, 0x200, 0x400, 0x800)]
    assert set(want) <= set(names)
    by = {c.name: c for c in lc.CASES}
    assert by["mtid n_contigs"].rec.mtid == len(lc.CLENS) and by["mtid -1"].rec.mtid == -1
    assert lc.CLENS == [20_000, 2_000] and all(lc.CLENS[1] < by[n].rec.mpos == 5_000 < lc.CLENS[0] for n in by if n.startswith("mpos 5 000"))
    # the inter-contig kinds are the four, from either contig
    assert sorted(ic.link_of(by["inter-contig, kind %d, from contig %d" % (k, t)].rec, lc.CLENS, lc.MIN_MAPQ)[:2] for t in (0, 1) for k in range(4)) == \
        [(t, k) for t in (0, 1) for k in range(4)]


def test_the_restatements_say_what_the_cases_state():
    for c in lc.CASES + [lc.PLAIN]:
        pair, mate = pk.link_of(c.rec, lc.CLENS, lc.MIN_MAPQ), ic.link_of(c.rec, lc.CLENS, lc.MIN_MAPQ)
        if c.short:
            # a whole record of these bytes would be a link: the 28 bytes alone keep it out
            assert (pair is not None) != (mate is not None) and not c.pair and not c.mate, c.name
            continue
        assert (pair is not None, mate is not None) == (c.pair, c.mate), c.name
        assert not (c.pair and c.mate), c.name                       # no record is a link of both
        if c.rec.mtid != c.rec.tid:
            assert pair is None, c.name                             # the inter-contig ones are links of the mate rule only
        if c.rec.mtid == c.rec.tid:
            assert mate is None, c.name
    assert sum(c.pair for c in lc.CASES) >= 6 and sum(c.mate for c in lc.CASES) >= 10
    # where a position check against the WRONG contig would answer differently
    by = {c.name: c.rec for c in lc.CASES}
    assert ic.link_of(by["mpos 5 000, mtid 1, from contig 0"], lc.CLENS, lc.MIN_MAPQ) is None
    assert ic.link_of(by["mpos 5 000, mtid 1, from contig 0"], [lc.CLENS[0]] * 2, lc.MIN_MAPQ) is not None
    assert pk.link_of(by["mpos 5 000, mtid 1, from contig 1"], [lc.CLENS[0]] * 2, lc.MIN_MAPQ) is not None


def test_the_chunks_put_every_case_on_an_edge_of_a_workgroup():
    assert lc.special_slots(1) == [0] and lc.special_slots(1023) == [0, 63, 64, 1022] and lc.special_slots(1024) == [0, 63, 64, 1023]
    assert lc.special_slots(1025) == [0, 63, 64, 1023, 1024] and lc.special_slots(2049) == [0, 63, 64, 1023, 1024, 1087, 1088, 2047, 2048]
    assert sorted({n for n, _, _ in lc.chunks()}) == [1023, 1024, 1025, 2049] and {q for _, _, q in lc.chunks()} == {True, False}
    on_edge = set()
    for n, turn, _ in lc.chunks():
        cases = lc.chunk(n, turn)
        assert len(cases) == n and {c.name for c in cases} == {c.name for c in lc.CASES} | {"plain"}
        assert all(cases[s] is not lc.PLAIN for s in lc.special_slots(n))
        on_edge |= {(cases[s].name, s % 1024) for s in lc.special_slots(n)} | {(cases[n - 1].name, "last")}
    assert {name for name, _ in on_edge} == {c.name for c in lc.CASES}
    assert {lane for _, lane in on_edge} >= {0, 63, 64, 1023, "last"}
    assert [c.name for c in lc.chunk(1, 5)] == [lc.CASES[5].name]


def test_packing_in_both_record_forms_and_the_short_record():
    cases = lc.chunk(1025, 0)
    for qual in (True, False):
        raw, off = lc.pack(cases, qual)
        assert len(off) == len(cases) + 1 and off[0] == 0 and off[-1] == len(raw) and all(int(o) % 4 == 0 for o in off)
        short = 0
        for c, a, b in zip(cases, off[:-1], off[1:]):
            if c.short:
                assert b - a == 28
                short += 1
                continue
            assert b - a >= 32
            tid, pos, _l, mapq, bin_, _n, flag, _ls, mtid, mpos = struct.unpack_from("<iiBBHHHiii", raw.tobytes(), int(a))
            assert (tid, pos, mapq, flag, mtid, mpos) == tuple(c.rec) and (bin_ == 0xFFFF) == (not qual)
        assert short == 2
    assert len(lc.delivered(cases)) == len(cases) - 2
