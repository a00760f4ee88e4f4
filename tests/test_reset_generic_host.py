"""The inputs of tests/test_gpu_reset_generic.py reach what they claim to reach, through the CPU oracle alone."""
from tests.support import oraclebind as ob
from tests.support import resetcases as rc
from tests.support import triagecases as tc


def test_runs_have_every_tail_and_one_is_shorter_than_a_store():
    runs = [4 * (clen + 1) for clen in rc.CONTIGS]
    assert {r % 16 for r in runs} == {0, 4, 12} and min(runs) < 16 and 16 in runs and max(runs) > 16 * 1024
    raw, off = tc.batch(rc.depth_records())
    for tid, clen in enumerate(rc.CONTIGS):
        d = ob.depth_of(raw, off, tid, clen)
        assert d[0] > 0 and d[clen - 1] > 0, tid            # the first and the last int of every run are in use


def test_generic_tables_say_what_they_name():
    recs = rc.generic_records()
    raw, off = tc.batch(recs)
    assert len(recs) > 256
    assert tc.djb2_bin(rc.GENERIC_EXT) == tc.djb2_bin("generic") and rc.GENERIC_EXT.startswith("generic")
    seen = set()
    for names, ranges, want in rc.GENERIC_TABLES:
        tri = ob.triage_records(raw, off, names, ranges)
        no_rg = [t for (t, _), r in zip(tri, recs) if b"RGZ" not in r]
        assert len(no_rg) > 256
        for t in no_rg:
            assert (t.cls, t.range_max) == ((16, 0) if want is None else (3, want)), (names, t.cls, t.range_max)
        seen.add(want)
        lib1 = tri[1][0]
        assert (lib1.cls, lib1.range_max) == ((3, 500) if "lib1" in names else (16, 0))
        assert tri[3][0].cls == 16
    assert None in seen and len(seen) >= 7
    # consecutive tables differ in what "generic" gives: a value carried over from the table before would show
    wants = [w for _, _, w in rc.GENERIC_TABLES]
    assert all(a != b or a is None for a, b in zip(wants[:-1], wants[1:])) and wants[2] is None and wants[3] is None and wants[4] is not None
