"""The CPU oracle against the real reference on seeded fuzz inputs (tests/support/refcases.py): the reference's answers
are committed (tests/golden/ref_fuzz.json, made by tests/golden/make_golden_fuzz.py from the reference compiled in place,
oracle/_ref/libimref.so; tests/golden/ref_lowcomplexity.json, made by make_golden_lowcomplexity.py, for the low-complexity
inputs of tests/support/lowcomplexity.py), so the check runs everywhere.  Where that library exists, the reference is also called live
and must still give the committed answers."""
import ctypes as C

import pytest

from tests.support import compare, golden, lowcomplexity as lc, oraclebind as ob, refbind, refcases

GOLD = golden.load(refcases.GOLDEN_NAME)["cases"]
LOWC = golden.load(lc.GOLDEN_NAME)["realign"]


def _live(k, g, maxdel, eth):
    if not refbind.available():
        return None
    R = refbind.Ref()
    R.set_params(k, g, maxdel, eth)
    return R


@pytest.mark.parametrize("k,g,seed", refcases.FUZZ)
def test_fuzz_against_reference(k, g, seed):
    maxdel, contig, cases = refcases.fuzz(seed)
    want = GOLD[refcases.key("fuzz", k, g, seed)]
    assert len(want) == len(cases)
    eth = max(k, 10)
    R = _live(k, g, maxdel, eth)
    P = ob.params(k, g, maxdel, eth)
    cb = contig.encode()
    buf = C.create_string_buffer(cb)
    n_ev = 0
    for c, ro in zip(cases, want):
        read = c["read"]
        st, res = ob.realign(P, cb, len(cb), c["anchor"], c["range_max"], read)
        if st == -1:             # the reference would exit(1) inside this process (forceassert): nothing to compare
            continue
        assert ro != "abort", c
        if R is not None:
            assert refcases.plain(R.realign(buf, c["anchor"], c["range_max"], read)) == ro, c
        msg = compare.ref_vs_oracle(ro, st, res, read)
        assert msg is None, msg
        n_ev += 0 if ro is None else len(ro)
    assert n_ev > 5 or k < 4          # two- and three-base seeds are never unique in a 100-base read: no band, no evidence


@pytest.mark.parametrize("k,g,seed", refcases.LEFT_EDGE)
def test_left_edge_bands_against_reference(k, g, seed):
    """Pins the left-edge behaviour of local_align's reverse pass (tests/support/leftedge.py): bands without a single
    k-mer vote that hang off the window's left edge, for -g 0 and -g > 0 (where endj - startj = -g != 0 lets the
    result reach ALIGN).  The oracle -- and through tests/test_gpu_realign.py the HIP kernels -- must give exactly
    what the reference compiled from its own sources gives, byte in front of the window included."""
    from tests.support import leftedge
    R = _live(k, g, 1000, 10)
    P = ob.params(k, g, 1000, 10)
    contig, cases = leftedge.cases(seed)
    want = GOLD[refcases.key("left_edge", k, g, seed)]
    assert len(want) == len(cases)
    cb = contig.encode()
    # one byte in front of the contig that never equals a base: what the reference reads for a window at the contig's start
    raw = C.create_string_buffer(b"#" + cb)
    buf = C.cast(C.addressof(raw) + 1, C.POINTER(C.c_char * (len(cb) + 1))).contents
    seen = 0
    for c, ro in zip(cases, want):
        st, res = ob.realign(P, cb, len(cb), c["anchor"], c["range_max"], c["read"])
        if st == -1:
            continue
        assert ro != "abort", c
        if R is not None:
            assert refcases.plain(R.realign(buf, c["anchor"], c["range_max"], c["read"])) == ro, c
        msg = compare.ref_vs_oracle(ro, st, res, c["read"])
        assert msg is None, (c, msg)
        seen += 1
    assert seen > 60


@pytest.mark.parametrize("k,g,seed", lc.REALIGN_RUNS)
def test_low_complexity_against_reference(k, g, seed):
    """Reads whose indel sits in a homopolymer or a short tandem repeat (tests/support/lowcomplexity.py): k-mers that are not
    unique in the piece, tied diagonals, runs of equally good cut points, equal-score paths.  Not vacuous: about half the
    cuts lie in a repeat, the reference returns evidence for a good part of the reads, hardly any read is left out."""
    contig, cases, share = lc.realign_cases(seed)
    want = LOWC[refcases.key("lowc", k, g, seed)]
    assert len(want) == len(cases) == 150
    assert share >= 0.4
    eth = max(k, 10)
    R = _live(k, g, 1000, eth)
    P = ob.params(k, g, 1000, eth)
    cb = contig.encode()
    raw = C.create_string_buffer(b"#" + cb)
    buf = C.cast(C.addressof(raw) + 1, C.POINTER(C.c_char * (len(cb) + 1))).contents
    n_ev = n_abort = 0
    for c, ro in zip(cases, want):
        read = c["read"]
        ro = lc.with_bases(ro, read)         # stored without the segments' bases
        st, res = ob.realign(P, cb, len(cb), c["anchor"], c["range_max"], read)
        assert (st == -1) == (ro == "abort"), c
        if st == -1:
            n_abort += 1
            continue
        if R is not None:
            assert refcases.plain(R.realign(buf, c["anchor"], c["range_max"], read)) == ro, c
        msg = compare.ref_vs_oracle(ro, st, res, read)
        assert msg is None, (c, msg)
        n_ev += 0 if ro is None else len(ro)
    assert n_ev >= 30, n_ev
    assert n_abort <= len(cases) // 10, n_abort
