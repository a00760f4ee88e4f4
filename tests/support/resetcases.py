"""Inputs for the reset of a contig's run of a counted array (im_*_reset: one fill launch, 16-byte stores and a tail) and for the
"generic" look-up that im_set_insert_ranges does once per table.  Built on tests/support/triagecases.py;
tests/test_reset_generic_host.py proves on the CPU that they reach what they name."""
from tests.support import triagecases as tc

# a contig's run holds len + 1 ints: 20 004 and 36 004 bytes (whole 16-byte stores and a tail of one int), 12 bytes (shorter than
# one store), 16 bytes (no tail), 28 bytes (a tail of three ints)
CONTIGS = tc.DEPTH_CONTIGS + [2, 3, 6]


def depth_records():
    """triagecases.depth_cases (its records of contig 2 lie behind that contig's end here) and a few on the short contigs"""
    M = lambda n: ((n, 0),)
    d = tc._drec
    return tc.depth_cases() + [d(2, 0, M(2)), d(2, 1, M(5)), d(2, -1, M(2)), d(3, 0, M(3)), d(3, 2, M(1)), d(4, 0, M(6)), d(4, 3, M(2)), d(4, 5, M(9))]


def _same_bin_extension(name):
    return next(name + a + b for a in "abcdefghij" for b in "abcdefghijklmnopqrstuvwxyz" if tc.djb2_bin(name + a + b) == tc.djb2_bin(name))


GENERIC_EXT = _same_bin_extension("generic")

# (names, ranges, what a record without an RG tag gets: its range, or None where the reference exits); set one after the other on ONE
# context: what the host carries must follow the table
GENERIC_TABLES = [
    (["generic"], [700], 700),
    (["lib1", "generic", "lib10"], [500, 900, 600], 900),
    (["lib1"], [500], None),
    ([], [], None),
    ([GENERIC_EXT, "generic"], [810, 820], 810),          # the older, longer name of the same bin answers (strncmp, the last hit wins)
    (["generic", GENERIC_EXT], [830, 840], 830),
    ([GENERIC_EXT], [850], 850),                          # "generic" itself is not in the table
    (["generi", "lib1"], [860, 500], None),               # a stored name that ends first is no match
    (["generic", "generic"], [870, 880], 870),            # the chain runs from the name added last to the one added first
]


def generic_records():
    """candidates (class 3) without an RG tag, with lib1's, and one whose tag names nobody"""
    return [tc._aux_rec(b"", mapq=60), tc._aux_rec(b"RGZlib1\0", mapq=60), tc._aux_rec(b"MQC\x1e"), tc._aux_rec(b"RGZnobody\0", mapq=60)] \
        + [tc._aux_rec(b"XAZ" + b"k" * 19 + b"\0MQC\x1e") for _ in range(300)]          # more than one workgroup
