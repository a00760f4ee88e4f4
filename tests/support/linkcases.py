"""What tests/test_gpu_links_together.py and tests/test_linkcases_host.py share: ONE set of hand-made records for BOTH link scatters
(-M's pair links and -T's mate links, im_links.hip), which state the front of their record rule once and add their own conditions to
it.  A front wired to the wrong tail, or a position checked against the wrong contig, shows only where one chunk goes through both
scatters: here every class of record that the two rules treat differently stands in one chunk.

The contigs are 20 000 and 2 000 bases: a position between the two lengths is inside one and outside the other.  Every case states by
hand whether it is a pair link and whether it is a mate link; tests/test_linkcases_host.py holds the restatements
(tests/support/pairlinks.py, tests/support/intercontig.py) to that, and the GPU test holds the kernels to the restatements.
"""
from collections import namedtuple

import numpy as np

from tests.support import pairlinks as pk
from tests.support.pairlinks import Rec

CLENS = [20_000, 2_000]
MIN_MAPQ = 10
PAIRED, PROPER, REV, MREV, FIRST, SECOND = 0x1, 0x2, 0x10, 0x20, 0x40, 0x80
EXCLUDED_BITS = (0x4, 0x8, 0x100, 0x200, 0x400, 0x800)
CORE = 32                               # bytes of a record's core; a record shorter than that stores nothing
LANES = (0, 63, 64, 1023)               # of a scatter workgroup of 1 024 records: the first wave's ends, the second's start, the last lane
SIZES = (1023, 1024, 1025, 2049)        # records of a chunk (and 1: singles below): around one workgroup, and two with a partial third

# pair, mate: whether the record is a pair link, a mate link; short: delivered with 28 of its bytes
Case = namedtuple("Case", "name rec pair mate short")
PLAIN = Case("plain", Rec(0, 100, 60, PAIRED | PROPER | MREV | FIRST, 0, 400), False, False, False)


def _cases():
    out = []

    def add(name, rec, pair=False, mate=False, short=False):
        out.append(Case(name, rec, pair, mate, short))

    ev = PAIRED | REV | FIRST                                           # everted when the mate is on the same contig; kind 1 of the mate links
    add("same contig, everted", Rec(0, 1_000, 60, ev, 0, 1_400), pair=True)
    add("same contig, forward", Rec(0, 1_300, 60, PAIRED | FIRST, 0, 1_700), pair=True)
    add("same contig, reverse", Rec(1, 300, 60, PAIRED | REV | MREV | SECOND, 1, 700), pair=True)
    add("same contig, normal", Rec(0, 1_600, 60, PAIRED | MREV | FIRST, 0, 1_900))
    for tid in (0, 1):
        for kind in range(4):
            flag = PAIRED | (REV if kind & 1 else 0) | (MREV if kind & 2 else 0) | (FIRST if tid == 0 else SECOND)
            add("inter-contig, kind %d, from contig %d" % (kind, tid), Rec(tid, 900 + 300 * kind + 50 * tid, 60, flag, 1 - tid, 1_500 - 200 * kind), mate=True)
    add("mtid -1", Rec(0, 3_000, 60, ev, -1, 3_400))
    add("mtid n_contigs", Rec(0, 3_100, 60, ev, len(CLENS), 100))        # length[mtid] does not exist
    add("mpos 5 000, mtid 1, from contig 0", Rec(0, 4_000, 60, ev, 1, 5_000))                 # inside contig 0, which is not the mate's
    add("mpos 5 000, mtid 0, from contig 0", Rec(0, 4_000, 60, ev, 0, 5_000), pair=True)
    add("mpos 5 000, mtid 0, from contig 1", Rec(1, 400, 60, ev, 0, 5_000), mate=True)        # outside contig 1, which is not the mate's
    add("mpos 5 000, mtid 1, from contig 1", Rec(1, 400, 60, ev, 1, 5_000))
    for m in (CLENS[1], CLENS[1] + 1):                                  # the last position a contig has (its length) and the one behind
        add("same contig, mpos %d" % m, Rec(1, 300, 60, ev, 1, m), pair=m == CLENS[1])
        add("inter-contig, mpos %d" % m, Rec(0, 500, 60, ev, 1, m), mate=m == CLENS[1])
    add("same contig, pos -1", Rec(0, -1, 60, ev, 0, 300))
    add("inter-contig, pos -1", Rec(0, -1, 60, ev, 1, 300))
    add("same contig, both behind the contig", Rec(1, 2_500, 60, ev, 1, 2_600))
    add("pos == mpos, first in pair", Rec(0, 6_000, 60, PAIRED | REV | FIRST, 0, 6_000), pair=True)
    add("pos == mpos, second in pair", Rec(0, 6_000, 60, PAIRED | REV | SECOND, 0, 6_000))
    for q in (MIN_MAPQ - 1, MIN_MAPQ):
        add("same contig, mapq %d" % q, Rec(0, 7_000, q, ev, 0, 7_400), pair=q >= MIN_MAPQ)
        add("inter-contig, mapq %d" % q, Rec(0, 7_100, q, ev, 1, 700), mate=q >= MIN_MAPQ)
    for bit in EXCLUDED_BITS:
        add("same contig, flag 0x%x" % bit, Rec(0, 8_000, 60, ev | bit, 0, 8_400))
        add("inter-contig, flag 0x%x" % bit, Rec(1, 800, 60, ev | bit, 0, 8_400))
    add("same contig, not paired", Rec(0, 8_500, 60, REV | FIRST, 0, 8_900))
    add("inter-contig, not paired", Rec(1, 850, 60, REV | FIRST, 0, 8_900))
    add("same contig, 28 bytes", Rec(0, 9_000, 60, ev, 0, 9_400), short=True)
    add("inter-contig, 28 bytes", Rec(0, 9_100, 60, ev, 1, 900), short=True)
    return out


CASES = _cases()


def special_slots(n):
    """the records of a chunk of n that sit on LANES of a workgroup, and the last one"""
    return sorted({g + lane for g in range(0, n, 1024) for lane in LANES if g + lane < n} | {n - 1})


def chunk(n, turn):
    """[Case] * n: CASES[turn], CASES[turn + 1] .. (going round) on the special slots, every other case on ordinary lanes in between
    (where there is room: not in a chunk of one), plain records elsewhere"""
    out = [PLAIN] * n
    slots = special_slots(n)
    placed = [(turn + j) % len(CASES) for j in range(len(slots))]
    for s, k in zip(slots, placed):
        out[s] = CASES[k]
    rest = [c for k, c in enumerate(CASES) if k not in placed]
    free = [s for s in range(n) if s not in slots]
    if len(free) >= len(rest):
        for j, c in enumerate(rest):
            out[free[j * (len(free) // len(rest))]] = c
    return out


def chunks():
    """[(n, turn, qual)]: every size three times, in either record form, the turn going on so that every case comes to a special slot"""
    out, turn = [], 0
    for qual in (True, False, True):
        for n in SIZES:
            out.append((n, turn, qual))
            turn += len(special_slots(n))
    return out


def pack(cases, qual=True):
    """the device layout of pairlinks.pack_records, a short case cut to 28 bytes"""
    blob, off, packed = bytearray(), [0], {}
    for c in cases:
        if c.rec not in packed:
            packed[c.rec] = pk.pack_records([c.rec], qual)[0].tobytes()
        blob += packed[c.rec][:CORE - 4] if c.short else packed[c.rec]
        off.append(len(blob))
    return np.frombuffer(bytes(blob), np.uint8).copy(), np.array(off, np.uint32)


def delivered(cases):
    """the records the restatements are asked about: a short one is no record"""
    return [c.rec for c in cases if not c.short]
