"""ONE chunk of records through BOTH link scatters of im_links.hip in one context: the pair links (-M) and the mate links (-T) state the
front of their record rule once and add their own conditions to it, so a front wired to the wrong tail, or a position held against
the wrong contig's length, shows only where the same records go through both.  The records are the hand-made classes of
tests/support/linkcases.py (tests/test_linkcases_host.py pins them without a GPU), padded to chunks around the scatter workgroup of
1 024 records, in both record forms; every expected value comes from the restatements tests/support/pairlinks.py and
tests/support/intercontig.py over the same records.
"""
import numpy as np
import pytest

from tests.support import intercontig as ic
from tests.support import linkcases as lc
from tests.support import pairlinks as pk

pytestmark = pytest.mark.gpu


class Device:
    """one context over the two contigs with both link tables enabled"""

    def __init__(self):
        from indelminer_amd import capi
        self.capi = capi
        rng = np.random.default_rng(11)
        self.ctx = capi.Context(0)
        self.ctx.set_reference([bytes(rng.choice(np.frombuffer(b"ACGT", np.uint8), n)) for n in lc.CLENS])
        self.ctx.pairlink_enable(lc.MIN_MAPQ, 12)
        self.ctx.matelink_enable(lc.MIN_MAPQ, 12)
        self.keep = []

    def scatter_both(self, cases, qual):
        raw, off = lc.pack(cases, qual)
        d_raw = self.capi.DevBuf(self.ctx, len(raw) + 64).upload(raw)
        d_off = self.capi.DevBuf(self.ctx, 4 * len(off)).upload(off)
        self.keep += [d_raw, d_off]
        recs = self.capi.DevRecords(len(off) - 1, d_raw.ptr, d_off.ptr, 0)
        self.ctx.pairlink_scatter(recs)
        self.ctx.matelink_scatter(recs)

    def reset(self):
        self.ctx.pairlink_reset()
        self.ctx.matelink_reset()

    def check(self, records):
        """both tables hold what the restatements make of the records: the stored counts, and every contig's counts and partners"""
        pairs, mates = pk.links_of(records, lc.CLENS, lc.MIN_MAPQ), ic.links_of(records, lc.CLENS, lc.MIN_MAPQ)
        assert pairs and mates
        assert self.ctx.pairlink_stats() == (len(pairs), 0) and self.ctx.matelink_stats() == (len(mates), 0)
        for tid, clen in enumerate(lc.CLENS):
            q = [(k, -5, clen + 5, -5, clen + 5) for k in range(3)] + [(k, p, p, m, m) for t, k, p, m in sorted(set(pairs)) if t == tid]
            got = [int(x) for x in self.ctx.pairlink_count(tid, *[[x[j] for x in q] for j in range(5)], 0)]
            assert got == [pk.count(pairs, lc.CLENS, tid, *x, 0) for x in q], (tid, q, got)
            q = [(k, -5, clen + 5) for k in range(4)] + [(k, p, p) for t, k, p, _, _ in sorted(set(mates)) if t == tid]
            got = [tuple(int(x) for x in row) for row in zip(*self.ctx.matelink_partner(tid, *[[x[j] for x in q] for j in range(3)]))]
            assert got == [ic.partner(mates, lc.CLENS, tid, *x) for x in q], (tid, q, got)

    def close(self):
        for b in self.keep:
            b.free()
        self.ctx.close()


@pytest.fixture(scope="module")
def dev():
    d = Device()
    yield d
    d.close()


@pytest.mark.parametrize("n,turn,qual", lc.chunks())
def test_one_chunk_through_both_scatters(dev, n, turn, qual):
    cases = lc.chunk(n, turn)
    dev.reset()
    dev.scatter_both(cases, qual)
    dev.check(lc.delivered(cases))


def test_every_case_as_a_chunk_of_one_record(dev):
    dev.reset()
    for k in range(len(lc.CASES)):
        dev.scatter_both(lc.chunk(1, k), qual=k % 2 == 0)
    dev.check(lc.delivered(lc.CASES))
