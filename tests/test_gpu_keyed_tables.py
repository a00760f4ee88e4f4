"""The clip-tail table (-V), the pair-link table (-M) and the mate-link table (-T) side by side in ONE context: all three are the keyed
table of im_keyed.hpp behind one set of helpers in im_capi.hip (enable, ready, scatter, reset, stats, the answers with their overflow
value), which take the table they work on as an argument.  A helper handed another table passes every test that enables one table
alone; here each table is filled, overflowed and reset while the other two must keep their entries, their counters and their answers.

Every expected value comes from the plain restatements: tests/support/cliptails.py (verify), tests/support/facingpiles.py (the
consensus, which is written over cliptails.py's entries), tests/support/pairlinks.py (count) and tests/support/intercontig.py
(partner).  All three tables have 64 slots, and the keys are chosen as tests/test_gpu_cliptail.py, tests/test_gpu_pairlink.py and
tests/test_gpu_intercontig.py choose theirs: home slots on the table's last slots and its first, so that probe runs collide and wrap.
"""
import numpy as np
import pytest

from tests.support import cliptails as ct
from tests.support import facingpiles as fp
from tests.support import intercontig as ic
from tests.support import pairlinks as pk
from tests.support.clipcounts import LEFT, RIGHT

pytestmark = pytest.mark.gpu

CLENS = [20_000, 2_000]
NONE = 0xFFFFFFFF
MIN_COVER = 2
HOMES = (63, 62, 63, 61, 0)            # of the five keys of every table; the second 63 is another key of that home slot


def contigs(seed=5):
    rng = np.random.default_rng(seed)
    return [bytes(rng.choice(np.frombuffer(b"ACGT", np.uint8), n)) for n in CLENS]


def link_home(tid, bucket, kind):
    """the first of 64 slots a link of this key probes (include/indelminer_amd.h, "Pair links", states the hash)"""
    key = (1 << 63) | (tid << 26) | (bucket << 2) | kind
    return ((key * ct.HASH_MUL) & (2**64 - 1)) >> 58


def keys_at(homes):
    """one key per entry of HOMES out of {home slot: [keys]}, the k-th key of a home slot for its k-th mention"""
    seen, out = {}, []
    for h in HOMES:
        out.append(homes[h][seen.get(h, 0)])
        seen[h] = seen.get(h, 0) + 1
    return out


def tail_keys():
    homes = {}
    for p in range(1_000, 19_000):
        for side in (RIGHT, LEFT):
            homes.setdefault(ct.home_slot(0, side, p, 6), []).append((side, p))
    return keys_at(homes)


def link_keys():
    homes = {}
    for bucket in range(CLENS[0] // 256 - 2):           # mpos, up to 400 bases behind the bucket, stays on the contig
        for kind in range(3):
            homes.setdefault(link_home(0, bucket, kind), []).append((bucket, kind))
    return keys_at(homes)


def mate_keys():
    homes = {}
    for bucket in range(CLENS[0] // 256 - 2):
        for kind in range(4):
            homes.setdefault(ic.home_slot(0, bucket, kind, 6), []).append((bucket, kind))
    return keys_at(homes)


def tail_table(refs, keys, per_key, seed):
    """{(tid, side, position): [bases]} and the partner position of every key: per_key entries each, most of them what the reference
    holds behind the partner at a shift of 0 .. 3, with 0 .. 3 bases changed and 1 .. 32 bases long"""
    rng = np.random.default_rng(seed)
    table, partner = {}, {}
    for tid, side, p in keys:
        other = p + 500 if side == RIGHT else p - 500
        for _ in range(per_key):
            n, s = int(rng.integers(1, 33)), int(rng.integers(0, 4))
            start, step = (other + s, 1) if side == RIGHT else (other - 1 - s, -1)
            bases = [b"ACGT".index(refs[tid][start + step * i:start + step * i + 1]) for i in range(n)]
            for i in rng.integers(0, n, int(rng.integers(0, 4))):
                bases[int(i)] = (bases[int(i)] + 1) % 4
            table.setdefault((tid, side, p), []).append(tuple(bases))
        partner[(tid, side, p)] = other
    return table, partner


def links_at(keys, per_key):
    """[(tid, kind, pos, mpos)]: per_key links in the bucket of every key, interleaved so that the runs lie in between each other"""
    return [(0, kind, 256 * bucket + 7 * i, 256 * bucket + 300 + 11 * i) for i in range(per_key) for bucket, kind in keys]


def mates_at(keys, per_key):
    """[(tid, kind, pos, mtid, mpos)]: per_key links in the bucket of every key, interleaved, their partners on contig 1 -- a key's
    mates within two neighbouring cells, the keys' cells apart"""
    return [(0, kind, 256 * bucket + 7 * i, 1, (300 * j + 13 * i) % CLENS[1]) for i in range(per_key) for j, (bucket, kind) in enumerate(keys)]


class Both:
    """one context over the two contigs with the three tables enabled at 64 slots"""

    def __init__(self, refs):
        from indelminer_amd import capi
        self.refs = refs
        self.ctx = capi.Context(0)
        self.ctx.set_reference(refs)
        self.ctx.cliptail_enable(20, 10, 6)
        self.ctx.pairlink_enable(10, 6)
        self.ctx.matelink_enable(10, 6)

    def add_tails(self, table):
        for tid in range(len(CLENS)):
            ent = [(p, side, b) for (t, side, p), lst in table.items() if t == tid for b in lst]
            self.ctx.cliptail_add(tid, [e[0] for e in ent], [e[1] for e in ent], [len(e[2]) for e in ent],
                                  np.array([ct.planes_of(e[2]) for e in ent], np.uint32).reshape(-1, 2))

    def add_links(self, links):
        for tid in range(len(CLENS)):
            mine = [x for x in links if x[0] == tid]
            self.ctx.pairlink_add(tid, [p for _, _, p, _ in mine], [m for _, _, _, m in mine], [k for _, k, _, _ in mine])

    def add_mates(self, mates):
        for tid in range(len(CLENS)):
            mine = [x for x in mates if x[0] == tid]
            self.ctx.matelink_add(tid, [p for _, _, p, _, _ in mine], [mt for _, _, _, mt, _ in mine], [m for _, _, _, _, m in mine], [k for _, k, _, _, _ in mine])

    def mate_answers(self, mates, keys):
        """the partners of every key's bucket, of a window over all of them and of one single link, and what the restatement says"""
        queries = [(kind, 256 * bucket, 256 * bucket + 255) for bucket, kind in keys]
        queries += [(kind, -5, CLENS[0] + 5) for kind in range(4)] + [(keys[0][1], 256 * keys[0][0], 256 * keys[0][0])]
        got = [tuple(int(x) for x in row) for row in zip(*self.ctx.matelink_partner(0, *[[q[k] for q in queries] for k in range(3)]))]
        return got, [ic.partner(mates, CLENS, 0, *q) for q in queries]

    def tail_answers(self, table, partner):
        """(verify, consensus) of every key of the table on contig 0, and what the restatements say"""
        keys = sorted(k for k in table if k[0] == 0)
        pr = [p if side == RIGHT else partner[(t, side, p)] for t, side, p in keys]
        pl = [partner[(t, side, p)] if side == RIGHT else p for t, side, p in keys]
        got_v = [tuple(int(x) for x in row) for row in zip(*self.ctx.cliptail_verify(0, pr, pl, 32))]
        got_c = [tuple(int(x) for x in row) for row in zip(*self.ctx.cliptail_consensus(0, [p for _, _, p in keys], [s for _, s, _ in keys], MIN_COVER))]
        want_v = ct.answer_many(table, self.refs[0], 0, pr, pl, 32)
        want_c = [fp.answer(table, 0, p, side, MIN_COVER, CLENS[0]) for _, side, p in keys]
        return (got_v, got_c), (want_v, want_c)

    def link_answers(self, links, keys):
        """the counts of every key's bucket, of a window over all of them and of one single link, and what the restatement says"""
        queries = [(kind, 256 * bucket, 256 * bucket + 255, 0, CLENS[0]) for bucket, kind in keys]
        queries += [(kind, -5, CLENS[0] + 5, -5, CLENS[0] + 5) for kind in range(3)] + [(keys[0][1], 256 * keys[0][0], 256 * keys[0][0], 0, CLENS[0])]
        got = [[int(x) for x in self.ctx.pairlink_count(0, *[[q[k] for q in queries] for k in range(5)], sep)] for sep in (0, 305)]
        want = [[pk.count(links, CLENS, 0, *q, sep) for q in queries] for sep in (0, 305)]
        return got, want


@pytest.mark.parametrize("overflowing", ["links", "tails", "mates"])
def test_one_table_overflows_and_is_reset_beside_the_other(overflowing):
    refs = contigs()
    tkeys, lkeys, mkeys = [(0, side, p) for side, p in tail_keys()], link_keys(), mate_keys()
    dev = Both(refs)
    try:
        if overflowing == "links":
            # 20 tail entries, 40 links, 20 mate links: the link table keeps 32 and answers nothing, the other two are whole
            table, partner = tail_table(refs, tkeys, 4, 41)
            links, mates = links_at(lkeys, 8), mates_at(mkeys, 4)
            dev.add_tails(table); dev.add_links(links); dev.add_mates(mates)
            assert dev.ctx.cliptail_stats() == (20, 0) and dev.ctx.pairlink_stats() == (32, 8) and dev.ctx.matelink_stats() == (20, 0)
            got, want = dev.tail_answers(table, partner)
            assert got == want and any(v[0] + v[1] > 0 for v in want[0]) and any(c[1] > 0 for c in want[1])
            got_m, want_m = dev.mate_answers(mates, mkeys)
            assert got_m == want_m and all(m[2] > 0 for m in want_m[:5])
            got_l, want_l = dev.link_answers(links, lkeys)
            assert got_l == [[NONE] * len(want_l[0])] * 2
            # the link table alone is reset and takes 5 links: its answers are exact again, the other tables' have not moved
            dev.ctx.pairlink_reset()
            few = links_at(lkeys, 1)
            dev.add_links(few)
            assert dev.ctx.pairlink_stats() == (5, 0) and dev.ctx.cliptail_stats() == (20, 0) and dev.ctx.matelink_stats() == (20, 0)
            got_l, want_l = dev.link_answers(few, lkeys)
            assert got_l == want_l and sum(want_l[0]) > 0
            assert dev.tail_answers(table, partner) == (want, want)
            assert dev.mate_answers(mates, mkeys) == (want_m, want_m)
        elif overflowing == "tails":
            # the roles swapped: 40 tail entries, 20 links, 20 mate links
            table, partner = tail_table(refs, tkeys, 8, 43)
            links, mates = links_at(lkeys, 4), mates_at(mkeys, 4)
            dev.add_links(links); dev.add_mates(mates); dev.add_tails(table)
            assert dev.ctx.cliptail_stats() == (32, 8) and dev.ctx.pairlink_stats() == (20, 0) and dev.ctx.matelink_stats() == (20, 0)
            got_l, want_l = dev.link_answers(links, lkeys)
            assert got_l == want_l and sum(want_l[0]) > 0
            got_m, want_m = dev.mate_answers(mates, mkeys)
            assert got_m == want_m and all(m[2] > 0 for m in want_m[:5])
            got, _ = dev.tail_answers(table, partner)
            assert got == ([(NONE, NONE, -1, NONE, NONE)] * len(tkeys), [(NONE,) * 5] * len(tkeys))
            # the tail table alone is reset and takes 5 entries
            dev.ctx.cliptail_reset()
            few, partner = tail_table(refs, tkeys, 1, 44)
            dev.add_tails(few)
            assert dev.ctx.cliptail_stats() == (5, 0) and dev.ctx.pairlink_stats() == (20, 0) and dev.ctx.matelink_stats() == (20, 0)
            got, want = dev.tail_answers(few, partner)
            assert got == want and all(v[3] + v[4] == 1 for v in want[0])
            assert dev.link_answers(links, lkeys) == (want_l, want_l)
            assert dev.mate_answers(mates, mkeys) == (want_m, want_m)
        else:
            # 20 tail entries, 20 links, 40 mate links: the mate table keeps 32 and every partner answer is blank
            table, partner = tail_table(refs, tkeys, 4, 41)
            links, mates = links_at(lkeys, 4), mates_at(mkeys, 8)
            dev.add_mates(mates); dev.add_tails(table); dev.add_links(links)
            assert dev.ctx.cliptail_stats() == (20, 0) and dev.ctx.pairlink_stats() == (20, 0) and dev.ctx.matelink_stats() == (32, 8)
            got, want = dev.tail_answers(table, partner)
            assert got == want and any(v[0] + v[1] > 0 for v in want[0]) and any(c[1] > 0 for c in want[1])
            got_l, want_l = dev.link_answers(links, lkeys)
            assert got_l == want_l and sum(want_l[0]) > 0
            got_m, want_m = dev.mate_answers(mates, mkeys)
            assert got_m == [(NONE, -1, NONE, -1, -1)] * len(want_m)
            # the mate table alone is reset and takes 5 links: its answers are exact again, the other tables' have not moved
            dev.ctx.matelink_reset()
            few = mates_at(mkeys, 1)
            dev.add_mates(few)
            assert dev.ctx.matelink_stats() == (5, 0) and dev.ctx.cliptail_stats() == (20, 0) and dev.ctx.pairlink_stats() == (20, 0)
            got_m, want_m = dev.mate_answers(few, mkeys)
            assert got_m == want_m and all(m[:3] == (1, 1, 1) for m in want_m[:5])
            assert dev.tail_answers(table, partner) == (want, want)
            assert dev.link_answers(links, lkeys) == (want_l, want_l)
    finally:
        dev.ctx.close()
