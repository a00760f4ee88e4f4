"""What tests/test_gpu_many_queries.py and tests/test_manyqueries_host.py share: plans of queries for the kernels that give one wave to a
query and take the next query in a loop past a fixed grid (wave_grid of im_keyed.hpp: 2 048 workgroups of 4 waves, so query q goes to
wave q mod 8 192 and q + 8 192 is that wave's SECOND TRIP through the body).  What a second trip can get wrong -- an accumulator
declared one brace too far out, an LDS table that still holds the previous query, a reset skipped by a continue -- shows only where a
wave meets two queries of different kinds one after the other, so a plan is D = 97 hand-classed base queries (a prime that does not
divide 8 192), tiled: query i is base[i % D], and the expected answers are the restatements' answers to the D base queries, tiled the same
way with numpy.  The base index moves by 8 192 mod 97 = 44 from one trip of a wave to the next, so the classes are laid out along the
chain 0, 44, 88, 35 .. in the orders in which leftover state would show; tests/test_manyqueries_host.py pins that.

The classes:  heavy     a key whose entries fill more than one 64-slot batch of keyed_walk (65 or more; 130 or more for the clip tails
                        and the overlap)
              ordinary  a site of a few to a few tens of entries
              empty     a window or a key that holds nothing
              clipped   an interval that is empty after the clip to the contig (a1 < 0, a0 > length), a position outside the contig
              wide      a window of 65 535 bases over 257 buckets, where the entry takes a window per query
              multi, single   (mate links) links that vote for several cells, then for one
              unknown, twice  (-H) a junction none of whose links states an overlap; one whose two directions count the same links

Every answer comes from the plain restatements (pairlinks.count, intercontig.partner and .junction, splitlinks.count,
splitoverlap.junction_summary, junctionpairs.junction_pairs, cliptails.answer, facingpiles.answer), once per distinct base query.
Everything is an integer and every comparison is exact.
"""
import numpy as np

from tests.support import cliptails as ct
from tests.support import facingpiles as fp
from tests.support import intercontig as ic
from tests.support import junctionpairs as jp
from tests.support import pairlinks as pk
from tests.support import splitlinks as sl
from tests.support import splitoverlap as so

D = 97
TRIP = 8192                                     # the waves of wave_grid()'s largest grid
STEP = TRIP % D                                 # 44: how far the base index moves from one trip of a wave to its next
SIZES = [8192, 8193, 16385, 20011]              # exactly one trip; one wave on a second trip; one wave on a third; a ragged last trip
CLENS = [150_000, 60_000, 20_000]
QUIET = 100_000                                 # nothing is stored on contig 0 from here on: the empty windows lie there
MIN_SEP, OVERLAP_WINDOW, MIN_COVER = pk.MIN_SEP, so.WINDOW, fp.MIN_COVER
HEAVY_LINKS, HEAVY_TAILS = 65, 130
LOG2_SLOTS = {"pair": 13, "mate": 13, "split": 12, "tail": 14}     # half of the slots are usable: no fill below overflows its table

# along the chain: every class is followed by the class behind it in this list, going round -- but for the two slots that layout()
# overwrites (base 1 and base 1 + STEP), whose neighbours along the chain tests/test_manyqueries_host.py pins through the transitions
PATTERN = ["heavy", "empty", "heavy", "clipped", "ordinary", "wide", "ordinary", "multi", "single", "unknown", "twice"]
# the orders in which leftover state would show; the host test asserts that they occur over SIZES
TRANSITIONS = [("heavy", "empty"), ("heavy", "clipped"), ("empty", "heavy"), ("clipped", "ordinary"), ("wide", "ordinary"), ("multi", "single")]


def layout():
    """the class of every base index: PATTERN along the chain 0, STEP, 2 STEP ..; base 1 and base 1 + STEP, which the rotated call of
    8 193 gives to the one wave that makes a second trip, are heavy and empty"""
    names = [None] * D
    for j in range(D):
        names[(STEP * j) % D] = PATTERN[j % len(PATTERN)]
    j1 = next(j for j in range(D) if (STEP * j) % D == 1)
    names[1], names[(1 + STEP) % D] = "heavy", "empty"
    assert PATTERN[(j1 + 2) % len(PATTERN)] in ("heavy", "ordinary")        # what follows the empty one stays a class that holds entries
    return names


def tile(base, nq):
    """base[i % D] for i < nq"""
    assert len(base) == D
    if isinstance(base, np.ndarray):
        return base[np.arange(nq) % D]
    return [base[i % D] for i in range(nq)]


def rotate(base, by=1):
    """the base set going round by `by`: other waves make the second trip"""
    if isinstance(base, np.ndarray):
        return np.roll(base, -by, axis=0)
    return list(base[by:]) + list(base[:by])


def trips(nq):
    """per wave that makes more than one trip through nq queries: (i % D, (i + 8192) % D[, (i + 16384) % D]), the base indices it
    meets, in order"""
    out = []
    for w in range(min(TRIP, nq)):
        mine = [i % D for i in range(w, nq, TRIP)]
        if len(mine) > 1:
            out.append(tuple(mine))
    return out


def transitions(classes, nq, by=0):
    """{(class, next class)} that some wave meets on consecutive trips through nq queries of the base set rotated by `by`"""
    seen = set()
    for t in trips(nq):
        for a, b in zip(t, t[1:]):
            seen.add((classes[(a + by) % D], classes[(b + by) % D]))
    return seen


def first_mismatches(got, want, limit=6):
    """[(i, i % D, trip i // 8192, got, want)] of the first rows at which two tiled columns differ"""
    bad = np.nonzero(np.asarray(got) != np.asarray(want))[0][:limit]
    return [(int(i), int(i) % D, int(i) // TRIP, int(got[i]), int(want[i])) for i in bad]


_REFS = []


def refs():
    """the contigs' bytes: random ACGT with a few N"""
    if not _REFS:
        rng = np.random.default_rng(97)
        for n in CLENS:
            a = rng.choice(np.frombuffer(b"ACGT", np.uint8), n)
            a[rng.integers(0, n, n // 5_000)] = ord("N")
            _REFS.append(a.tobytes())
    return _REFS


class Plan:
    """name; classes[D]; base[D] query tuples; kinds: the numpy type of every query column; out_kinds: of every answer column; answer:
    query -> answer tuple (the restatement); and whatever its builder adds for the fill"""

    def __init__(self, name, classes, base, kinds, out_kinds, answer, **more):
        assert len(classes) == len(base) == D
        self.name, self.classes, self.base, self.kinds, self.out_kinds, self.answer = name, classes, base, kinds, out_kinds, answer
        self._answers = None
        vars(self).update(more)

    def answers(self):
        """the restatement's answer to every base query, each distinct query asked once"""
        if self._answers is None:
            done = {}
            for q in self.base:
                if q not in done:
                    done[q] = tuple(int(x) for x in self.answer(q))
            self._answers = [done[q] for q in self.base]
        return self._answers

    def columns(self, nq, by=0):
        """(query columns, expected answer columns) of the call of nq queries, the base set rotated by `by`"""
        idx = (np.arange(nq) + by) % D
        qs = [np.array([q[k] for q in self.base], t)[idx] for k, t in enumerate(self.kinds)]
        want = [np.array([a[k] for a in self.answers()], np.int64).astype(t)[idx] for k, t in enumerate(self.out_kinds)]
        return [np.ascontiguousarray(c) for c in qs], want


def _classes(keep):
    """the layout with the classes a plan does not have turned ordinary"""
    return [c if c in keep else "ordinary" for c in layout()]


COMMON = ("heavy", "ordinary", "empty", "clipped")
N_SITES, N_HEAVY = 40, 4


def _site_pos(s):
    return 2_000 + 2_100 * s                    # 40 sites of contig 0 below 84 000


def _heavy_pos(h):
    return 91_136 + 1_024 * h                   # the start of a bucket (a multiple of 256), below QUIET with all that lies around it


def _wide(k):
    a0 = 20_001 + 13 * k
    return a0, a0 + 65_535


# ---------------------------------------------------------------------- the pair links (-M, -E)

def pair_links():
    """([(tid, kind, pos, mpos)], sites [(tid, kind, a, b)], heavy sites): per site 4 .. 40 links of its kind within 300 bases of a and
    of b and three of the next kind among them; a heavy site keeps 70 .. 190 links of one kind in ONE bucket"""
    rng = np.random.default_rng(1)
    links, sites, heavy = [], [], []
    for s in range(N_SITES + 20):
        tid = 0 if s < N_SITES else 1
        a = _site_pos(s) if tid == 0 else 1_500 + 2_500 * (s - N_SITES)
        b, kind = a + 600 + 37 * s, s % 4
        for _ in range(int(rng.integers(4, 41))):
            links.append((tid, kind, a + int(rng.integers(-300, 301)), b + int(rng.integers(-300, 301))))
        for _ in range(3):
            links.append((tid, (kind + 1) % 4, a + int(rng.integers(-300, 301)), b + int(rng.integers(-300, 301))))
        sites.append((tid, kind, a, b))
    for h in range(N_HEAVY):
        a, kind = _heavy_pos(h), h % 4
        for _ in range(70 + 40 * h):
            links.append((0, kind, a + int(rng.integers(0, 256)), a + 700 + int(rng.integers(0, 400))))
        heavy.append((0, kind, a, a + 700))
    return links, sites, heavy


def pairlink_plan():
    """im_pairlink_count on contig 0, min_sep MIN_SEP, kinds 0 .. 3 (the stretched form enabled): (kind, a0, a1, b0, b1) -> (count,)"""
    links, sites, heavy = pair_links()
    rng = np.random.default_rng(11)
    clen = CLENS[0]
    classes = _classes(COMMON + ("wide",))
    base = []
    for k, c in enumerate(classes):
        if c == "heavy":
            _, kind, a, b = heavy[k % N_HEAVY]
            q = (kind, a + int(rng.integers(0, 60)), a + int(rng.integers(200, 500)), b + int(rng.integers(0, 150)), b + int(rng.integers(250, 500)))
        elif c == "empty":
            q = (k % 4, QUIET + 300 * k, QUIET + 300 * k + 500, 0, clen)
        elif c == "clipped":
            q = [(k % 4, -700 - k, -1, 0, clen), (k % 4, clen + 1, clen + 900 + k, 0, clen), (sites[k % N_SITES][1], sites[k % N_SITES][2] - 300, sites[k % N_SITES][2] + 300, -900, -1 - k)][k % 3]
        elif c == "wide":
            q = (k % 4,) + _wide(k) + (0, clen)
        else:
            _, kind, a, b = sites[k % N_SITES]
            q = (kind, a - 200 + int(rng.integers(-150, 151)), a + 200 + int(rng.integers(-150, 151)), b - 250 + int(rng.integers(-100, 101)), b + 250 + int(rng.integers(-100, 101)))
        base.append(q)
    answer = lambda q: (pk.count(links, CLENS, 0, *q, MIN_SEP),)           # the count compares the kind it is given: 3 is one more value
    return Plan("im_pairlink_count", classes, base, (np.uint8, np.int32, np.int32, np.int32, np.int32), (np.uint32,), answer, links=links, heavy=heavy, sites=sites)


# ---------------------------------------------------------------------- the mate links (-T, -E)

def mate_links():
    """([(tid, kind, pos, mtid, mpos)], sites [(kind, a, mtid, b, cells)], heavy sites): the sites of contig 0 send their mates by
    turns into ONE cell of 1 024 bases (single) or into three to six cells of both other contigs (multi); every link has its mirror at the
    mate's contig"""
    rng = np.random.default_rng(2)
    links, sites, heavy = [], [], []

    def put(kind, pos, mtid, mpos):
        links.append((0, kind, pos, mtid, mpos))
        links.append((mtid, (kind >> 1) | ((kind & 1) << 1), mpos, 0, pos))

    for s in range(N_SITES):
        a, kind, mtid = _site_pos(s) + 500, s % 4, 1 + s % 2
        cells = 1 if s % 2 == 0 else 3 + s % 4
        b = 1_024 * (2 + s % 12)                                       # the start of a cell, inside both other contigs with what follows
        for _ in range(int(rng.integers(4, 41))):
            c = int(rng.integers(0, cells))
            mt = mtid if c < 3 else 3 - mtid
            put(kind, a + int(rng.integers(-300, 301)), mt, b + 1_024 * (c % 3) * 2 + int(rng.integers(100, 900)))
        sites.append((kind, a, mtid, b, cells))
    for h in range(N_HEAVY):
        a, kind = _heavy_pos(h), h % 4
        for _ in range(70 + 40 * h):
            put(kind, a + int(rng.integers(0, 256)), 1, 10_240 + int(rng.integers(0, 2_048 + 1_024 * (h % 2))))
        heavy.append((kind, a, 1, 10_240, 2 + h % 2))
    return links, sites, heavy


def matelink_plan():
    """im_matelink_partner on contig 0: (kind, a0, a1) -> (n_links, mtid, n_partner, lo, hi)"""
    links, sites, heavy = mate_links()
    rng = np.random.default_rng(12)
    clen = CLENS[0]
    classes = _classes(COMMON + ("wide", "multi", "single"))
    single, multi = [s for s in sites if s[4] == 1], [s for s in sites if s[4] > 1]
    base = []
    for k, c in enumerate(classes):
        if c == "heavy":
            kind, a = heavy[k % N_HEAVY][:2]
            q = (kind, a + int(rng.integers(0, 60)), a + int(rng.integers(200, 500)))
        elif c == "empty":
            q = (k % 4, QUIET + 300 * k, QUIET + 300 * k + 500)
        elif c == "clipped":
            q = (k % 4, -700 - k, -1) if k % 2 else (k % 4, clen + 1, clen + 900 + k)
        elif c == "wide":
            q = (k % 4,) + _wide(k)
        elif c in ("multi", "single"):
            pool = multi if c == "multi" else single
            kind, a = pool[k % len(pool)][:2]
            q = (kind, a - 320, a + 320)
        else:
            kind, a = sites[k % N_SITES][:2]
            q = (kind, a - 200 + int(rng.integers(-150, 151)), a + 200 + int(rng.integers(-150, 151)))
        base.append(q)
    answer = lambda q: ic.partner(links, CLENS, 0, *q)
    return Plan("im_matelink_partner", classes, base, (np.uint8, np.int32, np.int32), (np.uint32, np.int32, np.uint32, np.int32, np.int32), answer,
                links=links, heavy=heavy, sites=sites)


# ---------------------------------------------------------------------- the read pairs of a junction (-E)

_KIND_SIDES = {v: k for k, v in jp.KIND.items()}        # kind -> (side of the lower end, side of the upper end)


def _end_near(p, side, rng):
    """an end whose window of 1 000 bases towards its reads and 32 the other way holds most of what lies within 300 bases of p"""
    return p + (300 if side == 0 else -300) + int(rng.integers(-200, 201))


def junction_pairs_plan():
    """im_junction_pairs over both tables at the driver's reach, back and min_sep, ends on one contig and on two in one call:
    (tid1, pos1, side1, tid2, pos2, side2) -> (pe1, pe2)"""
    pairs, psites, pheavy = pair_links()
    mates, msites, mheavy = mate_links()
    rng = np.random.default_rng(13)
    classes = _classes(COMMON)
    base = []

    def one(site, turn):
        tid, kind, a, b = site
        slo, shi = _KIND_SIDES[kind]
        lo, hi = (tid, _end_near(a, slo, rng), slo), (tid, _end_near(b, shi, rng), shi)
        return lo + hi if turn % 2 == 0 else hi + lo

    def two(site, turn):
        kind, a, mtid, b = site[:4]
        s1, s2 = kind & 1, kind >> 1
        e1, e2 = (0, _end_near(a, s1, rng), s1), (mtid, _end_near(b + 500, s2, rng), s2)
        return e1 + e2 if turn % 2 == 0 else e2 + e1

    for k, c in enumerate(classes):
        if c == "heavy":
            q = one(pheavy[k % N_HEAVY], k // 2) if k % 2 else two(mheavy[k % N_HEAVY], k // 2)
        elif c == "empty":
            q = (0, QUIET + 5_000 + 300 * k, k % 2, 0, QUIET + 9_000 + 300 * k, (k >> 1) % 2) if k % 2 else (0, QUIET + 5_000 + 300 * k, k % 2, 1, 30_000, (k >> 1) % 2)
        elif c == "clipped":
            q = [(0, -33 - k, 0, 0, 5_000, 1), (0, 5_000, 0, 1, CLENS[1] + 33 + k, 1), (2, CLENS[2] + 40 + k, 1, 0, 4_000, 0), (1, 900, 1, 1, -40 - k, 0)][k % 4]
        else:
            q = one(psites[k % len(psites)], k // 2) if k % 2 else two(msites[k % N_SITES], k // 2)
        base.append(q)
    answer = lambda q: jp.junction_pairs(pairs, mates, CLENS, q)
    return Plan("im_junction_pairs", classes, base, (np.int32, np.int32, np.uint8, np.int32, np.int32, np.uint8), (np.uint32, np.uint32), answer,
                pairs=pairs, mates=mates, pheavy=pheavy, mheavy=mheavy)


# ---------------------------------------------------------------------- the split links (-S, -H)

N_SPLIT = 50


def split_pairs():
    """([(link, d)], sites, heavy, unknown, twice): a site is a junction (tA, pA, sA, tB, pB, sB); its 3 .. 30 links lie within 20 bases
    of either end, stored from either end, their d around one value, one in five without; the heavy sites keep 130 .. 200 links in
    one bucket, all stored from end A; the unknown sites' links state no d; the twice sites have both ends on one contig and one side,
    20 bases apart"""
    rng = np.random.default_rng(3)
    room = [88_000, 48_000, 17_000]
    pairs, sites, heavy, unknown, twice = [], [], [], [], []

    def put(site, n, known=0.8, from_a=0.6, spread=20):
        ta, pa, sa, tb, pb, sb = site
        d0 = int(rng.integers(-12, 13))
        for _ in range(n):
            a, b = pa + int(rng.integers(-spread, spread + 1)), pb + int(rng.integers(-spread, spread + 1))
            link = (ta, a, sa, tb, b, sb) if rng.random() < from_a else (tb, b, sb, ta, a, sa)
            pairs.append((link, d0 + int(rng.integers(-1, 2)) * int(rng.random() < 0.4) if rng.random() < known else None))

    for s in range(N_SPLIT):
        ta, tb = s % 3, (s // 3) % 3
        site = (ta, 1_000 + int(rng.integers(0, room[ta])), s % 2, tb, 1_000 + int(rng.integers(0, room[tb])), (s // 2) % 2)
        put(site, int(rng.integers(3, 31)))
        sites.append(site)
    for h in range(3):
        site = (0, _heavy_pos(h) + 120, h % 2, 1 + h % 2, 9_000 + 700 * h, (h + 1) % 2)
        put(site, 130 + 35 * h, from_a=1.0)
        heavy.append(site)
    for u in range(3):
        site = (u % 2, 89_000 + 400 * u if u % 2 == 0 else 50_000 + 400 * u, u % 2, 2, 18_000 + 100 * u, 1)
        put(site, 5 + 4 * u, known=0.0)
        unknown.append(site)
    for t in range(3):
        site = (t, 19_000 + 150 * t, t % 2, t, 19_020 + 150 * t, t % 2)
        put(site, 12 + 9 * t, spread=25)
        twice.append(site)
    return pairs, sites, heavy, unknown, twice


def _turned(site, turn):
    return site if turn % 2 == 0 else site[3:6] + site[0:3]


def splitlink_plan():
    """im_splitlink_count: (tid1, side1, a0, a1, tid2, side2, b0, b1) -> (count,)"""
    pairs, sites, heavy, unknown, twice = split_pairs()
    links = [l for l, _ in pairs]
    rng = np.random.default_rng(14)
    classes = _classes(COMMON + ("wide",))
    base = []
    for k, c in enumerate(classes):
        if c == "heavy":
            ta, pa, sa, tb, pb, sb = heavy[k % 3]
            q = (ta, sa, pa - int(rng.integers(5, 40)), pa + int(rng.integers(5, 40)), tb, sb, pb - int(rng.integers(5, 40)), pb + int(rng.integers(5, 40)))
        elif c == "empty":
            q = (0, k % 2, QUIET + 300 * k, QUIET + 300 * k + 500, 1 + k % 2, (k >> 1) % 2, 0, CLENS[1 + k % 2])
        elif c == "clipped":
            ta, pa, sa, tb, pb, sb = sites[k % N_SPLIT]
            q = [(ta, sa, -700 - k, -1, tb, sb, 0, CLENS[tb]), (ta, sa, CLENS[ta] + 1, CLENS[ta] + 900, tb, sb, 0, CLENS[tb]), (ta, sa, pa - 40, pa + 40, tb, sb, CLENS[tb] + 1 + k, CLENS[tb] + 70 + k)][k % 3]
        elif c == "wide":
            inside = [x for x in sites if x[0] == 0 and 22_000 <= x[1] <= 85_000]     # end A on contig 0, inside every wide window
            ta, pa, sa, tb, pb, sb = inside[k % len(inside)]
            q = (0, sa) + _wide(k) + (tb, sb, 0, CLENS[tb])
        else:
            ta, pa, sa, tb, pb, sb = _turned((sites + twice)[k % (N_SPLIT + 3)], k // 7)
            w = int(rng.integers(8, 60))
            q = (ta, sa, pa - w, pa + w, tb, sb, pb - w, pb + w)
        base.append(q)
    answer = lambda q: (sl.count(links, CLENS, q),)
    return Plan("im_splitlink_count", classes, base, (np.int32, np.uint8, np.int32, np.int32, np.int32, np.uint8, np.int32, np.int32), (np.uint32,), answer,
                pairs=pairs, links=links, heavy=heavy)


def overlap_plan():
    """im_splitlink_overlap at the driver's window: (tid1, pos1, side1, tid2, pos2, side2) -> (known, median, agree)"""
    pairs, sites, heavy, unknown, twice = split_pairs()
    rng = np.random.default_rng(15)
    classes = _classes(COMMON + ("unknown", "twice"))
    base = []
    for k, c in enumerate(classes):
        jitter = lambda: int(rng.integers(-6, 7))
        if c == "empty":
            q = (0, QUIET + 300 * k, k % 2, 1 + k % 2, (30_000 if k % 2 == 0 else 15_000) - 100 * k, (k >> 1) % 2)
        elif c == "clipped":
            ta, pa, sa, tb, pb, sb = sites[k % N_SPLIT]
            q = [(ta, -33 - k, sa, tb, pb, sb), (ta, pa, sa, tb, CLENS[tb] + 33 + k, sb), (tb, CLENS[tb] + 40 + k, sb, ta, -40, sa)][k % 3]
        else:
            pool = {"heavy": heavy, "unknown": unknown, "twice": twice}.get(c, sites)
            ta, pa, sa, tb, pb, sb = _turned(pool[k % len(pool)], k // 5)
            q = (ta, pa + jitter(), sa, tb, pb + jitter(), sb)
        base.append(q)
    answer = lambda q: so.junction_summary(pairs, CLENS, q, OVERLAP_WINDOW)
    return Plan("im_splitlink_overlap", classes, base, (np.int32, np.int32, np.uint8, np.int32, np.int32, np.uint8), (np.uint32, np.int32, np.uint32), answer,
                pairs=pairs, heavy=heavy, unknown=unknown, twice=twice)


# ---------------------------------------------------------------------- the clip tails (-V, -I, -T)

N_PILES, N_JUNCTIONS = 40, 30


def tail_table():
    """({(tid, side, position): [bases]}, verify sites [(pr, pl)] of contig 0, junction sites [(t1, p1, s1, t2, p2, s2)], heavy verify
    sites, heavy junction sites): a pile holds 3 .. 40 entries of 20 .. 32 bases (a heavy one 130 .. 190), seven in ten of them the
    reference at the other end at the site's shift with a difference now and then, the others random"""
    rng = np.random.default_rng(4)
    R = refs()
    table, verify, junctions, vheavy, jheavy = {}, [], [], [], []
    code = {ord(c): k for k, c in enumerate("ACGT")}

    def pile(key, n, expect):
        """n entries at key; expect(i): the character base i should be, or None"""
        out = table.setdefault(key, [])
        for _ in range(n):
            nb = int(rng.integers(20, 33))
            if rng.random() < 0.7:
                b = [code.get(ord(expect(i) or "A"), 0) for i in range(nb)]
                if rng.random() < 0.5:
                    b[int(rng.integers(0, nb))] ^= 1 + int(rng.integers(0, 3))
            else:
                b = [int(x) for x in rng.integers(0, 4, nb)]
            out.append(tuple(b))

    def verify_site(pr, pl, n):
        s = int(rng.integers(0, 33))
        at = lambda p: chr(R[0][p]) if 0 <= p < CLENS[0] and R[0][p] in code else None
        pile((0, ct.RIGHT, pr), n(), lambda i: at(pl + s + i))
        pile((0, ct.LEFT, pl), n(), lambda i: at(pr - 1 - s - i))

    def junction_site(j, n):
        t1, p1, s1, t2, p2, s2 = j
        s, same = int(rng.integers(0, 33)), s1 == s2
        pile((t1, s1, p1), n(), lambda i: ic.expected(R[t2], p2, s2, same, s, i))
        pile((t2, s2, p2), n(), lambda i: ic.expected(R[t1], p1, s1, same, s, i))

    few = lambda: int(rng.integers(3, 41))
    for s in range(N_PILES):
        pr = _site_pos(s) + 1_000
        pl = pr + int(rng.integers(100, 900))
        verify_site(pr, pl, few)
        verify.append((pr, pl))
    for s in range(N_JUNCTIONS):
        t1, t2 = s % 3, (s // 3 + 1) % 3
        j = (t1, 3_100 + 550 * s, s % 2, t2, 1_700 + 570 * s, (s // 2) % 2)     # below 20 000: inside every contig, off the verify sites
        junction_site(j, few)
        junctions.append(j)
    for h in range(3):
        pr = _heavy_pos(h) + 77
        verify_site(pr, pr + 300 + 50 * h, lambda: HEAVY_TAILS + 30 * h)
        vheavy.append((pr, pr + 300 + 50 * h))
    for h in range(2):
        j = (0, 96_000 + 500 * h, h, 1 + h, 55_000 - 40_000 * h, 1)
        junction_site(j, lambda: HEAVY_TAILS + 5 + 25 * h)
        jheavy.append(j)
    return table, verify, junctions, vheavy, jheavy


def verify_plan():
    """im_cliptail_verify on contig 0 at max_shift 32: (pr, pl) -> (v_right, v_left, shift, stored_right, stored_left)"""
    table, verify, junctions, vheavy, jheavy = tail_table()
    clen, ref = CLENS[0], refs()[0]
    classes = _classes(COMMON)
    base = []
    for k, c in enumerate(classes):
        if c == "heavy":
            q = vheavy[k % 3] if k % 4 != 3 else (vheavy[0][0], vheavy[1 + k % 2][1])
        elif c == "empty":
            q = (QUIET + 7 * k, QUIET + 7 * k + 500)
        elif c == "clipped":
            q = [(-5 - k, verify[k % N_PILES][1]), (verify[k % N_PILES][0], clen + 1 + k), (-9, clen + 9), verify[k % N_PILES][::-1]][k % 4]
        else:
            q = verify[k % N_PILES] if k % 5 else (verify[k % N_PILES][0], verify[(k + 3) % N_PILES][1])
        base.append(tuple(q))
    answer = lambda q: ct.answer(table, ref, 0, *q)
    return Plan("im_cliptail_verify", classes, base, (np.int32, np.int32), (np.uint32, np.uint32, np.int32, np.uint32, np.uint32), answer,
                table=table, heavy=vheavy)


def consensus_plan():
    """im_cliptail_consensus on contig 0 at min_cover MIN_COVER: (pos, side) -> (entries, len, low plane, high plane, agree)"""
    table, verify, junctions, vheavy, jheavy = tail_table()
    clen = CLENS[0]
    classes = _classes(COMMON)
    base = []
    for k, c in enumerate(classes):
        if c == "heavy":
            q = (vheavy[k % 3][k % 2], k % 2)
        elif c == "empty":
            q = (QUIET + 7 * k, k % 2) if k % 2 else (verify[k % N_PILES][0], ct.LEFT)         # the other side of a pile's position holds nothing
        elif c == "clipped":
            q = (-1 - k, k % 2) if k % 2 else (clen + 1 + k, (k >> 1) % 2)
        else:
            q = (verify[k % N_PILES][k % 2], k % 2)
        base.append(q)
    answer = lambda q: fp.answer(table, 0, q[0], q[1], MIN_COVER, clen)
    return Plan("im_cliptail_consensus", classes, base, (np.int32, np.uint8), (np.uint32, np.uint32, np.uint32, np.uint32, np.uint32), answer,
                table=table, heavy=vheavy)


def junction_plan():
    """im_cliptail_junction at max_shift 32: (tid1, p1, side1, tid2, p2, side2) -> (v1, v2, shift, stored1, stored2)"""
    table, verify, junctions, vheavy, jheavy = tail_table()
    R = refs()
    classes = _classes(COMMON)
    base = []
    for k, c in enumerate(classes):
        if c == "heavy":
            q = _turned(jheavy[k % 2], k // 2) if k % 3 else (0, vheavy[k % 3][0], ct.RIGHT, 0, vheavy[k % 3][1], ct.LEFT)
        elif c == "empty":
            q = (0, QUIET + 7 * k, k % 2, 1 + k % 2, 40_000 - 300 * k if k % 2 == 0 else 19_900 - k, (k >> 1) % 2)
        elif c == "clipped":
            j = junctions[k % N_JUNCTIONS]
            q = [(j[0], -3 - k, j[2]) + j[3:], j[:3] + (j[3], CLENS[j[3]] + 5 + k, j[5]), (2, CLENS[2] + 1, 0, 1, -1, 1)][k % 3]
        else:
            q = _turned(junctions[k % N_JUNCTIONS], k // 3)
            if k % 6 == 5:
                q = q[:3] + _turned(junctions[(k + 1) % N_JUNCTIONS], k // 3)[3:]             # ends of two sites: stored, not matching
        base.append(tuple(q))
    answer = lambda q: ic.junction(table, R, *q)
    return Plan("im_cliptail_junction", classes, base, (np.int32, np.int32, np.uint8, np.int32, np.int32, np.uint8), (np.uint32, np.uint32, np.int32, np.uint32, np.uint32), answer,
                table=table, heavy=jheavy)


def tail_entries(table):
    """{tid: (pos, side, nbases, planes[n, 2])} of a table: what im_cliptail_add takes, contig by contig"""
    out = {}
    for tid in range(len(CLENS)):
        rows = [(p, side, len(b)) + ct.planes_of(b) for (t, side, p), es in sorted(table.items()) if t == tid for b in es]
        if rows:
            a = np.array(rows, np.int64)
            out[tid] = (a[:, 0].astype(np.int32), a[:, 1].astype(np.uint8), a[:, 2].astype(np.uint8), a[:, 3:5].astype(np.uint32))
    return out


PLANS = {"im_pairlink_count": pairlink_plan, "im_matelink_partner": matelink_plan, "im_splitlink_count": splitlink_plan,
         "im_splitlink_overlap": overlap_plan, "im_junction_pairs": junction_pairs_plan, "im_cliptail_verify": verify_plan,
         "im_cliptail_consensus": consensus_plan, "im_cliptail_junction": junction_plan}
_PLANS = {}


def plan(name):
    """the plan of one entry point, built once"""
    if name not in _PLANS:
        _PLANS[name] = PLANS[name]()
    return _PLANS[name]
