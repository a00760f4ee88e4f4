"""tests/support/manyqueries.py, pinned where no GPU is needed: the tiling is what it says, every base query is of the class its name
states, the waves that make a second and a third trip meet the classes in the orders in which leftover state would show, no fill
overflows its table, and the restatements agree with their faster forms on the base sets."""
import numpy as np
import pytest

from tests.support import cliptails as ct
from tests.support import intercontig as ic
from tests.support import junctionpairs as jp
from tests.support import manyqueries as mq
from tests.support import splitlinks as sl
from tests.support import splitoverlap as so

WITH_WINDOWS = ("im_pairlink_count", "im_matelink_partner", "im_splitlink_count")        # the entries that take a window per query
ZERO = {"im_pairlink_count": (0,), "im_splitlink_count": (0,), "im_matelink_partner": (0, -1, 0, 0, 0), "im_splitlink_overlap": (0, 0, 0),
        "im_junction_pairs": (0, 0), "im_cliptail_consensus": (0, 0, 0, 0, 0)}


def test_the_tiling_and_the_trips():
    assert mq.D == 97 and all(mq.D % p for p in range(2, 10)) and mq.TRIP == 8192 and mq.TRIP % mq.D == mq.STEP == 44
    assert mq.SIZES == [8192, 8193, 16385, 20011]
    base = list(range(100, 100 + mq.D))
    for nq in (1, 96, 97, 98, 8193):
        assert mq.tile(base, nq) == [base[i % mq.D] for i in range(nq)]
        assert np.array_equal(mq.tile(np.array(base), nq), np.array(base)[np.arange(nq) % mq.D])
    assert mq.rotate(base) == base[1:] + base[:1] and np.array_equal(mq.rotate(np.array(base)), np.array(base[1:] + base[:1]))
    assert mq.trips(8192) == [] and mq.trips(8193) == [(0, 44)]
    t = mq.trips(16385)
    assert len(t) == 8192 and t[0] == (0, 44, 88) and t[1] == (1, 45) and all(len(x) == 2 for x in t[1:])
    t = mq.trips(20011)
    assert len(t) == 8192 and sum(len(x) == 3 for x in t) == 20011 - 16384 and t[20011 - 16384 - 1] == tuple(i % mq.D for i in (3626, 3626 + 8192, 20010))
    assert all(b == (a + mq.STEP) % mq.D for x in t for a, b in zip(x, x[1:]))
    assert {a for x in mq.trips(16385) for a in x[:1]} == set(range(mq.D))                  # every base query is some wave's first of two


@pytest.mark.parametrize("name", sorted(mq.PLANS))
def test_the_columns_are_the_tiled_base_set(name):
    P = mq.plan(name)
    assert len(P.base) == len(P.classes) == len(P.answers()) == mq.D and len(set(P.base)) > 40
    for nq, by in ((8193, 0), (8193, 1), (20011, 0)):
        qs, want = P.columns(nq, by)
        assert all(len(c) == nq and c.dtype == t for c, t in zip(qs, P.kinds)) and all(len(c) == nq and c.dtype == t for c, t in zip(want, P.out_kinds))
        base, answers = mq.rotate(P.base, by), mq.rotate(P.answers(), by)
        for i in (0, 1, 96, 97, 8191, 8192, nq - 1):
            assert tuple(int(c[i]) for c in qs) == base[i % mq.D] and tuple(int(c[i]) for c in want) == answers[i % mq.D]
    assert [tuple(int(c[i]) for c in P.columns(97)[1]) for i in range(mq.D)] == P.answers()         # nothing is lost in a column's type


@pytest.mark.parametrize("name", sorted(mq.PLANS))
def test_the_trips_meet_the_classes_in_the_orders_that_show_leftover_state(name):
    P = mq.plan(name)
    need = [t for t in mq.TRANSITIONS if set(t) <= set(P.classes)]
    assert set(mq.TRANSITIONS[:4]) <= set(need)
    assert (("wide", "ordinary") in need) == (name in WITH_WINDOWS) and (("multi", "single") in need) == (name == "im_matelink_partner")
    seen = set()
    for nq in mq.SIZES:
        seen |= mq.transitions(P.classes, nq)
    assert set(need) <= seen, set(need) - seen
    assert mq.transitions(P.classes, 8192) == set()
    # the one wave on a second trip at 8 193, as asked and rotated by one; the one on a third trip at 16 385
    assert mq.transitions(P.classes, 8193) == {("heavy", "empty")} == mq.transitions(P.classes, 8193, 1)
    assert [P.classes[i] for i in mq.trips(16385)[0]] == ["heavy", "empty", "heavy"]
    assert set(need) <= mq.transitions(P.classes, 16385) and set(need) <= mq.transitions(P.classes, 20011)


def _bucket_counts(keys):
    out = {}
    for k in keys:
        out[k] = out.get(k, 0) + 1
    return out


def _clip(a0, a1, clen):
    return max(a0, 0), min(a1, clen)


def _empty_after_clip(a0, a1, clen):
    a0, a1 = _clip(a0, a1, clen)
    return a0 > a1


def _zero(name, answer):
    return answer[:3] == (0, 0, -1) if name in ("im_cliptail_verify", "im_cliptail_junction") else answer == ZERO[name]


def _heaviest(name, P, q):
    """the most entries one key holds among the keys that query q walks"""
    if name == "im_pairlink_count":
        n = _bucket_counts((t, k, p >> 8) for t, k, p, _ in P.links)
        return max(n.get((0, q[0], b), 0) for b in range(q[1] >> 8, (q[2] >> 8) + 1))
    if name == "im_matelink_partner":
        n = _bucket_counts((t, k, p >> 8) for t, k, p, _, _ in P.links)
        return max(n.get((0, q[0], b), 0) for b in range(q[1] >> 8, (q[2] >> 8) + 1))
    if name == "im_splitlink_count":
        n = _bucket_counts((ta, sa | sb << 1, pa >> 8) for ta, pa, sa, tb, pb, sb in P.links)
        return max(n.get((q[0], q[1] | q[5] << 1, b), 0) for b in range(max(q[2], 0) >> 8, (q[3] >> 8) + 1))
    if name == "im_splitlink_overlap":
        n = _bucket_counts((ta, sa | sb << 1, pa >> 8) for (ta, pa, sa, tb, pb, sb), _ in P.pairs)
        w = mq.OVERLAP_WINDOW
        return max(n.get((t, s | s2 << 1, b), 0) for t, p, s, s2 in ((q[0], q[1], q[2], q[5]), (q[3], q[4], q[5], q[2])) for b in range((p - w) >> 8, ((p + w) >> 8) + 1))
    if name == "im_junction_pairs":
        if q[0] == q[3]:
            n = _bucket_counts((t, k, p >> 8) for t, k, p, _ in P.pairs)
            (plo, slo), (phi, shi) = sorted([(q[1], q[2]), (q[4], q[5])], key=lambda e: e[0]) if q[1] != q[4] else [(q[1], q[2]), (q[4], q[5])]
            w = jp.window(plo, slo, mq.CLENS[q[0]])
            return max(n.get((q[0], jp.KIND[(slo, shi)], b), 0) for b in range(w[0] >> 8, (w[1] >> 8) + 1))
        n = _bucket_counts((t, k, p >> 8) for t, k, p, _, _ in P.mates)
        w1, w2 = jp.window(q[1], q[2], mq.CLENS[q[0]]), jp.window(q[4], q[5], mq.CLENS[q[3]])
        return max([n.get((q[0], q[2] | q[5] << 1, b), 0) for b in range(w1[0] >> 8, (w1[1] >> 8) + 1)] +
                   [n.get((q[3], q[5] | q[2] << 1, b), 0) for b in range(w2[0] >> 8, (w2[1] >> 8) + 1)])
    if name == "im_cliptail_verify":
        return max(len(P.table.get((0, ct.RIGHT, q[0]), [])), len(P.table.get((0, ct.LEFT, q[1]), [])))
    if name == "im_cliptail_consensus":
        return len(P.table.get((0, q[1], q[0]), []))
    return max(len(P.table.get((q[0], q[2], q[1]), [])), len(P.table.get((q[3], q[5], q[4]), [])))


def _clipped_away(name, q):
    L = mq.CLENS
    if name == "im_pairlink_count":
        return _empty_after_clip(q[1], q[2], L[0]) or _empty_after_clip(q[3], q[4], L[0])
    if name == "im_matelink_partner":
        return _empty_after_clip(q[1], q[2], L[0])
    if name == "im_splitlink_count":
        return _empty_after_clip(q[2], q[3], L[q[0]]) or _empty_after_clip(q[6], q[7], L[q[4]])
    if name == "im_splitlink_overlap":
        w = mq.OVERLAP_WINDOW
        return _empty_after_clip(q[1] - w, q[1] + w, L[q[0]]) or _empty_after_clip(q[4] - w, q[4] + w, L[q[3]])
    if name == "im_junction_pairs":
        return jp.window(q[1], q[2], L[q[0]]) is None or jp.window(q[4], q[5], L[q[3]]) is None
    if name == "im_cliptail_verify":
        return not 0 <= q[0] <= L[0] or not 0 <= q[1] <= L[0] or q[1] <= q[0]
    if name == "im_cliptail_consensus":
        return not 0 <= q[0] <= L[0]
    return not 0 <= q[1] <= L[q[0]] or not 0 <= q[4] <= L[q[3]]


@pytest.mark.parametrize("name", sorted(mq.PLANS))
def test_every_base_query_is_of_the_class_its_name_states(name):
    P = mq.plan(name)
    tails = name.startswith("im_cliptail") or name == "im_splitlink_overlap"
    need = mq.HEAVY_TAILS if tails else mq.HEAVY_LINKS
    want = {"heavy", "ordinary", "empty", "clipped"} | ({"wide"} if name in WITH_WINDOWS else set())
    want |= {"multi", "single"} if name == "im_matelink_partner" else {"unknown", "twice"} if name == "im_splitlink_overlap" else set()
    assert set(P.classes) == want and all(P.classes.count(c) >= 3 for c in want)
    assert P.classes[0] == "heavy" and P.classes[mq.STEP] == "empty" and P.classes[1] == "heavy" and P.classes[1 + mq.STEP] == "empty"
    for k, (c, q, a) in enumerate(zip(P.classes, P.base, P.answers())):
        what = (name, k, c, q, a)
        if c == "heavy":
            assert _heaviest(name, P, q) >= need and not _clipped_away(name, q), what
            assert not _zero(name, a) or (name == "im_cliptail_verify" and min(a[-2:]) >= need), what     # or two heavy piles that do not match
        elif c == "empty":
            assert _zero(name, a) and not _clipped_away(name, q), what
            if name.startswith("im_cliptail"):
                assert a[-2:] == (0, 0) or name == "im_cliptail_consensus", what           # nothing stored at either key
        elif c == "clipped":
            assert _clipped_away(name, q) and _zero(name, a), what
        elif c == "wide":
            a0, a1 = (q[1], q[2]) if name != "im_splitlink_count" else (q[2], q[3])
            assert a1 - a0 == 65_535 and (a1 >> 8) - (a0 >> 8) + 1 == 257 and 0 <= a0 and a1 <= mq.CLENS[0] and a[0] > 0, what
        elif c in ("multi", "single"):
            a0, a1 = _clip(q[1], q[2], mq.CLENS[0])
            cells = {(mt, m >> ic.CELL_SHIFT) for t, kd, p, mt, m in P.links if t == 0 and kd == q[0] and a0 <= p <= a1}
            assert (len(cells) > 2 and a[0] > a[2] > 0) if c == "multi" else (len(cells) == 1 and a[0] == a[2] > 0), what
        elif c == "unknown":
            assert a == (0, 0, 0) and len(so.junction_ds(P.pairs, mq.CLENS, q, mq.OVERLAP_WINDOW)) >= 5, what
        elif c == "twice":
            w = mq.OVERLAP_WINDOW
            q1 = (q[0], q[2], q[1] - w, q[1] + w, q[3], q[5], q[4] - w, q[4] + w)
            q2 = q1[4:] + q1[:4]
            both = [l for l, _ in P.pairs if sl.count([l], mq.CLENS, q1) and sl.count([l], mq.CLENS, q2)]
            assert q[0] == q[3] and q[2] == q[5] and len(both) >= 3 and a[0] > 0, what
        else:
            assert not _clipped_away(name, q), what
    ordinary = [a for c, a in zip(P.classes, P.answers()) if c == "ordinary"]
    assert sum(1 for a in ordinary if not _zero(name, a)) > len(ordinary) * 2 // 3 and len(set(ordinary)) > len(ordinary) // 3
    if name == "im_pairlink_count":
        assert {q[0] for q, a in zip(P.base, P.answers()) if a[0] > 0} == {0, 1, 2, 3}                # every kind, the stretched one too
    if name == "im_junction_pairs":
        live = [q for q, a in zip(P.base, P.answers()) if a != (0, 0)]
        assert sum(q[0] == q[3] for q in live) > 15 and sum(q[0] != q[3] for q in live) > 15 and any(a[1] > 0 for a in P.answers())
    if name == "im_cliptail_verify":
        assert sum(1 for a in P.answers() if a[0] > 0 and a[1] > 0 and a[2] > 0) > 20


def test_no_fill_overflows_its_table():
    half = {k: 1 << (v - 1) for k, v in mq.LOG2_SLOTS.items()}
    pairs, mates = mq.pair_links()[0], mq.mate_links()[0]
    split, table = mq.split_pairs()[0], mq.tail_table()[0]
    L = mq.CLENS
    assert 1_500 < len(pairs) <= half["pair"] and 2_000 < len(mates) <= half["mate"] and 1_000 < len(split) <= half["split"]
    assert 3_000 < sum(len(es) for es in table.values()) <= half["tail"]
    assert all(12 <= v <= 14 for v in mq.LOG2_SLOTS.values()) and len(L) == 3 and all(20_000 <= n <= 150_000 for n in L)
    # every entry is one the _add entries store: inside its contigs
    assert all(0 <= p <= L[t] and 0 <= m <= L[t] and 0 <= k <= 3 for t, k, p, m in pairs)
    assert all(0 <= p <= L[t] and 0 <= m <= L[mt] and mt != t for t, k, p, mt, m in mates)
    assert all(0 <= pa <= L[ta] and 0 <= pb <= L[tb] for (ta, pa, sa, tb, pb, sb), _ in split) and any(d is None for _, d in split)
    assert all(0 <= p <= L[t] and all(1 <= len(b) <= 32 for b in es) for (t, side, p), es in table.items())
    entries = mq.tail_entries(table)
    assert sum(len(e[0]) for e in entries.values()) == sum(len(es) for es in table.values()) and sorted(entries) == [0, 1, 2]
    # nothing lies where the empty windows are
    assert not any(t == 0 and p >= mq.QUIET for t, k, p, m in pairs) and not any(t == 0 and p >= mq.QUIET for t, k, p, mt, m in mates)
    assert not any((ta == 0 and pa >= mq.QUIET) or (tb == 0 and pb >= mq.QUIET) for (ta, pa, sa, tb, pb, sb), _ in split)
    assert not any(t == 0 and p >= mq.QUIET for t, side, p in table)


def test_the_restatements_agree_with_their_faster_forms_on_the_base_sets():
    P = mq.plan("im_junction_pairs")
    assert jp.answers(P.pairs, P.mates, mq.CLENS, P.base) == jp.answers_fast(P.pairs, P.mates, mq.CLENS, P.base) == P.answers()
    P = mq.plan("im_splitlink_overlap")
    assert so.summaries_fast(P.pairs, mq.CLENS, P.base, mq.OVERLAP_WINDOW) == P.answers()
    P = mq.plan("im_cliptail_verify")
    assert ct.answer_many(P.table, mq.refs()[0], 0, [q[0] for q in P.base], [q[1] for q in P.base]) == P.answers()
